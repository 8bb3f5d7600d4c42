"""CPU: the host side of pixel-level metrics - ground-truth masks in the prepared dataset (prepare_mvtec_data --with-masks),
mask loading for the evaluator, the evaluator's new flags, and the argument checks of the new C entry points."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image


def _source_tree(root, size=40):
    """An MVTec-layout source: <cls>/train/good, <cls>/test/{good,<defect>}, <cls>/ground_truth/<defect>/<stem>_mask.png.
    One defective image (grid/test/bent/001) has no mask."""
    rng = np.random.RandomState(3)
    for cls in ("carpet", "grid"):
        for sub, names in (("train/good", ["000", "001", "002"]), ("test/good", ["000"]), ("test/crack", ["000", "001"]),
                           ("test/bent", ["000", "001"])):
            d = root / cls / sub
            d.mkdir(parents=True)
            for n in names:
                Image.fromarray(rng.randint(0, 256, (size, size, 3), dtype=np.uint8)).save(d / f"{n}.png")
        for defect, names in (("crack", ["000", "001"]), ("bent", ["000", "001"] if cls == "carpet" else ["000"])):
            d = root / cls / "ground_truth" / defect
            d.mkdir(parents=True)
            for n in names:
                m = np.zeros((size, size), np.uint8)
                m[rng.randint(0, size // 2):, rng.randint(0, size // 2):rng.randint(size // 2 + 1, size)] = 255
                Image.fromarray(m).save(d / f"{n}_mask.png")


def test_prepare_with_masks(tmp_path, capsys):
    from srad_amd import prepare_mvtec_data as P
    src = tmp_path / "mvtec"
    _source_tree(src)
    P.prepare_mvtec_dataset(str(src), str(tmp_path / "plain"), scale_factors=(2, 4), target_hr=(32, 32), val_ratio=0.34, seed=42)
    assert not list((tmp_path / "plain").rglob("GT"))                     # the default writes no masks
    capsys.readouterr()
    dst = tmp_path / "masked"
    P.prepare_mvtec_dataset(str(src), str(dst), scale_factors=(2, 4), target_hr=(32, 32), val_ratio=0.34, seed=42, with_masks=True)
    text = capsys.readouterr().out
    assert "WARNING no ground-truth mask for bent/001.png" in text
    for cls in ("carpet", "grid"):
        bad = dst / cls / "test" / "bad"
        hr_names = sorted(p.name for p in (bad / "HR").glob("*.png"))
        gt_names = sorted(p.name for p in (bad / "GT").glob("*.png"))
        assert hr_names == ["bent_000.png", "bent_001.png", "crack_000.png", "crack_001.png"]
        assert gt_names == (hr_names if cls == "carpet" else ["bent_000.png", "crack_000.png", "crack_001.png"])
        for n in gt_names:
            gt, hr = np.array(Image.open(bad / "GT" / n)), np.array(Image.open(bad / "HR" / n))
            assert gt.shape == hr.shape[:2] == (32, 32) and gt.dtype == np.uint8
            assert set(np.unique(gt)) <= {0, 255} and gt.max() == 255
        assert not (dst / cls / "test" / "good" / "GT").exists()
    # everything but GT/ is what the default call writes
    plain = sorted(str(p.relative_to(tmp_path / "plain")) for p in (tmp_path / "plain").rglob("*.png"))
    masked = sorted(str(p.relative_to(dst)) for p in dst.rglob("*.png") if "/GT/" not in str(p))
    assert plain == masked


def test_cli_flag_with_masks(tmp_path):
    from srad_amd import prepare_mvtec_data as P
    src = tmp_path / "mvtec"
    _source_tree(src)
    assert P.main(["--hr-size", "32", "--source", str(src), "--target", str(tmp_path / "out"), "--with-masks"]) == 0
    assert len(list((tmp_path / "out" / "carpet" / "test" / "bad" / "GT").glob("*.png"))) == 4


def test_load_masks(tmp_path):
    from srad_amd import evaluate as E
    gt = tmp_path / "grid" / "test" / "bad" / "GT"
    gt.mkdir(parents=True)
    m = np.zeros((40, 40), np.uint8)
    m[30:, 5:9] = 255
    m[:20, 36:] = 255                                                      # outside the 32 x 32 crop
    Image.fromarray(m).save(gt / "crack_000.png")
    Image.fromarray(np.zeros((16, 16), np.uint8)).save(gt / "small.png")  # smaller than the HR image: unusable
    names = [("good", "000"), ("bad", "crack_000"), ("bad", "hole_000"), ("bad", "small")]
    masks, missing = E.load_masks(str(tmp_path), "grid", names, [(32, 32)] * 4)
    assert masks[0].shape == (32, 32) and masks[0].dtype == np.uint8 and not masks[0].any()
    assert masks[1].shape == (32, 32) and np.array_equal(masks[1], (m[:32, :32] != 0).astype(np.uint8)) and masks[1].sum() == 8
    assert masks[2] is None and masks[3] is None and missing == ["hole_000", "small"]


def test_eval_flags_default_off():
    from srad_amd import options as Opt
    a = Opt.parse_eval_args([])
    assert a.pixel_metrics is False and a.save_anomaly_maps is False and a.map_ws == 0
    a = Opt.parse_eval_args(["--pixel-metrics", "--save-anomaly-maps", "--map-ws", "13"])
    assert a.pixel_metrics and a.save_anomaly_maps and a.map_ws == 13


def test_argument_errors_of_the_new_entry_points_without_gpu():
    from srad_amd import _lib as L
    lib = L.lib()
    nb = C.c_size_t()
    assert lib.srad_anomaly_map_workspace_bytes(0, 32, 32, C.byref(nb)) != 0
    assert lib.srad_anomaly_map_workspace_bytes(2, 32, 32, C.byref(nb)) == 0 and nb.value >= 2 * 33 * 33 * 5 * 8
    assert lib.srad_pixel_auc_workspace_bytes(C.c_int64(0), C.byref(nb)) != 0
    assert lib.srad_pixel_auc_workspace_bytes(C.c_int64(1 << 31), C.byref(nb)) != 0
    assert lib.srad_pixel_auc_workspace_bytes(C.c_int64(1000), C.byref(nb)) == 0 and nb.value >= 16 * 1000
    fake = C.c_void_p(4096)                                                # never dereferenced: the checks come first
    big = C.c_size_t(1 << 40)
    # a window that needs two reflections of a 33 x 40 image, and n = 0 / no window
    assert lib.srad_anomaly_maps(fake, fake, 1, 33, 40, 1, 67, fake, fake, big, None) != 0
    assert b"more than one reflection" in lib.srad_last_error()
    assert lib.srad_anomaly_maps(fake, fake, 0, 33, 40, 1, 3, fake, fake, big, None) != 0
    assert lib.srad_anomaly_maps(fake, fake, 1, 33, 40, 2, 3, fake, fake, big, None) != 0
    assert b"channels" in lib.srad_last_error()
    assert lib.srad_anomaly_maps(fake, fake, 1, 33, 40, 1, 0, fake, fake, big, None) != 0
    assert lib.srad_anomaly_maps(fake, fake, 1, 33, 40, 1, 3, fake, fake, C.c_size_t(16), None) != 0
    assert b"workspace" in lib.srad_last_error()
    assert lib.srad_pixel_roc_auc(fake, fake, C.c_int64(0), fake, fake, fake, big, None) != 0
    assert lib.srad_pixel_roc_auc(fake, fake, C.c_int64(100), fake, fake, fake, C.c_size_t(16), None) != 0
    assert b"workspace" in lib.srad_last_error()
    assert lib.srad_pixel_roc_auc(None, fake, C.c_int64(100), fake, fake, fake, big, None) != 0
