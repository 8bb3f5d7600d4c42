"""GPU: the evaluator's pixel level (anomaly maps + exact pixel ROC-AUC against ground-truth masks) end to end, against the
same pipeline run through the CPU oracle, and the evaluation CLI with --pixel-metrics / --save-anomaly-maps on a prepared tree."""
import numpy as np
import pytest
import torch
from PIL import Image

from oracle import scorer_ref as O
from oracle import sr_ref as R
from srad_amd import spec as S
from tests.test_gpu_anomaly_maps import blob_masks, map_oracle
from tests.test_gpu_pixel_auc import mann_whitney_auc

pytestmark = pytest.mark.gpu


def _pairs_and_masks(n_good, n_bad, hr_size, scale, ch, seed=3):
    y, sr, hr = O.synth_pairs(n_good, n_bad, hr_size, ch, seed=seed)
    pairs = []
    for s_img, h_img in zip(sr, hr):                         # the LR input carries the planted blob of the bad images
        lr = s_img.reshape(hr_size // scale, scale, hr_size // scale, scale, ch).astype(np.float32).mean((1, 3))
        pairs.append((np.clip(np.rint(lr), 0, 255).astype(np.uint8), h_img))
    masks = [m.astype(np.uint8) for m in blob_masks(n_good, n_bad, hr_size, ch, seed=seed)]
    return y, pairs[:n_good], pairs[n_good:], masks


def _model(model_type, hr_size, scale):
    from srad_amd import options as Opt
    from srad_amd.model import Model
    opt = Opt.build_opt(model_type, 'grid', hr_size, scale)
    opt.use_graph = False
    if model_type == 'drct':
        opt.depths, opt.num_heads = (6,), (6,)
        cfg = S.DRCTConfig(in_chans=1, img_size=16, window_size=4, upscale=4, n_rdg=1)
        sd = S.synth_state(S.drct_spec(cfg), seed=9, gain=0.7, cfg=cfg)
    else:
        cfg = S.DRNConfig.for_scale(4, 1)
        sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    model = Model(opt, None, dual_model=(model_type == 'drn-l'))
    model.get_model().load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return opt, model, cfg, sd


@pytest.mark.parametrize("model_type", ["drct", "drn-l"])
def test_pixel_auc_matches_oracle_pipeline(model_type):
    from srad_amd import evaluate as E
    scale, hr_size = 4, 64
    opt, model, cfg, sd = _model(model_type, hr_size, scale)
    y, good, bad, masks = _pairs_and_masks(6, 8, hr_size, scale, 1)
    plain = E.evaluate_on_test(opt, model, good, bad)
    got = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True)
    for k in ("best_ws", "auc_ssim", "auc_mse", "auc_psnr", "n_images", "window_sizes"):
        assert got[k] == plain[k], k
    assert set(got) - set(plain) == {"auc_pixel", "map_ws"}
    sr_u8, hr_u8 = [], []
    with torch.no_grad():
        for lr, hr in good + bad:
            x = torch.from_numpy(lr).permute(2, 0, 1)[None].float()
            out = R.drct_forward(sd, x, cfg) if model_type == 'drct' else R.drn_forward(sd, x, cfg)[-1]
            sr_u8.append(np.transpose(O.to_u8_trunc(out.numpy()[0]), (1, 2, 0)))
            hr_u8.append(hr)
    ref = O.evaluate_pairs(y, sr_u8, hr_u8)
    assert got["map_ws"] == ref["best_ws"] == got["best_ws"]
    ref_maps = np.stack([map_oracle(s, h, ref["best_ws"]) for s, h in zip(sr_u8, hr_u8)])
    ref_auc = mann_whitney_auc(ref_maps.ravel(), np.stack(masks).ravel())
    assert abs(got["auc_pixel"] - ref_auc) <= 0.002, (got["auc_pixel"], ref_auc)      # north_star: AUC within +-0.002
    # an explicit window size, and a missing mask skips the pixel AUC without failing the run
    other = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True, map_ws=3)
    assert other["map_ws"] == 3 and 0.0 <= other["auc_pixel"] <= 1.0
    holey = list(masks)
    holey[-1] = None
    skipped = E.evaluate_on_test(opt, model, good, bad, masks=holey, pixel_metrics=True)
    assert "auc_pixel" not in skipped and skipped["auc_ssim"] == plain["auc_ssim"]


def _write_prepared_tree(root, n_good, n_bad, size, scale):
    y, good, bad, masks = _pairs_and_masks(n_good, n_bad, size, scale, 1, seed=12)
    names = []
    for split, items, off in (("good", good, 0), ("bad", bad, n_good)):
        for k, (lr, hr) in enumerate(items):
            name = f"{'crack_' if split == 'bad' else ''}{k:03d}"
            base = root / "grid" / "test" / split
            lr2 = hr.reshape(size // 2, 2, size // 2, 2, 1).astype(np.float32).mean((1, 3)).round().astype(np.uint8)
            for sub, img in (("HR", hr), ("LR_2", lr2), (f"LR_{scale}", lr)):     # DRN-L x4 reads the x2 level too
                (base / sub).mkdir(parents=True, exist_ok=True)
                Image.fromarray(img[:, :, 0]).save(base / sub / f"{name}.png")
            if split == "bad":
                (base / "GT").mkdir(parents=True, exist_ok=True)
                Image.fromarray(masks[off + k] * 255).save(base / "GT" / f"{name}.png")
            names.append((split, name))
    return names


def test_cli_pixel_metrics_and_saved_maps(tmp_path, capsys):
    from srad_amd import evaluate as E
    size, scale = 64, 4
    root, out = tmp_path / "data", tmp_path / "out"
    names = _write_prepared_tree(root, 3, 4, size, scale)
    cfg = S.DRNConfig.for_scale(scale, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    ckpt = tmp_path / "model.pt"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ckpt)
    E.main(["--model-type", "drn-l", "--classe", "grid", "--scale", str(scale), "--resolution", str(size), "--data-root", str(root),
            "--checkpoint", str(ckpt), "--output-dir", str(out), "--dtype", "fp32", "--pixel-metrics", "--save-anomaly-maps"])
    text = capsys.readouterr().out
    assert "Test AUCs - SSIM(best ws=" in text
    line = [ln for ln in text.splitlines() if ln.startswith("Pixel AUC - SSIM map (ws=")]
    assert len(line) == 1, text
    assert 0.0 <= float(line[0].rsplit(":", 1)[1]) <= 1.0
    for split, name in names:
        f = out / "anomaly_maps" / split / f"{name}.png"
        a = np.array(Image.open(f))
        assert a.shape == (size, size) and a.dtype == np.uint8, f
    assert sorted(p.name for p in (out / "anomaly_maps").rglob("*.png")) == sorted(f"{n}.png" for _, n in names)
