"""GPU: AU-PRO in the evaluator (evaluate_on_test(aupro=True) and the CLI's --aupro) end to end, against the same pipeline run
through the CPU oracle and the numpy restatement of the metric (tests/golden/make_pro_golden.py)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import scorer_ref as O
from oracle import sr_ref as R
from srad_amd import spec as S
from tests.test_gpu_anomaly_maps import map_oracle
from tests.test_gpu_pixel_eval import _model, _pairs_and_masks, _write_prepared_tree

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_pro_golden", os.path.join(GOLDEN_DIR, "make_pro_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _aupro_ref(maps, masks, limit):
    G = _generator()
    z, n_reg = G.uf_sizes(np.stack(masks))
    fpr, pro = G.pro_curve_ref(maps, z, n_reg)
    return G.aupro_ref(fpr, pro, limit)


@pytest.mark.parametrize("model_type", ["drct", "drn-l"])
def test_aupro_matches_oracle_pipeline(model_type):
    from srad_amd import evaluate as E
    from srad_amd import metrics as M
    scale, hr_size = 4, 64
    opt, model, cfg, sd = _model(model_type, hr_size, scale)
    y, good, bad, masks = _pairs_and_masks(6, 8, hr_size, scale, 1)
    plain = E.evaluate_on_test(opt, model, good, bad)
    got = E.evaluate_on_test(opt, model, good, bad, masks=masks, aupro=True)
    for k in plain:
        assert got[k] == plain[k], k
    assert set(got) - set(plain) == {"aupro", "pro_fpr_limit", "map_ws"}
    assert got["pro_fpr_limit"] == 0.3 and 0.0 <= got["aupro"] <= 1.0
    # both pixel metrics: one set of maps, each number as when asked alone
    pix = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True)
    both = E.evaluate_on_test(opt, model, good, bad, masks=masks, pixel_metrics=True, aupro=True, pro_fpr_limit=0.05)
    assert set(both) - set(plain) == {"auc_pixel", "aupro", "pro_fpr_limit", "map_ws"}
    assert both["auc_pixel"] == pix["auc_pixel"] and both["pro_fpr_limit"] == 0.05
    sr_u8, hr_u8 = [], []
    with torch.no_grad():
        for lr, hr in good + bad:
            x = torch.from_numpy(lr).permute(2, 0, 1)[None].float()
            out = R.drct_forward(sd, x, cfg) if model_type == 'drct' else R.drn_forward(sd, x, cfg)[-1]
            sr_u8.append(np.transpose(O.to_u8_trunc(out.numpy()[0]), (1, 2, 0)))
            hr_u8.append(hr)
    ref = O.evaluate_pairs(y, sr_u8, hr_u8)
    assert got["map_ws"] == ref["best_ws"] == got["best_ws"]
    ws = ref["best_ws"]
    ref_maps = np.stack([map_oracle(s, h, ws) for s, h in zip(sr_u8, hr_u8)])
    ref_aupro = _aupro_ref(ref_maps, masks, 0.3)
    print(f"{model_type}: pipeline AU-PRO {got['aupro']:.9f}, oracle pipeline {ref_aupro:.9f}, "
          f"|d| = {abs(got['aupro'] - ref_aupro):.2e}")
    assert abs(got["aupro"] - ref_aupro) <= 0.002, (got["aupro"], ref_aupro)          # north_star: as the AUCs, within +-0.002
    # the same SR images on both sides: only the maps' own parity (~1e-6) separates the two
    maps = M.anomaly_maps(torch.from_numpy(np.stack(sr_u8)).cuda(), torch.from_numpy(np.stack(hr_u8)).cuda(), ws)
    dev = M.aupro(maps, torch.from_numpy(np.stack(masks)).cuda())
    assert abs(dev - ref_aupro) <= 1e-6, (dev, ref_aupro)
    # a missing mask skips AU-PRO without failing the run
    holey = list(masks)
    holey[-1] = None
    skipped = E.evaluate_on_test(opt, model, good, bad, masks=holey, aupro=True)
    assert "aupro" not in skipped and skipped["auc_ssim"] == plain["auc_ssim"]


def test_cli_aupro(tmp_path, capsys):
    from srad_amd import evaluate as E
    size, scale = 64, 4
    root = tmp_path / "data"
    _write_prepared_tree(root, 3, 4, size, scale)
    cfg = S.DRNConfig.for_scale(scale, 1)
    sd = S.synth_state(S.drn_spec(cfg), seed=9, gain=0.4, cfg=cfg)
    ckpt = tmp_path / "model.pt"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, ckpt)
    out = E.main(["--model-type", "drn-l", "--classe", "grid", "--scale", str(scale), "--resolution", str(size), "--data-root",
                  str(root), "--checkpoint", str(ckpt), "--output-dir", str(tmp_path / "out"), "--dtype", "fp32", "--aupro",
                  "--pro-fpr-limit", "0.2"])
    text = capsys.readouterr().out
    line = [ln for ln in text.splitlines() if ln.startswith("AU-PRO - SSIM map (ws=")]
    assert len(line) == 1, text
    assert "fpr <= 0.2)" in line[0]
    assert out["pro_fpr_limit"] == 0.2 and 0.0 <= out["aupro"] <= 1.0
    assert abs(float(line[0].rsplit(":", 1)[1]) - out["aupro"]) <= 5e-5
    assert "auc_pixel" not in out and not [ln for ln in text.splitlines() if ln.startswith("Pixel AUC")]
