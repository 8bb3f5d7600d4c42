"""CPU: ``evaluate_on_test`` at world 1 against a recording of what the evaluator gave before it was last restructured
(tests/golden/eval_stage.json, written by tests/golden/make_eval_stage_golden.py on the commit before that change): for every
case the returned dictionary with its key order, every printed line character for character, and what was asked to be saved.
The kernels are CPU stand-ins, the same for the recording and here, so this pins the host side only: which maps are made, which
metrics run, which keys and lines come out.  A case that differs means the evaluator changed; the recording is not remade from
the code under test."""
import importlib.util
import json
import os

import numpy as np
import pytest

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def generator():
    spec = importlib.util.spec_from_file_location("make_eval_stage_golden", os.path.join(GOLDEN_DIR, "make_eval_stage_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recomputed(generator):
    return generator.run_cases()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN_DIR, "eval_stage.json")) as f:
        return json.load(f)


def test_the_recording_holds_the_cases(generator, recorded):
    cases = generator.cases()
    assert list(recorded) == list(cases) and len(cases) == 46
    assert sum(n.startswith("flags_") for n in cases) == 16 and sum(n.startswith("op_") for n in cases) == 9
    assert sum(n.startswith(("ssim_", "mse_")) for n in cases) == 20 and sum(n.endswith("_sigma_fpr") for n in cases) == 10
    # the recording reaches what the world-2 tests do not: the single-rank half, with and without masks, and every line
    lines = [ln for c in recorded.values() for ln in c["lines"]]
    for head in ("Test AUCs - ", "Image AUC - max of the SSIM map", "Image AUC - max of the MSE map", "Pixel AUC - ", "AU-PRO - ",
                 "Operating point - ", "Pixel metrics skipped: 1 test", "Pixel metrics skipped: 7 test"):
        assert any(ln.startswith(head) for ln in lines), head
    assert recorded["flags_0000"]["result"][0] == ["best_ws", 13]          # not the first size: map_ws 0 and 3 are two cases
    assert any(e[0] == "masks" for e in recorded["save_masks"]["saved"]) and any(e[0] == "sr" for e in recorded["save_masks"]["saved"])
    assert recorded["flags_1000"]["saved"][0][1][-2:] == ["00005", "00006"]                # images beyond the list of names


def test_every_case_equals_the_recording(recomputed, recorded):
    assert list(recomputed) == list(recorded)
    for name, want in recorded.items():
        got = recomputed[name]
        assert [k for k, _ in got["result"]] == [k for k, _ in want["result"]], name      # the keys, in order
        for (k, a), (_, b) in zip(got["result"], want["result"]):
            assert type(a) is type(b) and a == b, (name, k, a, b)                          # floats exactly
        assert got["lines"] == want["lines"], name
        assert got["saved"] == want["saved"], name


def test_best_window_first_maximum_wins():
    from srad_amd import metrics as M
    y = [0, 0, 1, 1]
    good, poor = [0.9, 0.8, 0.2, 0.1], [0.9, 0.1, 0.8, 0.2]               # as SSIM: the score is 1 - it
    cols = np.array([poor, good, good, poor]).T
    assert M.best_window(y, cols, [3, 13, 23, 33]) == (1, [0.5, 1.0, 1.0, 0.5])
    assert M.best_window(y, np.array([good, good]).T, [3, 13]) == (0, [1.0, 1.0])
    wide = np.concatenate([cols, np.zeros((4, 2))], axis=1)               # the evaluator's table: MSE and PSNR columns follow
    assert M.best_window(y, wide, [3, 13, 23, 33]) == (1, [0.5, 1.0, 1.0, 0.5])
