"""GPU: which launches one DRCT training step runs, held to tests/golden/drct_train_census.json - per profiler class the launch
count and the flops and bytes summed over the launch parameters, separately for the training forward and for the backward, the
workspace size the engine asks for, and the split-K queue's reduce launches by reason with the block peak.  One RDG per case,
the smallest shape that reaches each Swin-block plan of csrc/drct_train_plan.h: fp32; bf16 with the fused forward and the
16-row fused backward, without and with DropPath factors; the unfused_blocks override over build and step, and over the step
only; 8192 tokens (every gradient and save as bf16); window 16; RGB x4 without an input gradient; a cut split-K budget.  The
fixture was recorded by tests/golden/make_drct_train_census.py at the commit it names, not on the code under test; this test
runs the same cases through the same function and asserts equality, entry for entry.  The chip-filling rules depend on the CU
count, so a device with another count than the recorded one is the one reason to skip."""
import functools
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def _maker():
    spec = importlib.util.spec_from_file_location("make_drct_train_census", os.path.join(HERE, "golden", "make_drct_train_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(os.path.join(HERE, "golden", "drct_train_census.json")) as f:
        return json.load(f)


def _case_ids():
    return list(_fixture()["cases"])


def test_fixture_covers_the_generator_cases():
    assert _case_ids() == _maker().case_ids()
    assert _fixture()["commit"] and _fixture()["device"] and _fixture()["cus"] > 0


@pytest.mark.parametrize("case", _case_ids())
def test_training_step_matches_the_recorded_census(case):
    want = _fixture()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != want["cus"]:
        pytest.skip(f"the census was recorded on {want['cus']} CUs, this device has {cus}")
    got = json.loads(json.dumps(_maker().run_case(case)))            # through JSON, as the fixture went
    for entry, value in want["cases"][case].items():
        assert got[entry] == value, (case, entry)
    assert got == want["cases"][case]
