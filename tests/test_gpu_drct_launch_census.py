"""GPU: which launches the DRCT inference forward runs, held to tests/golden/drct_launch_census.json - per profiler class the
launch count and the flops and bytes summed over the launch parameters, of three eager forwards (the first under an override
set, the next, the one after a folded parameter changed) for fp32 / bf16 / split-bf16 at the smallest inputs where the paths
differ, under each launch-plan override, all four together and unfused_blocks, plus a bf16 handle bound for training.  The
fixture was recorded by tests/golden/make_drct_launch_census.py at the commit it names, not on the code under test; this test
runs the same cases through the same functions and asserts equality.  Classes, not kernels, are what the library's profiler
counts (several kernels share one: the fold builds count as pack_weight); the flops and bytes sums are what tells the folded
form of a launch from the plain one inside a class.  No source of the folded output end changes in these cases: that a stale
output end stays stale under tail_chain is held by tests/host/drct_derived_check.cpp alone.  The chip-filling rules depend on the CU count, so a device
with another count than the recorded one is the one reason to skip."""
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
    spec = importlib.util.spec_from_file_location("make_drct_launch_census", os.path.join(HERE, "golden", "make_drct_launch_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(os.path.join(HERE, "golden", "drct_launch_census.json")) as f:
        return json.load(f)


def _case_ids():
    return list(_fixture()["cases"])


def test_fixture_covers_the_generator_cases():
    assert _case_ids() == _maker().case_ids()
    assert _fixture()["commit"] and _fixture()["device"] and _fixture()["cus"] > 0


@pytest.mark.parametrize("case", _case_ids())
def test_launches_match_the_recorded_census(case):
    want = _fixture()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != want["cus"]:
        pytest.skip(f"the census was recorded on {want['cus']} CUs, this device has {cus}")
    got = json.loads(json.dumps(_maker().run_case(case)))            # through JSON, as the fixture went
    for label, forwards in want["cases"][case].items():
        for which, classes in forwards.items():
            assert got[label][which] == classes, (case, label, which)
    assert got == want["cases"][case]
