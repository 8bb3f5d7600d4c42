"""CPU: the host core of the folded DRCT output end (csrc/tail_fold.h) through tests/host/tail_fold_check.cpp, a stand-alone
program that includes only the header, built with AddressSanitizer and UndefinedBehaviorSanitizer (linked statically, nothing
is preloaded) and run once.  In double, with 4 features, for x2 and x4, gray and RGB: the fold applied by position class to maps
of 5 x 5, 7 x 9 and 8 x 12 against a literal evaluation of the chain with zero padding at every level (1e-12 absolute on values
of order 1); no response of an impulse beyond two LR pixels, exactly; the interior weights applied on the border are noticed;
taps outside the image carry zero weights.  The launch-plan override the engine tests use is declared where they look for it."""
import os
import re
import subprocess

from tests.test_wgrad_queue_host import SANITIZE, _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "tail_fold_check.cpp")


def test_fold_against_the_chain_under_sanitizers(tmp_path):
    cxx = _compiler()
    version = subprocess.run(cxx + ["--version"], capture_output=True, text=True, timeout=60).stdout
    static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]       # clang links its runtimes statically by default
    exe = str(tmp_path / "tail_fold_check")
    build = subprocess.run(cxx + ["-std=c++17", "-Wall", "-Wextra", "-Werror"] + SANITIZE + static + [SOURCE, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in run.stdout + run.stderr, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("tail_fold_check: ok"), run.stdout


def test_tail_chain_is_a_launch_plan_override():
    """SRAD_PATH_TAIL_CHAIN = 17 in the header and in ops.PLAN_PATHS, not in ops.PATHS; the ids end at 18."""
    from srad_amd import ops
    text = open(os.path.join(ROOT, "include", "srad.h")).read()
    assert re.search(r"SRAD_PATH_TAIL_CHAIN\s*=\s*17\b", text) and re.search(r"SRAD_PATH_END\s*=\s*18\b", text)
    assert ops.PLAN_PATHS["tail_chain"] == 17 and "tail_chain" not in ops.PATHS
    lib = __import__("srad_amd._lib", fromlist=["lib"]).lib()
    assert lib.srad_get_path_override(17) == 0
    assert lib.srad_set_path_override(17, 1) == 0 and lib.srad_get_path_override(17) == 1
    assert lib.srad_set_path_override(17, 0) == 0 and lib.srad_get_path_override(18) == -1
