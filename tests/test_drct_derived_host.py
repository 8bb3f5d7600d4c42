"""CPU: the registry of the DRCT forward's composed weights (csrc/drct_derived.h) through tests/host/drct_derived_check.cpp, a
stand-alone program that includes only that header, tail_fold.h and mlp_fold.h, built with AddressSanitizer and
UndefinedBehaviorSanitizer (linked statically, nothing is preloaded) and run once.  It holds the arena layout to the closed
formulas the engine used before the registry (F = 64, gray and RGB, x2 and x4 and no folded output end, no / 5 / 10 block folds at
E = 180, gc = 32: every region 256-aligned, in order, not overlapping, the end exact), every source name to its region and layout
offset (upsample.2 at scale 4 only, twenty other parameters to nothing), and the state machine: fresh = all stale; a refresh
builds the stale regions of the active kinds once each in arena order and leaves the others stale; one source dirties one region;
rebinding dirties all; a refresh while capturing with something to build fails and clears nothing, with nothing to build it
succeeds; a failing build leaves its region stale."""
import os
import subprocess

from tests.test_wgrad_queue_host import SANITIZE, _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "drct_derived_check.cpp")


def test_registry_layout_sources_and_states_under_sanitizers(tmp_path):
    cxx = _compiler()
    version = subprocess.run(cxx + ["--version"], capture_output=True, text=True, timeout=60).stdout
    static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]       # clang links its runtimes statically by default
    exe = str(tmp_path / "drct_derived_check")
    build = subprocess.run(cxx + ["-std=c++17", "-Wall", "-Wextra", "-Werror"] + SANITIZE + static + [SOURCE, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in run.stdout + run.stderr, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("drct_derived_check: ok"), run.stdout
