"""CPU: what one Swin block of the DRCT training step takes (csrc/drct_train_plan.h) through tests/host/drct_train_plan_check.cpp,
a stand-alone program that includes only that header, built with AddressSanitizer and UndefinedBehaviorSanitizer (linked
statically, nothing is preloaded) and run once.  It enumerates every BlockCaps value (fifteen yes / no answers, head dimensions
on both sides of 128) and holds plan_block to the rule the engine had before the header, restated there as implications and as
each flag's conjunction; block_saved_form to zero without the fused forward and to one named bit each for the bf16 q | k | v and
the bf16 fc1 pre-activation; and the typed view of the backward's buffers, for every plan that occurs, d in {32, 180, 276, 308},
hidden in {64, 360, 512}, KA in {32, 180} and 64 and 8192 tokens: every member inside its raw buffer as the planner sizes it,
dx1 * rs1 behind the bf16 dx2 and adjust5's dA copy behind the bf16 dh, bf16 members 16-byte aligned, and the capacity rule
(true there, false for a model whose hidden layers are too narrow for the copy)."""
import os
import subprocess

from tests.test_wgrad_queue_host import SANITIZE, _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "drct_train_plan_check.cpp")


def test_block_plan_saved_form_and_buffer_view_under_sanitizers(tmp_path):
    cxx = _compiler()
    version = subprocess.run(cxx + ["--version"], capture_output=True, text=True, timeout=60).stdout
    static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]       # clang links its runtimes statically by default
    exe = str(tmp_path / "drct_train_plan_check")
    build = subprocess.run(cxx + ["-std=c++17", "-Wall", "-Wextra", "-Werror"] + SANITIZE + static + [SOURCE, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in run.stdout + run.stderr, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("drct_train_plan_check: ok"), run.stdout
