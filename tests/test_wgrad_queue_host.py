"""CPU: the split-K gradient queue's bookkeeping (csrc/wgrad_queue.h) under AddressSanitizer and UndefinedBehaviorSanitizer.
tests/host/wgrad_queue_check.cpp is a stand-alone program that includes only that header (no HIP): it drives the queue with a
recorder in place of the reduce launch through the scripted cases of tests/test_gpu_wgrad_queue.py and a few thousand seeded
random sequences, and checks regions, pending marks, batches, tile numbering and the peak after every step.  Here it is built
into a temporary directory and run once.  The sanitizer runtimes are linked statically, so nothing is preloaded; nothing that
is loaded into Python is sanitised, and nothing of this runs on a GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "wgrad_queue_check.cpp")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _compiler():
    """$CXX if set, else the clang++ beside hipcc in ROCm's LLVM.  None found is a failure: the library needs one too."""
    cxx = os.environ.get("CXX")
    if cxx:
        found = shutil.which(cxx.split()[0])
        assert found, f"CXX={cxx} is not an executable"
        return cxx.split()
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++")):
        if os.path.exists(cand):
            return [cand]
    raise AssertionError(f"no C++ compiler: CXX is not set and there is no clang++ in ROCm's LLVM under {rocm}")


def test_queue_bookkeeping_under_sanitizers(tmp_path):
    cxx = _compiler()
    version = subprocess.run(cxx + ["--version"], capture_output=True, text=True, timeout=60).stdout
    static = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]       # clang links its runtimes statically by default
    exe = str(tmp_path / "wgrad_queue_check")
    build = subprocess.run(cxx + ["-std=c++17", "-Wall", "-Wextra", "-Werror"] + SANITIZE + static + [SOURCE, "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in run.stdout + run.stderr, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("wgrad_queue_check: ok"), run.stdout
