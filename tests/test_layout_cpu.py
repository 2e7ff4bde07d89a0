"""The block layout helper (svo_amd/csrc/layout.hpp) under ASan + UBSan:
tools/layout_check.cpp built with the line at its top and run. No GPU, and no
part of the library: the header includes nothing of HIP."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_check_runs_clean_under_asan_and_ubsan():
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"  # (the library's host compiler)
    os.makedirs(os.path.join(ROOT, "tools", "bin"), exist_ok=True)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-Isvo_amd/csrc",
                           "tools/layout_check.cpp", "-o", "tools/bin/layout_check"], cwd=ROOT)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([os.path.join(ROOT, "tools", "bin", "layout_check")], cwd=ROOT, env=env,
                         capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert "layout_check: ok" in out.stdout
