"""The host-only unit tests of the fourth-order time integrator (csrc/tests/test_time_order.cpp: Problem::time_order, the
coefficients and the CFL guard at courant = 3/2, cpu_lap4 / cpu_leapfrog44 / cpu_first_step_t4 against a direct triple loop
on N = 6 and N = 24 grids, cube and box, with NaN in the ghost layers, the eigenmode's closed form, CpuSolver's refusals)
built as a stand-alone program with host AddressSanitizer + UBSan and run directly on the CPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ["csrc/tests/test_time_order.cpp", "csrc/src/cpu_kernels.cpp", "csrc/src/cpu_solver.cpp"]


@pytest.fixture(scope="module")
def sanitized_binary(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed for the native unit tests"
    out = tmp_path_factory.mktemp("native_time_order") / "test_time_order_asan"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fopenmp", "-ffp-contract=off", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{ROOT}/csrc/include",
           *[os.path.join(ROOT, s) for s in SOURCES], "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return out


def test_time_order_under_asan_ubsan(sanitized_binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="4")
    r = subprocess.run([str(sanitized_binary)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks, 0 failed" in r.stdout
    assert "runtime error" not in r.stderr  # UBSan report
