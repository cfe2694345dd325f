"""The host-only unit tests of the point sources (csrc/tests/test_sources.cpp: plan_sources over one rank, slab and block
decompositions at N = 77; cpu_source_response against a CpuSolver run from a zero field; the split identity forced solve
= unforced passes + responses, whose rounding d_split it prints) built as a stand-alone program with host
AddressSanitizer + UBSan and run directly on the CPU. The d_split / umax it prints for the N = 40 configurations are the
constants the fused GPU tests derive their tolerance from (tests/sources_common.py); those of the K = 203 shot
(tests/long_reference.py) belong to tests/test_gpu_long_solves.py, and the program built that shot's time step and
wavelets itself: they are compared with the Python side's."""
import os
import re
import shutil
import subprocess

import pytest

import numpy as np

from long_reference import D_SPLIT_LONG, UMAX_LONG, long_shot, long_spec
from sources_common import D_SPLIT, UMAX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ["csrc/tests/test_sources.cpp", "csrc/src/cpu_kernels.cpp", "csrc/src/cpu_solver.cpp", "csrc/src/schedule.cpp"]


@pytest.fixture(scope="module")
def sanitized_binary(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx is not None, "g++ is needed for the native unit tests"
    out = tmp_path_factory.mktemp("native_sources") / "test_sources_asan"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fopenmp", "-ffp-contract=off", "-fno-omit-frame-pointer",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{ROOT}/csrc/include",
           *[os.path.join(ROOT, s) for s in SOURCES], "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return out


def test_sources_under_asan_ubsan(sanitized_binary):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="4")
    r = subprocess.run([str(sanitized_binary)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checks, 0 failed" in r.stdout
    assert "runtime error" not in r.stderr  # UBSan report
    # the figures behind the fused GPU tolerance are the ones this program prints for the same solves
    got = {m[0]: (float(m[1]), float(m[2]))
           for m in re.findall(r"split (\S+) N=\d+ K=\d+: d_split = (\S+) umax = (\S+)", r.stdout)}
    assert set(got) == {"one-source", "cube", "box", "long-cube", "long-box"}, r.stdout
    assert got["cube"] == (D_SPLIT[False], UMAX[False]) and got["box"] == (D_SPLIT[True], UMAX[True]), got
    assert got["long-cube"] == (D_SPLIT_LONG[False], UMAX_LONG[False]), got
    assert got["long-box"] == (D_SPLIT_LONG[True], UMAX_LONG[True]), got
    # ... and the long shot it solved is the Python side's: the same time step and the same wavelet samples
    shot = {m[0]: (float(m[1]), float(m[2]))
            for m in re.findall(r"long-shot (\S+): tau = (\S+) sum \|w\| = (\S+)", r.stdout)}
    for box, name in ((False, "long-cube"), (True, "long-box")):
        assert shot[name] == (long_spec(40, box).tau, float(np.abs(long_shot(40, box).w).sum())), (name, shot)
