"""Blow-up detection on the CPU path, the definition every GPU check is compared with (tests/test_gpu_blowup.py).

`finite` in the error log is the only blow-up detector: bench.py rejects a run on it and both CLIs turn it into exit
code 3. Every maximum in the code drops NaN, so a field that is NaN everywhere has maximum error 0 and is reported only
through the sum of squares. Here: a genuine overflow (tau = 10 and 3 times tau_max, forced) passes through its four
phases — sum Inf, maximum Inf, sum NaN, maximum back at 0.0 — and stays non-finite from the first bad step on; a start
with one NaN or +Inf node is non-finite from the first checked step; both CLIs exit with 3."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nonfinite_common import (N_BLOW, OVERFLOW, assert_overflow_phases, blowup_spec, first_nonfinite_step, klass,
                              save_initial)
from sources_common import lcg_fields

from mpi_cuda_amd._native import load
from mpi_cuda_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "wave3d")


def _overflow(key):
    s = Solver(blowup_spec(key), backend="cpu", force=True)
    s.set_initial(*lcg_fields(N_BLOW))
    return s, s.run()


@pytest.mark.parametrize("key", list(OVERFLOW))
def test_overflow_passes_through_all_four_phases(key):
    s, r = _overflow(key)
    first = assert_overflow_phases(r)
    print(f"BLOWUP cpu {key}: sum Inf at {first[0]}, max Inf at {first[1]}, sum NaN at {first[2]}")
    assert r.steps == list(range(1, OVERFLOW[key][1] + 1))
    u = s.global_field(0).numpy()
    assert np.isnan(u[1:-1, 1:-1, 1:-1]).all() and not u[0].any() and not u[:, :, -1].any()


def test_thread_count_does_not_move_the_overflow():
    logs = []
    for t in (1, 3):
        s = Solver(blowup_spec("10x"), backend="cpu", force=True, threads=t)
        s.set_initial(*lcg_fields(N_BLOW))
        r = s.run()
        logs.append((np.array(r.max_err).view(np.int64).tolist(), [klass(v) for v in r.rms_err]))
    assert logs[0] == logs[1]


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "+inf"])
def test_planted_start_is_reported_from_the_first_step(value):
    from long_reference import long_spec

    spec = long_spec(N_BLOW, False, K=11, check_every=1)
    phi, psi = (f.copy() for f in lcg_fields(N_BLOW))
    phi[12, 11, 13] = value
    s = Solver(spec, backend="cpu")
    s.set_initial(phi, psi)
    r = s.run()
    assert r.finite is False and first_nonfinite_step(r) == 1
    assert not np.isnan(np.array(r.max_err)).any()
    assert all(not np.isfinite(e) for e in r.rms_err)
    if np.isnan(value):
        assert np.isnan(np.array(r.rms_err)).all() and np.isfinite(np.array(r.max_err)).all()


@pytest.fixture(scope="module")
def cli_built():
    if not os.path.exists(CLI):
        load()
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build.py")], check=True)
    assert os.path.exists(CLI)


def test_both_clis_exit_with_3(tmp_path, cli_built):
    spec = blowup_spec("10x")
    pre = str(tmp_path / "ini")
    save_initial(pre, spec, *lcg_fields(N_BLOW))
    js = tmp_path / "n.json"
    args = [str(spec.N), repr(spec.tau), str(spec.K)]
    rn = subprocess.run([CLI, *args, "--cpu", "--force", "--check-every", "1", "--initial", pre, "--json", str(js)],
                        capture_output=True, text=True, timeout=120)
    assert rn.returncode == 3, (rn.returncode, rn.stderr[-2000:])
    assert "solution blew up (non-finite error)" in rn.stderr
    assert '"finite": false' in js.read_text()
    jp = tmp_path / "p.json"
    rp = subprocess.run([sys.executable, "-m", "mpi_cuda_amd", *args, "--backend", "cpu", "--force", "--check-every", "1",
                         "--initial", pre, "--json", str(jp)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert rp.returncode == 3, (rp.returncode, rp.stderr[-2000:])
    rec = json.loads(jp.read_text())
    assert rec["finite"] is False and '"finite": false' in jp.read_text()
    # without --force the CFL guard refuses before anything runs
    assert subprocess.run([CLI, *args, "--cpu"], capture_output=True, text=True, timeout=120).returncode == 2
