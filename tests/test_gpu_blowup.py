"""Blow-up detection of whole GPU solves against CpuSolver, the definition (tests/test_blowup_cpu.py has the CPU side).

a. A start with one NaN or +Inf node (N = 24, tau = 0.9 tau_max, K = 11, every step checked): every one-rank schedule
   on the first run, the graph replay and run_batch(2), cube and box, groups over loopback and rccl-self with the node
   deep inside one rank, and sponge layers. The log is CpuSolver's — steps, maxima bit for bit (never NaN), the rms
   column of the same class at every step — `finite` is False and both stored levels equal CpuSolver's under
   same_class_bits.
b. A genuine overflow (tau = 10 tau_max forced, K = 160; 3 tau_max, K = 260): the maximum bit-equal at every step
   through the Inf phase and the final zeros, the rms column of the same class and within 1e-12 where finite.
c. Both CLIs exit with 3."""
import dataclasses
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from long_reference import long_spec
from nonfinite_common import (N_BLOW, assert_log_same_class, assert_overflow_phases, blowup_spec, first_nonfinite_step,
                              klass, same_class_bits, save_initial)
from sources_common import lcg_fields
from test_gpu_sponge import SCHEDULES, SPONGES

from mpi_cuda_amd.solver import Solver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "wave3d")

N, K = N_BLOW, 11
NODE = (12, 11, 13)
VALUES = {"nan": float("nan"), "+inf": float("inf")}


def _planted(value, node=NODE):
    phi, psi = (f.copy() for f in lcg_fields(N))
    phi[node] = VALUES[value]
    return phi, psi


@functools.lru_cache(maxsize=None)
def _cpu_planted(value, box, sponge=None, node=NODE):
    spec = long_spec(N, box, K=K, check_every=1)
    if sponge:
        spec = dataclasses.replace(spec, sponge=SPONGES[sponge])
    c = Solver(spec, backend="cpu")
    c.set_initial(*_planted(value, node))
    r = c.run()
    assert r.finite is False and first_nonfinite_step(r) == 1
    return spec, r, c.global_field(0).numpy().copy(), c.global_field(1).numpy().copy()


def _check(s, r, want, what, pinned_face=False):
    """pinned_face: schedules that run k_leapfrog_p2 on rows with an odd number of interior nodes (N = 24: 23). The pass
    enforces the Dirichlet value through tau^2 = 0, fma(0, Lap, +0), which is NaN for a non-finite Laplacian where the CPU
    never computes, and the boundary node z = N is the second half of the last stored pair: there the stored value is +0
    or NaN, NaN only where the CPU's field is NaN at (x, y, N - 1) (tests/test_gpu_nonfinite_kernels.py pins the exact
    rule per pass). Every other node equals CpuSolver's."""
    assert_log_same_class(r, want[1], what)
    _check_fields(s, want, what, pinned_face)


def _check_fields(s, want, what, pinned_face):
    _, _, uK, uK1 = want
    for which, ref in ((0, uK), (1, uK1)):
        got = s.global_field(which).numpy().copy()
        if pinned_face:
            face = got[:, :, N]
            assert ((face.view(np.int64) == 0) | np.isnan(face)).all(), (what, which)
            assert not (np.isnan(face) & ~np.isnan(ref[:, :, N - 1])).any(), (what, which)
            assert not np.isnan(face[0]).any() and not np.isnan(face[:, 0]).any(), (what, which)
            assert not np.isnan(face[N]).any() and not np.isnan(face[:, N]).any(), (what, which)
            got[:, :, N] = ref[:, :, N]
        assert same_class_bits(got, ref), (what, "u^K" if which == 0 else "u^K-1")


def _fused(sched):
    return SCHEDULES[sched]["temporal"] >= 2


@functools.lru_cache(maxsize=None)
def _fused_sponge_log(value, S):
    """What the error log of a fused solve under sponge layers holds, from the native CPU kernels: step 1 is the check of
    the stored u^1; then each unit of min(S, K - n) steps checks the UNDAMPED steps from its inputs u^{n-1}, u^n, and the
    next unit starts from the damped levels. Returns (maxima, sums) for steps 1..K; the damped levels it ends with are
    asserted to be CpuSolver's."""
    from mpi_cuda_amd._native import load

    C = load()
    spec, _, uK, uK1 = _cpu_planted(value, False, sponge="all6")
    prob = spec.native()
    lay = C.make_layout(prob, C.rank_box(prob, C.Dims(1, 1, 1), 0))
    co, box, s_ext = C.Coeffs.from_problem(prob), C.compute_box(lay), C.sin_table_ext(prob)
    src = C.initial_layout(prob, lay)
    phi, psi = _planted(value)
    a, b = np.zeros(int(lay.total)), np.zeros(int(lay.total))
    C.cpu_first_step_field(lay, src, co, spec.tau, C.initial_to_local(src, phi.reshape(-1)),
                           C.initial_to_local(src, psi.reshape(-1)), a, b)
    ct = lambda n: math.cos(prob.a_t * (n * spec.tau))  # noqa: E731  (problem.hpp time_factor's order)
    log = {1: C.cpu_error(lay, b, box, s_ext, ct(1))}
    n = 1
    while n < K:
        steps = min(S, K - n)
        pa, pb = a.copy(), b.copy()
        for k in range(1, steps + 1):
            log[n + k] = C.cpu_leapfrog(lay, co, pb, pa, box, s_ext, ct(n + k), True)
            pa, pb = pb, pa
            C.cpu_leapfrog(lay, co, b, a, box, s_ext, sponge=prob)
            a, b = b, a
        n += steps
    from mpi_cuda_amd.ops.stencil import grid_view
    import torch

    for f, ref in ((b, uK), (a, uK1)):
        assert same_class_bits(grid_view(lay, torch.from_numpy(f))[1:-1, 1:-1, 1:-1].numpy(), ref)
    return [float(log[k][0]) for k in range(1, K + 1)], [float(log[k][1]) for k in range(1, K + 1)]


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("box", [False, True], ids=["cube", "box"])
@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_planted_start_one_rank(gpu, sched, box, value):
    want = _cpu_planted(value, box)
    s = Solver(want[0], backend="hip", device=0, **SCHEDULES[sched])
    s.set_initial(*_planted(value))
    for run in ("first run", "second run"):
        _check(s, s.run(), want, (sched, box, value, run), _fused(sched))
    for r in s.run_batch(2):
        _check(s, r, want, (sched, box, value, "run_batch"), _fused(sched))


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("transport,decomp,world,node", [("loopback", "slab", 2, (6, 11, 13)),
                                                         ("rccl-self", "2x2x2", 8, (18, 17, 6))])
def test_planted_start_groups(gpu, transport, decomp, world, node, value):
    """The planted node lies six nodes from every face of one rank: for the first steps only that rank's partials are
    non-finite, and the combined log is CpuSolver's at every step."""
    want = _cpu_planted(value, False, node=node)
    g = Solver(want[0], backend="hip", transport=transport, world=world, rank=0, decomp=decomp, device=0)
    g.set_initial(*_planted(value, node))
    for run in range(2):
        _check(g, g.run(), want, (transport, decomp, value, run))


@pytest.mark.parametrize("value", list(VALUES))
@pytest.mark.parametrize("temporal", [1, 5])
def test_planted_start_with_sponge_layers(gpu, temporal, value):
    """all6: k_sponge_box and the DAMP single steps see non-finite inputs. temporal = 1 is CpuSolver's log and fields.
    temporal = 5: both stored levels are CpuSolver's (apart from the pinned face of _check) — the check of k_sponge_box on
    non-finite data. The log of that mode is not CpuSolver's, for any data: a fused unit's error partials come from the
    undamped pass, before k_sponge_box rewrites the slabs (solver.hpp: "The error log then has no meaning"). It is pinned
    to what it is, the check of the undamped continuation of each unit's damped inputs (_fused_sponge_log): maxima bit for
    bit, the sum's class at every step, `finite` False from step 1."""
    want = _cpu_planted(value, False, sponge="all6")
    s = Solver(want[0], backend="hip", device=0, temporal=temporal)
    assert s.native.sponge
    s.set_initial(*_planted(value))
    for run in ("first run", "second run"):
        if temporal == 1:
            _check(s, s.run(), want, ("sponge", temporal, value, run))
            continue
        r = s.run()
        mx, sm = _fused_sponge_log(value, temporal)
        assert r.steps == want[1].steps == list(range(1, K + 1)) and r.finite is False, run
        assert first_nonfinite_step(r) == 1 and not np.isnan(np.array(r.max_err)).any(), run
        assert same_class_bits(r.max_err, mx), (run, r.max_err, mx)
        assert [klass(v) for v in r.rms_err] == [klass(v) for v in sm], (run, r.rms_err, sm)
        _check_fields(s, want, ("sponge", temporal, value, run), True)


# ---- b. genuine overflow -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_overflow(key):
    spec = blowup_spec(key)
    c = Solver(spec, backend="cpu", force=True)
    c.set_initial(*lcg_fields(N))
    r = c.run()
    assert_overflow_phases(r)
    return spec, r, c.global_field(0).numpy().copy(), c.global_field(1).numpy().copy()


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_overflow_one_rank(gpu, sched):
    want = _cpu_overflow("10x")
    s = Solver(want[0], backend="hip", device=0, force=True, **SCHEDULES[sched])
    s.set_initial(*lcg_fields(N))
    for run in ("first run", "second run"):
        _check(s, s.run(), want, (sched, run), _fused(sched))
    for r in s.run_batch(2):
        _check(s, r, want, (sched, "run_batch"), _fused(sched))


def test_overflow_loopback_group(gpu):
    want = _cpu_overflow("10x")
    g = Solver(want[0], backend="hip", transport="loopback", world=2, rank=0, decomp="slab", device=0, force=True)
    g.set_initial(*lcg_fields(N))
    _check(g, g.run(), want, "loopback 2")


def test_slower_overflow_on_the_default_schedule(gpu):
    want = _cpu_overflow("3x")
    s = Solver(want[0], backend="hip", device=0, force=True)
    s.set_initial(*lcg_fields(N))
    _check(s, s.run(), want, "3x", True)


# ---- c. exit codes -------------------------------------------------------------------------------------------------------
def _args(spec):
    return [str(spec.N), repr(spec.tau), str(spec.K), "--force", "--check-every", "1"]


def test_both_clis_exit_with_3_on_the_gpu(gpu, tmp_path):
    spec = blowup_spec("10x")
    pre = str(tmp_path / "ini")
    save_initial(pre, spec, *lcg_fields(N))
    js = tmp_path / "n.json"
    rn = subprocess.run([CLI, *_args(spec), "--initial", pre, "--json", str(js)], capture_output=True, text=True,
                        timeout=120)
    assert rn.returncode == 3, (rn.returncode, rn.stderr[-2000:])
    assert "solution blew up (non-finite error)" in rn.stderr and '"finite": false' in js.read_text()
    jp = tmp_path / "p.json"
    rp = subprocess.run([sys.executable, "-m", "mpi_cuda_amd", *_args(spec), "--backend", "hip", "--initial", pre,
                         "--json", str(jp)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert rp.returncode == 3, (rp.returncode, rp.stderr[-2000:])
    assert json.loads(jp.read_text())["finite"] is False


def test_native_binary_on_two_ranks_exits_with_3(gpu, tmp_path):
    """Two rank processes on one GPU under the launcher tests/test_gpu_native_proc.py uses (copy engines over IPC, no
    RCCL): both exit with 3."""
    spec = blowup_spec("10x")
    pre = str(tmp_path / "ini")
    save_initial(pre, spec, *lcg_fields(N))
    script = tmp_path / "w.py"
    script.write_text(
        "import os, subprocess, sys\n"
        "r = subprocess.run([os.environ['CLI'], *os.environ['ARGS'].split('\\x1f'), '--transport', 'sdma', '--no-rccl', '--tb-min-planes', '8'],"
        " capture_output=True, text=True, timeout=90)\n"
        "open(os.environ['OUT'] + '.' + os.environ['RANK'], 'w').write(str(r.returncode) + '\\n' + r.stderr)\n")
    # (the ranks are children of the worker processes, not of the launcher, so they cannot derive a common rendezvous
    # path from their parent's pid: it is given, as parallel/native_proc.py gives it; a rank that misses its peer gives
    # up after 20 s)
    env = dict(os.environ, CLI=CLI, OUT=str(tmp_path / "rc"), ARGS="\x1f".join(_args(spec) + ["--initial", pre]),
               W3D_TIMEOUT_S="30", W3D_FILE_TIMEOUT_S="20", W3D_RDZV_FILE=str(tmp_path / "rdzv.uid"),
               W3D_JOB_ID=f"blowup{os.getpid()}", W3D_SHARE_GPUS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(29850 + os.getpid() % 100), str(script)]
    p = subprocess.run(cmd, env=env, timeout=240, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    for rank in range(2):
        out = (tmp_path / f"rc.{rank}").read_text()
        assert out.splitlines()[0] == "3", out[-2000:]
        assert "solution blew up (non-finite error)" in out
