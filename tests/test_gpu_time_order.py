"""time_order = 4 solves on one GPU rank against CpuSolver, the definition: u^K, u^{K-1}, the error log's steps and Max Error
column and the traces bit for bit (the L2 column to summation order).

N = 24 (cube) and N = 40 (box 1 x 1.3 x 0.7) at tau = 0.9 of the limit (courant 1.35), K = 23, check cadence 1 and 4; the
default options (temporal = 5, which such a solve turns into single steps of two launches), temporal = 1 (a schedule with
two field buffers: the solver allocates v itself), graph = False and 16-row tiles; first run and graph replay; the eigenmode
start, set_initial(phi, psi) and receivers; one K = 203 solve at N = 40. Every unit is a single step and no start is
analytic. The refusals that need no second process, and both CLIs against the API."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from long_reference import long_shot
from sources_common import lcg_fields, same_bits
from time_order_reference import time_order_spec

from mpi_cuda_amd.models.wave3d import ProblemSpec
from mpi_cuda_amd.solver import Solver
from mpi_cuda_amd.utils import dump as dumpio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {"N24-cube": (24, False), "N40-box": (40, True)}
OPTIONS = {"default": dict(), "temporal1": dict(temporal=1), "nograph": dict(graph=False), "ty16": dict(tiling={"ty": 16})}


def _spec(grid, K, check_every):
    N, box = GRIDS[grid]
    s = time_order_spec(N, box, K, check_every)
    assert s.cfl_ok and s.courant > 1.3
    return s


def _arm(s, grid, mode):
    N, box = GRIDS[grid]
    if mode in ("initial", "receivers"):
        s.set_initial(*lcg_fields(N))
    if mode == "receivers":
        s.set_receivers(long_shot(N, box).receivers)
    return s


@functools.lru_cache(maxsize=None)
def _cpu(grid, K, mode, check_every):
    s = _arm(Solver(_spec(grid, K, check_every), backend="cpu"), grid, mode)
    r = s.run()
    return (s.global_field(0).numpy().copy(), s.global_field(1).numpy().copy(), r,
            s.traces().numpy().copy() if mode == "receivers" else None)


def _check(s, r, ref, what, traces):
    uK, uK1, rc, tr = ref
    assert s.native.unit_steps and set(s.native.unit_steps) == {1} and not s.native.analytic_start, what
    assert same_bits(s.global_field(0).numpy(), uK), f"{what}: u^K differs from CpuSolver"
    assert same_bits(s.global_field(1).numpy(), uK1), f"{what}: u^K-1 differs from CpuSolver"
    assert r.steps == rc.steps and r.max_err == rc.max_err and r.finite == rc.finite, what
    # (the log's L2 column is sqrt of a sum of (N - 1)^3 non-negative squares that the workgroups and the CPU's planes add
    # in different orders: equal within (N - 1)^3 eps / 2, the worst case of reordering such a sum, as in every GPU test here)
    tol = (s.spec.N - 1) ** 3 * np.finfo(float).eps
    assert all(abs(a - b) <= tol * b for a, b in zip(r.rms_err, rc.rms_err)), what
    if traces:
        assert same_bits(s.traces().numpy(), tr), f"{what}: traces differ from CpuSolver"


@pytest.mark.parametrize("check_every", [1, 4])
@pytest.mark.parametrize("mode", ["eigen", "initial", "receivers"])
@pytest.mark.parametrize("opts", list(OPTIONS))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_solves_are_the_cpu_solvers(gpu, grid, opts, mode, check_every):
    K = 23
    s = _arm(Solver(_spec(grid, K, check_every), backend="hip", device=0, **OPTIONS[opts]), grid, mode)
    ref = _cpu(grid, K, mode, check_every)
    _check(s, s.run(), ref, "first run", mode == "receivers")
    _check(s, s.run(), ref, "second run (graph replay)", mode == "receivers")


def test_long_solve(gpu):
    s = Solver(_spec("N40-box", 203, 2), backend="hip", device=0)
    _check(s, s.run(), _cpu("N40-box", 203, "eigen", 2), "K = 203", False)


def test_a_forced_solve_over_the_limit_is_reported_as_a_blow_up(gpu):
    # at 1.1 of the limit the stiffest mode of the N = 16 grid has z = 14.35 and grows by 4.6 per step: overflow before
    # step 500 from random data, and before step 600 from the eigenmode's rounding noise alone
    N = 16
    tau = 1.1 * 1.5 * ProblemSpec(N=N).tau_max
    spec = ProblemSpec(N=N, tau=tau, K=500, check_every=100, order=4, time_order=4)
    out = []
    for backend in (dict(backend="cpu"), dict(backend="hip", device=0)):
        s = Solver(spec, force=True, **backend)
        s.set_initial(*lcg_fields(N))
        out.append(s.run())
    assert not out[0].finite and not out[1].finite and out[0].steps == out[1].steps
    assert [np.isfinite(m) for m in out[0].max_err] == [np.isfinite(m) for m in out[1].max_err]
    p = subprocess.run([os.path.join(ROOT, "bin", "wave3d"), str(N), repr(tau), "600", "--order", "4", "--time-order", "4",
                        "--force", "--quiet"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 3, p.stdout + p.stderr


def test_time_order_2_given_explicitly_changes_nothing(gpu):
    for order in (2, 4):
        a = Solver(ProblemSpec(N=24, tau=1e-3, K=23, order=order), backend="hip", device=0)
        b = Solver(ProblemSpec(N=24, tau=1e-3, K=23, order=order, time_order=2), backend="hip", device=0)
        ra, rb = a.run(), b.run()
        assert ra.max_err == rb.max_err and ra.rms_err == rb.rms_err
        assert list(a.native.unit_steps) == list(b.native.unit_steps)
        assert (a.native.field_hash(0), a.native.field_hash(1)) == (b.native.field_hash(0), b.native.field_hash(1))
        assert a.native.analytic_start == b.native.analytic_start


def test_refusals(gpu):
    from mpi_cuda_amd._native import load

    C = load()
    N = 24
    spec = _spec("N24-cube", 23, 2)
    one = np.ones((N + 1,) * 3)
    nodes, w = np.array([[3, 4, 5]], dtype=np.int64), np.ones((23, 1))

    def native(world=1, **opts):
        o = C.SolverOptions()
        for k, v in opts.items():
            setattr(o, k, v)
        return C.GpuSolver(spec.native(), o, 0, world, None)

    # what order = 4 refuses stays refused, with its messages
    for kw, msg in ((dict(fake_comm=True, world=2), "order: order = 4 runs on one GPU rank"),
                    (dict(fake_comm=True), "order: not on a fake rank"), (dict(push=True), "order: not on the push or copy"),
                    (dict(sdma=True), "order: not on the push or copy")):
        with pytest.raises(RuntimeError, match="^wave3d: " + msg):
            native(**kw)
    with pytest.raises(RuntimeError, match="^wave3d: order: order = 4 runs on one GPU rank only, not in a GpuGroup"):
        C.GpuGroup(spec.native(), C.SolverOptions(), 2, "loopback")
    s = native()
    with pytest.raises(RuntimeError, match="^wave3d: order: no speed field"):
        s.set_speed(one.reshape(-1))
    with pytest.raises(RuntimeError, match="^wave3d: order: not together with set_state"):
        s.set_state(np.zeros((N + 1) ** 3), np.zeros((N + 1) ** 3), 3)
    # point sources: new with the time order
    with pytest.raises(RuntimeError, match="^wave3d: time_order: no point sources"):
        s.set_sources(nodes, w)
    s.run()
    with pytest.raises(RuntimeError, match="^wave3d: order: the second-order discrete energy"):
        s.energy(0)
    hip = dict(backend="hip", device=0)
    for kw, msg in ((dict(transport="loopback", world=2, rank=0), "order: order = 4 runs on one rank only"),
                    (dict(runtime="process"), "order: order = 4 not with runtime"),
                    (dict(copy_engines=True), "order: order = 4 runs on one GPU rank"),
                    (dict(speed=one), "order: no speed field")):
        with pytest.raises(ValueError, match=msg):
            Solver(spec, **hip, **kw)
    t = Solver(spec, **hip)
    for call, msg in ((lambda: t.energy(0), "order: the second-order discrete energy"),
                      (lambda: t.set_speed(one), "order: no speed field"),
                      (lambda: t.set_state(one, one, 3), "order: order = 4 not together"),
                      (lambda: t.set_sources(nodes, w), "time_order: no point sources")):
        with pytest.raises(ValueError, match=msg):
            call()
    # the CFL guard at the new limit: just under 3/2 of tau_max runs, just over is refused, and runs when forced
    lim = ProblemSpec(N=N).tau_max * 1.5
    kw = dict(N=N, K=5, order=4, time_order=4)
    Solver(ProblemSpec(tau=0.999 * lim, **kw), **hip).run()
    with pytest.raises(ValueError, match="CFL violated: courant = .* for order = 4, time_order = 4"):
        Solver(ProblemSpec(tau=1.001 * lim, **kw), **hip)
    Solver(ProblemSpec(tau=1.001 * lim, **kw), force=True, **hip).run()
    with pytest.raises(ValueError, match="CFL violated: courant = .* > sqrt\\(3\\)/2 for order = 4 \\(effective"):
        Solver(ProblemSpec(N=N, tau=0.999 * lim, K=5, order=4), **hip)  # ((4, 2) keeps its own limit)


@pytest.mark.parametrize("cli", ["native", "python"])
def test_cli_dump_equals_the_api(gpu, tmp_path, cli):
    N, K = 24, 23
    spec = _spec("N24-cube", K, 2)
    out, js = str(tmp_path / "out"), str(tmp_path / "summary.json")
    common = [str(N), repr(spec.tau), str(K), "--order", "4", "--time-order", "4", "--dump", out, "--json", js, "--quiet"]
    if cli == "python":
        cmd = [sys.executable, "-m", "mpi_cuda_amd", *common, "--backend", "hip"]
    else:
        cmd = [os.path.join(ROOT, "bin", "wave3d"), *common]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    f, meta = dumpio.load(out)
    assert same_bits(f, _cpu("N24-cube", K, "eigen", 2)[0])
    assert meta["time_order"] == 4 and meta["space_order"] == 4 and json.load(open(js))["time_order"] == 4
    # without --time-order this tau is refused (CFL of the (4, 2) scheme)
    i = cmd.index("--time-order")
    p = subprocess.run(cmd[:i] + cmd[i + 2:], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "CFL violated" in p.stderr
