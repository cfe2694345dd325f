"""Order-4 solves on one GPU rank against CpuSolver, the definition: u^K, u^{K-1}, the error log's steps and Max Error column and the traces bit for bit (the L2 column to summation order).

N = 24 (cube) and N = 40 (box 1 x 1.3 x 0.7), K = 23, check cadence 1 and 4; the default options (temporal = 5, which an
order-4 solve turns into single steps), temporal = 1 and graph = False; first run and graph replay; the eigenmode start,
set_initial and a shot (sources + receivers); one K = 203 solve at N = 40. Every unit is a single step and no start is
analytic. The refusals that need no second process, and both CLIs against the API."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from long_reference import long_shot
from sources_common import BOX, lcg_fields, same_bits

from mpi_cuda_amd.models.wave3d import ProblemSpec
from mpi_cuda_amd.solver import Solver
from mpi_cuda_amd.utils import dump as dumpio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = {"N24-cube": (24, False), "N40-box": (40, True)}
OPTIONS = {"default": dict(), "temporal5": dict(temporal=5), "temporal1": dict(temporal=1), "nograph": dict(graph=False),
           "ty16": dict(tiling={"ty": 16})}


def _spec(grid, K, check_every):
    N, box = GRIDS[grid]
    s = ProblemSpec(N=N, tau=0.5 / (N * 3.2) if box else 0.5 / (N * 1.8), K=K, L=BOX[0] if box else 1.0,
                    check_every=check_every, Ly=BOX[1] if box else None, Lz=BOX[2] if box else None, order=4)
    assert s.cfl_ok
    return s


def _arm(s, grid, K, mode):
    N, box = GRIDS[grid]
    if mode == "initial":
        s.set_initial(*lcg_fields(N))
    if mode == "shot":
        shot = long_shot(N, box)
        s.set_initial(np.zeros((N + 1,) * 3))
        s.set_sources(shot.sources, np.ascontiguousarray(shot.w[:K]))
        s.set_receivers(shot.receivers)
    return s


@functools.lru_cache(maxsize=None)
def _cpu(grid, K, mode, check_every):
    s = _arm(Solver(_spec(grid, K, check_every), backend="cpu"), grid, K, mode)
    r = s.run()
    return (s.global_field(0).numpy().copy(), s.global_field(1).numpy().copy(), r,
            s.traces().numpy().copy() if mode == "shot" else None)


def _check(s, r, ref, what, traces):
    uK, uK1, rc, tr = ref
    assert s.native.unit_steps and set(s.native.unit_steps) == {1} and not s.native.analytic_start, what
    assert same_bits(s.global_field(0).numpy(), uK), f"{what}: u^K differs from CpuSolver"
    assert same_bits(s.global_field(1).numpy(), uK1), f"{what}: u^K-1 differs from CpuSolver"
    assert r.steps == rc.steps and r.max_err == rc.max_err, what
    # (the log's L2 column is sqrt of a sum of (N - 1)^3 non-negative squares that the workgroups and the CPU's planes add
    # in different orders: equal within (N - 1)^3 eps / 2, the worst case of reordering such a sum, as in every GPU test here)
    tol = (s.spec.N - 1) ** 3 * np.finfo(float).eps
    assert all(abs(a - b) <= tol * b for a, b in zip(r.rms_err, rc.rms_err)), what
    if traces:
        assert same_bits(s.traces().numpy(), tr), f"{what}: traces differ from CpuSolver"


@pytest.mark.parametrize("check_every", [1, 4])
@pytest.mark.parametrize("mode", ["eigen", "initial", "shot"])
@pytest.mark.parametrize("opts", list(OPTIONS))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_solves_are_the_cpu_solvers(gpu, grid, opts, mode, check_every):
    K = 23
    s = _arm(Solver(_spec(grid, K, check_every), backend="hip", device=0, **OPTIONS[opts]), grid, K, mode)
    ref = _cpu(grid, K, mode, check_every)
    _check(s, s.run(), ref, "first run", mode == "shot")
    _check(s, s.run(), ref, "second run (graph replay)", mode == "shot")


def test_the_eigenmode_converges_at_fourth_order(gpu):
    # (the error column keeps its meaning: odd reflection is exact for the sine mode)
    errs = []
    for N in (8, 16):
        r = Solver(ProblemSpec(N=N, tau=1e-4, K=200, order=4), backend="hip", device=0).run()
        errs.append(r.max_err[-1])
    assert 14.0 <= errs[0] / errs[1] <= 18.0


def test_long_solve(gpu):
    s = Solver(_spec("N40-box", 203, 2), backend="hip", device=0)
    _check(s, s.run(), _cpu("N40-box", 203, "eigen", 2), "K = 203", False)


def test_order2_given_explicitly_changes_nothing(gpu):
    a = Solver(ProblemSpec(N=24, tau=1e-3, K=23), backend="hip", device=0)
    b = Solver(ProblemSpec(N=24, tau=1e-3, K=23, order=2), backend="hip", device=0)
    ra, rb = a.run(), b.run()
    assert ra.max_err == rb.max_err and ra.rms_err == rb.rms_err and list(a.native.unit_steps) == list(b.native.unit_steps)
    assert (a.native.field_hash(0), a.native.field_hash(1)) == (b.native.field_hash(0), b.native.field_hash(1))
    assert a.native.analytic_start == b.native.analytic_start


def test_refusals(gpu):
    from mpi_cuda_amd._native import load

    C = load()
    N = 24
    spec = _spec("N24-cube", 23, 2)

    def native(world=1, **opts):
        o = C.SolverOptions()
        for k, v in opts.items():
            setattr(o, k, v)
        return C.GpuSolver(spec.native(), o, 0, world, None)

    for kw, msg in ((dict(fake_comm=True, world=2), "order: order = 4 runs on one GPU rank"),
                    (dict(fake_comm=True), "order: not on a fake rank"), (dict(push=True), "order: not on the push or copy"),
                    (dict(sdma=True), "order: not on the push or copy")):
        with pytest.raises(RuntimeError, match="^wave3d: " + msg):
            native(**kw)
    with pytest.raises(RuntimeError, match="^wave3d: order: order = 4 runs on one GPU rank only, not in a GpuGroup"):
        C.GpuGroup(spec.native(), C.SolverOptions(), 2, "loopback")
    with pytest.raises(RuntimeError, match="^wave3d: order: no sponge"):
        C.Problem(N, spec.tau, 23, 1.0, sponge=C.Sponge(5, 0.0, 63), order=4)
    with pytest.raises(RuntimeError, match="^wave3d: order: the spatial order must be 2 or 4"):
        C.Problem(N, spec.tau, 23, 1.0, order=3)
    s = native()
    with pytest.raises(RuntimeError, match="^wave3d: order: no speed field"):
        s.set_speed(np.ones((N + 1) ** 3))
    with pytest.raises(RuntimeError, match="^wave3d: order: not together with set_state"):
        s.set_state(np.zeros((N + 1) ** 3), np.zeros((N + 1) ** 3), 3)
    s.run()
    with pytest.raises(RuntimeError, match="^wave3d: order: the second-order discrete energy"):
        s.energy(0)
    hip = dict(backend="hip", device=0)
    for kw, msg in ((dict(transport="loopback", world=2, rank=0), "order: order = 4 runs on one rank only"),
                    (dict(runtime="process"), "order: order = 4 not with runtime"),
                    (dict(copy_engines=True), "order: order = 4 runs on one GPU rank"),
                    (dict(speed=np.ones((N + 1,) * 3)), "order: no speed field")):
        with pytest.raises(ValueError, match=msg):
            Solver(spec, **hip, **kw)
    t = Solver(spec, **hip)
    for call, msg in ((lambda: t.energy(0), "order: the second-order discrete energy"),
                      (lambda: t.set_speed(np.ones((N + 1,) * 3)), "order: no speed field"),
                      (lambda: t.set_state(np.zeros((N + 1,) * 3), np.zeros((N + 1,) * 3), 3), "order: order = 4 not together")):
        with pytest.raises(ValueError, match=msg):
            call()
    # the CFL guard at the new limit: just under sqrt(3)/2 of tau_max runs, just over is refused, and runs when forced
    lim = ProblemSpec(N=N).tau_max * np.sqrt(3.0) / 2.0
    Solver(ProblemSpec(N=N, tau=0.999 * lim, K=5, order=4), **hip)
    with pytest.raises(ValueError, match="CFL violated: courant = .* for order = 4"):
        Solver(ProblemSpec(N=N, tau=1.001 * lim, K=5, order=4), **hip)
    Solver(ProblemSpec(N=N, tau=1.001 * lim, K=5, order=4), force=True, **hip)
    Solver(ProblemSpec(N=N, tau=1.001 * lim, K=5), **hip)  # (order 2 at the same tau is untouched)


@pytest.mark.parametrize("cli", ["native", "python"])
def test_cli_dump_equals_the_api(gpu, tmp_path, cli):
    N, K = 24, 23
    spec = _spec("N24-cube", K, 2)
    out, js = str(tmp_path / "out"), str(tmp_path / "summary.json")
    common = [str(N), repr(spec.tau), str(K), "--order", "4", "--dump", out, "--json", js, "--quiet"]
    if cli == "python":
        cmd = [sys.executable, "-m", "mpi_cuda_amd", *common, "--backend", "hip"]
    else:
        cmd = [os.path.join(ROOT, "bin", "wave3d"), *common]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    f, meta = dumpio.load(out)
    assert same_bits(f, _cpu("N24-cube", K, "eigen", 2)[0])
    assert meta["space_order"] == 4 and meta["order"] == "C" and json.load(open(js))["order"] == 4
    # without --order the sidecars do not name it
    p = subprocess.run([c for c in cmd if c not in ("--order", "4")], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "space_order" not in dumpio.load(out)[1] and "order" not in json.load(open(js))
