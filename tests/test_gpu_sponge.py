"""Sponge layers on one GPU rank against CpuSolver, the definition: N = 40, K = 23, every pass depth (temporal = 1..5, the
fused units followed by k_sponge_box), both single-step kernels (the DAMP instantiations), first run / graph replay /
run_batch, keep_prev, eigenmode start and seeded random set_initial. Both stored levels are bit for bit CpuSolver's, the
energy agrees within the summation rule of tests/test_gpu_initial.py, a shot recorded outside the layers' reach gives
CpuSolver's traces (bit for bit on single steps; on fused passes within the sources tolerance rule max(8 d_split,
16 eps umax) of tests/sources_common.py, with d_split — the rounding of the split identity "forced damped solve = unforced
damped passes + responses" on the CPU — computed here for this shot as csrc/tests/test_sources.cpp computes it), the
refusals that need no second process, and one K = 203 solve on the default schedule. One source and one receiver sit at
the smallest distance the solver allows, W + temporal + 1 = 12 nodes from a damped face: at temporal = 5 the source's ball
(radius 4) overlaps the recomputed slabs d < 10, so the order pass, k_sponge_box, source correction is exercised."""
import dataclasses
import functools

import numpy as np
import pytest

from long_reference import long_spec, ricker16
from sources_common import EPS, lcg_fields, same_bits

from mpi_cuda_amd.solver import Solver

pytestmark = pytest.mark.gpu

N, K = 40, 23
SPONGES = {"all6": (6, 0.0, 63), "xXz-box": (7, 0.0, "xXz")}
U = 2.0 ** -53


def _spec(name, K_=K):
    return dataclasses.replace(long_spec(N, name.endswith("box"), K=K_, check_every=2), sponge=SPONGES[name])


@functools.lru_cache(maxsize=None)
def _cpu(name, random, K_=K):
    s = Solver(_spec(name, K_), backend="cpu")
    if random:
        s.set_initial(*lcg_fields(N))
    s.run()
    return (s.global_field(0).numpy().copy(), s.global_field(1).numpy().copy(), s.energy(0),
            s.energy(1) if random else None)


def _check(s, name, random, K_=K, what=""):
    uK, uK1, eK, e1 = _cpu(name, random, K_)
    assert same_bits(s.global_field(0).numpy(), uK), f"{what}: u^K differs from CpuSolver"
    assert same_bits(s.global_field(1).numpy(), uK1), f"{what}: u^K-1 differs from CpuSolver"
    from mpi_cuda_amd._native import load

    C = load()
    c = C.cpu_energy(s.spec.native(), s.native.layout, s.native.download(1), s.native.download(0))
    tol = (C.gpu_energy_depth(s.native.layout) + 8) * U * c["abs_terms"]
    assert c["E"] == eK and abs(s.energy(0) - eK) <= tol, (what, s.energy(0), eK, tol)
    if random:
        assert abs(s.energy(1) - e1) <= tol * max(1.0, e1 / eK), (what, s.energy(1), e1)


SCHEDULES = {"t1-rq": dict(temporal=1), "t1-lds": dict(temporal=1, tiling={"variant": 0}), "t2": dict(temporal=2),
             "t3": dict(temporal=3), "t4": dict(temporal=4), "t5": dict(temporal=5),
             "t5-keep": dict(temporal=5, keep_prev=True), "t3-nograph": dict(temporal=3, graph=False)}


@pytest.mark.parametrize("random", [False, True], ids=["eigenmode", "random"])
@pytest.mark.parametrize("name", list(SPONGES))
@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_fields_are_the_cpu_solvers(gpu, sched, name, random):
    """First run (eager or the capture's first replay), a second run (graph replay) and run_batch(2): the same bits."""
    s = Solver(_spec(name), backend="hip", device=0, **SCHEDULES[sched])
    assert s.native.sponge and s.native.stored_prev
    if random:
        s.set_initial(*lcg_fields(N))
    for what in ("first run", "second run"):
        s.run()
        assert not s.native.analytic_start and s.native.stored_prev
        _check(s, name, random, what=f"{sched} {what}")
    s.run_batch(2)
    _check(s, name, random, what=f"{sched} run_batch")
    t = s.native.traffic()
    plain = Solver(dataclasses.replace(_spec(name), sponge=None), backend="hip", device=0, **SCHEDULES[sched])
    if random:
        plain.set_initial(*lcg_fields(N))
    plain.run()
    assert not same_bits(plain.global_field(0).numpy(), _cpu(name, random)[0])  # (the layers do something)
    if SCHEDULES[sched]["temporal"] >= 2:  # (fused units: the recomputation's compulsory bytes are counted)
        assert t["field_bytes"] > plain.native.traffic()["field_bytes"]
    else:
        assert t["field_bytes"] >= plain.native.traffic()["field_bytes"]


# ---- a shot with receivers outside the reach ---------------------------------------------------------------------------------
def _shot():
    tau = _spec("all6").tau
    # (the third: 12 nodes from x-, 12 from z+, the smallest distance allowed at W = 6, temporal = 5)
    src = np.array([[20, 20, 20], [18, 22, 19], [12, 14, 28]], dtype=np.int64)
    w = np.stack([ricker16(6.0, 0.12, tau, K), ricker16(8.0, 0.1, tau, K, -0.5), ricker16(7.0, 0.08, tau, K, 0.75)], axis=1)
    rec = np.array([[20, 20, 20], [21, 20, 20], [12, 12, 12], [28, 27, 13], [19, 23, 20], [12, 28, 20]], dtype=np.int64)
    return src, np.ascontiguousarray(w), rec


def _armed(s):
    src, w, rec = _shot()
    s.set_initial(np.zeros((N + 1,) * 3), None)
    s.set_sources(src, w)
    s.set_receivers(rec)
    s.run()
    return s


@functools.lru_cache(maxsize=None)
def _cpu_shot():
    return _armed(Solver(_spec("all6"), backend="cpu"))


@functools.lru_cache(maxsize=None)
def _split(steps):
    """(d_split, umax) of this shot for passes of `steps` steps, as csrc/tests/test_sources.cpp check_split forms them:
    from the zero start, damped cpu_leapfrog passes without forcing plus cpu_source_response added to both levels after
    each pass, against CpuSolver's forced solve; d_split = the largest difference on the two last levels, umax = the
    largest |u| over those and over the levels at every pass boundary."""
    from mpi_cuda_amd._native import load

    C = load()
    spec = _spec("all6")
    prob = spec.native()
    lay = C.make_layout(prob, C.rank_box(prob, C.Dims(1, 1, 1), 0))
    co = C.Coeffs.from_problem(prob)
    s_ext = C.sin_table_ext(prob)
    src, w, _ = _shot()
    a = np.array([[C.source_addend(prob, float(w[m, q])) for q in range(len(src))] for m in range(K)])
    r = np.arange(-5, 6)
    cube = r[:, None, None] * int(lay.plane) + r[None, :, None] * int(lay.pitch) + r[None, None, :]
    u = [np.zeros(int(lay.total)), np.zeros(int(lay.total))]  # u^{n-1}, u^n

    def add(n, s, start):
        for q, node in enumerate(src.tolist()):
            last, prev = C.cpu_source_response(prob, co, node, np.ascontiguousarray(a[n:n + s, q]), start, s)
            at = int(lay.off(*node)) + cube  # (every ball lies inside the interior: the sources are 12 nodes from the faces)
            u[1][at] += last
            u[0][at] += prev

    add(0, 1, True)
    n, umax = 1, 0.0
    while n < K:
        s = min(steps, K - n)
        for _ in range(s):
            C.cpu_leapfrog(lay, co, u[1], u[0], C.compute_box(lay), s_ext, sponge=prob)
            u.reverse()
        add(n, s, False)
        n += s
        umax = max(umax, float(np.abs(u[0]).max()), float(np.abs(u[1]).max()))
    ref = _cpu_shot()._impl
    d = max(float(np.abs(ref.field(0) - u[1]).max()), float(np.abs(ref.field(1) - u[0]).max()))
    return d, max(umax, float(np.abs(ref.field(0)).max()), float(np.abs(ref.field(1)).max()))


@pytest.mark.parametrize("temporal", [1, 3, 5])
def test_shot_and_traces(gpu, temporal):
    """W = 6, temporal <= 5: every source and receiver is 12 nodes or more from every face, outside W + temporal = 11."""
    c = _cpu_shot()
    s = _armed(Solver(_spec("all6"), backend="hip", device=0, temporal=temporal))
    tc, ts = c.traces().numpy(), s.traces().numpy()
    assert float(np.abs(tc).max()) > 0 and np.isfinite(ts).all()
    if temporal == 1:
        assert same_bits(ts, tc) and same_bits(s.global_field(0).numpy(), c.global_field(0).numpy())
        return
    d_split, umax = _split(temporal)
    b = max(8.0 * d_split, 16.0 * EPS * umax)  # (sources_common.tolerance's rule)
    print(f"SPONGE gpu shot temporal={temporal}: d_split = {d_split:.3e} umax = {umax:.3e}")
    for what, d in (("traces", np.abs(ts - tc).max()), ("u^K", np.abs(s.global_field(0).numpy() - c.global_field(0).numpy()).max()),
                    ("u^K-1", np.abs(s.global_field(1).numpy() - c.global_field(1).numpy()).max())):
        print(f"SPONGE gpu shot temporal={temporal} {what}: max |gpu - cpu| = {d:.3e} bound {b:.3e}")
        assert d <= b, (what, d, b)


def test_refusals(gpu):
    from mpi_cuda_amd._native import load

    C = load()
    spec = _spec("all6")
    o = C.SolverOptions()
    with pytest.raises(RuntimeError, match="^wave3d: sponge: one GPU rank only"):
        C.GpuSolver(spec.native(), o, 0, 2, None)
    with pytest.raises(RuntimeError, match="^wave3d: sponge: one GPU rank only"):
        C.GpuGroup(spec.native(), o, 2, "loopback")
    for attr, msg in (("fake_comm", "fake rank"), ("push", "push or copy-engine"), ("sdma", "push or copy-engine")):
        o = C.SolverOptions()
        setattr(o, attr, True)
        with pytest.raises(RuntimeError, match="^wave3d: sponge: not on .*" + msg):
            C.GpuSolver(spec.native(), o, 0, 1, None)
    o = C.SolverOptions()
    o.tb = False
    with pytest.raises(RuntimeError, match="^wave3d: sponge: tb = false"):
        C.GpuSolver(spec.native(), o, 0, 1, None)
    o = C.SolverOptions()
    o.tiling.rows = 8  # (k_leapfrog_rq<8> spills its damped form)
    with pytest.raises(RuntimeError, match="^wave3d: sponge: the register-queue single step with 8 rows"):
        C.GpuSolver(spec.native(), o, 0, 1, None)
    with pytest.raises(ValueError, match="sponge: tb=False"):
        Solver(spec, backend="hip", device=0, tb=False)
    with pytest.raises(ValueError, match="sponge: one rank only"):
        Solver(spec, backend="hip", transport="loopback", world=2, rank=0, device=0)
    s = Solver(spec, backend="hip", device=0, temporal=4)
    with pytest.raises(RuntimeError, match="^wave3d: sponge: receiver 1 lies 10 nodes from a damped face, within width \\+ temporal = 10"):
        s.set_receivers(np.array([[20, 20, 20], [20, 30, 20]]))
    s.set_receivers(np.array([[20, 29, 20]]))  # 11 nodes: outside the reach
    with pytest.raises(RuntimeError, match="^wave3d: sponge: source 0 lies 9 nodes"):
        s.set_sources(np.array([[9, 20, 20]]), np.zeros((K, 1)))
    # a face that is not damped does not count
    t = Solver(dataclasses.replace(spec, sponge=(6, 0.0, "xX")), backend="hip", device=0)
    t.set_receivers(np.array([[20, 1, 39]]))


def test_long_solve_on_the_default_schedule(gpu):
    """K = 203 (40 five-step units and their k_sponge_box launches, past every buffer rotation), seeded random data."""
    s = Solver(_spec("xXz-box", 203), backend="hip", device=0)
    s.set_initial(*lcg_fields(N))
    s.run()
    _check(s, "xXz-box", True, 203, "K=203")
    s.run()
    _check(s, "xXz-box", True, 203, "K=203 replay")
