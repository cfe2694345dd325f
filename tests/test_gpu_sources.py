"""Point sources at solve level: GpuSolver / GpuGroup with set_sources against CpuSolver (the definition).

Single-step schedules apply the CPU definition itself (the ball of a one-step unit is the node): fields and traces are
bit-identical. Fused passes add the response of a zero field to the pass's forcing (k_source_cone), another evaluation
order of the same linear recurrence: fields u^K, u^{K-1} and every trace row agree within sources_common.tolerance =
max(8 d_split, 16 eps umax), d_split and umax printed by the native CPU program for these very solves (N = 40, K = 12,
tau = 0.005, SOURCES_40, seeded phi and psi; cube and box 1 x 1.3 x 0.7). The groups run with poison_ghosts: a ghost
plane that is not delivered, or a correction enqueued before the exchange it must follow, shows as NaN; a ghost
corrected twice or not at all as an error of the size of the addend, some 1e13 tolerances."""
import numpy as np
import pytest

from sources_common import (K40, N40, SOURCES_40, cpu_reference, lcg_fields, receivers_around, same_bits, spec40,
                            tolerance, wavelet)

from mpi_cuda_amd import ProblemSpec
from mpi_cuda_amd.solver import Solver

pytestmark = pytest.mark.gpu

W40 = wavelet(K40, len(SOURCES_40))
REC40 = receivers_around(SOURCES_40, N40)


def _armed(s, N=N40, nodes=SOURCES_40, w=W40, rec=REC40):
    s.set_initial(*lcg_fields(N))
    s.set_sources(nodes, w)
    s.set_receivers(rec)
    return s


def _fields(s):
    return s.global_field(0).numpy().copy(), s.global_field(1).numpy().copy(), s.traces().numpy().copy()


def _close(got, box, what):
    tol = tolerance(box)
    for g, w, name in zip(got, cpu_reference(box), ("u^K", "u^{K-1}", "traces")):
        assert g.shape == w.shape and not np.isnan(g).any(), (what, name)
        d = float(np.abs(g - w).max())
        print(f"{what} {name}: max |gpu - cpu| = {d:.3e} (tolerance {tol:.3e})")
        assert d <= tol, (what, name, d, tol)


def test_single_step_bit_identical(gpu):
    """temporal = 1 at N = 24, K = 7: every unit is one step, the correction is u[node] += a — the CPU definition."""
    N, K = 24, 7
    spec = ProblemSpec(N=N, tau=0.008, K=K, L=1.0)
    nodes = np.array([[12, 11, 13], [1, 1, 1], [23, 8, 20], [12, 12, 14], [12, 11, 13]], dtype=np.int64)
    w, rec = wavelet(K, len(nodes)), receivers_around(nodes, N)
    c = _armed(Solver(spec, backend="cpu"), N, nodes, w, rec)
    s = _armed(Solver(spec, backend="hip", device=0, temporal=1), N, nodes, w, rec)
    assert s.native.mode == "single-step" and s.sources == len(nodes) and s.native.sources == len(nodes)
    c.run()
    for i in range(2):  # (capture + launch, then the replay)
        s.run()
        for got, want in zip(_fields(s), _fields(c)):
            assert same_bits(got, want), i
    assert not s.native.analytic_start and s.native.stored_prev


FUSED = {"tb2": dict(temporal=2, tiling_tb={"p2": False}), "tb3": dict(temporal=3, tiling_tb={"p2": False}),
         "tb4": dict(temporal=4, tiling_tb={"p2": False}), "p2_2": dict(temporal=2), "p2_3": dict(temporal=3),
         "p2_4": dict(temporal=4), "p2_5": dict(temporal=5), "lf2": dict(tb=False)}


@pytest.mark.parametrize("box", [False, True], ids=["cube", "box"])
@pytest.mark.parametrize("sched", list(FUSED))
def test_fused_one_rank(gpu, sched, box):
    s = _armed(Solver(spec40(box), backend="hip", device=0, **FUSED[sched]))
    assert s.native.mode == "fused-single"
    s.run()
    assert not s.native.analytic_start and s.native.stored_prev
    first = _fields(s)
    _close(first, box, f"{sched} box={box}")
    # the replay of the captured graph and a pipelined batch: the same bits (the per-solve NaN fill of the traces and
    # the corrections are nodes of the graph)
    s.run()
    assert all(same_bits(a, b) for a, b in zip(_fields(s), first))
    assert s.native.graph_enabled
    rs = s.run_batch(3)
    assert [r.extra["batched"] for r in rs] == [True] * 3
    assert all(same_bits(a, b) for a, b in zip(_fields(s), first))
    # energy() works (and rebuilds nothing: both levels are stored)
    assert np.isfinite(s.energy(0)) and np.isfinite(s.energy(1))
    assert all(same_bits(a, b) for a, b in zip(_fields(s), first))


GROUPS = {"slab4": (4, "slab", (4, 1, 1), {}), "slab4tb": (4, "slab", (4, 1, 1), dict(tb_min_planes=8)),
          "block8": (8, "2x2x2", (2, 2, 2), {})}
_group_bits = {}


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "seq"])
@pytest.mark.parametrize("transport", ["loopback", "rccl-self"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_groups(gpu, group, transport, overlap):
    """SOURCES_40 has sources on the first plane of a slab, one node from a slab face, and on the corner of the 2x2x2
    blocks: their balls cross rank faces, edges and corners. Ranks that run single steps reproduce CpuSolver (and the
    one-rank temporal = 1 GPU solve) bit for bit. Ranks on the LDS passes split the steps into other units than one
    rank does, so their responses are rounded differently from the one-rank solve's: they are held to the CPU
    tolerance, and to bit equality between transports and between the eager and the captured solve."""
    world, decomp, dims, kw = GROUPS[group]
    g = Solver(spec40(False), backend="hip", transport=transport, world=world, rank=0, decomp=decomp, device=0,
               overlap=overlap, poison_ghosts=True, **kw)
    assert tuple(g.dims) == dims
    _armed(g)
    mode = g.native.mode()
    assert mode == {"slab4": "single-step", "slab4tb": "deep-tb", "block8": "deep-tb-block"}[group]
    what = f"{group} {transport} overlap={overlap}"
    g.run()
    first = _fields(g)
    assert g.native.stored_prev(0) and g.native.sources == len(SOURCES_40)
    if mode == "single-step":
        assert all(same_bits(a, b) for a, b in zip(first, cpu_reference(False))), what
        one = _armed(Solver(spec40(False), backend="hip", device=0, temporal=1))
        one.run()
        assert all(same_bits(a, b) for a, b in zip(first, _fields(one))), what
    else:
        _close(first, False, what)
    g.run()  # (the captured group solve where the runtime captures groups)
    assert all(same_bits(a, b) for a, b in zip(_fields(g), first)), what
    # the same units on every transport and with either exchange order: the same bits
    ref = _group_bits.setdefault(group, first)
    assert all(same_bits(a, b) for a, b in zip(first, ref)), what


def test_removal_restores_the_plain_solve(gpu):
    """Q = 0 after Q > 0: the analytic start and the dropped u^{K-1} come back, the fields are a fresh solver's."""
    fresh = Solver(spec40(False), backend="hip", device=0)
    fresh.run()
    s = Solver(spec40(False), backend="hip", device=0)
    s.set_sources(SOURCES_40, W40)
    s.run()
    assert not s.native.analytic_start and s.native.stored_prev
    assert not same_bits(s.global_field(0).numpy(), fresh.global_field(0).numpy())
    s.set_sources(np.zeros((0, 3), dtype=np.int64), np.zeros((K40, 0)))
    assert s.sources == 0 and s.native.sources == 0
    s.run()
    assert s.native.analytic_start == fresh.native.analytic_start and s.native.stored_prev == fresh.native.stored_prev
    for which in (0, 1):
        assert s.field_hash(which) == fresh.field_hash(which)
    assert same_bits(s.global_field(0).numpy(), fresh.global_field(0).numpy())


def test_refusals(gpu):
    """Every refusal of the GPU side but runtime="process" and --np > 1, which would start rank processes."""
    from mpi_cuda_amd._native import load

    C = load()
    N, K = 77, 12
    spec = ProblemSpec(N=N, tau=0.002, K=K, L=1.0)
    nodes, w = np.array([[30, 30, 30]], dtype=np.int64), np.ones((K, 1))
    g = Solver(spec, backend="hip", transport="push", world=4, rank=0, decomp="slab", device=0)
    with pytest.raises(RuntimeError, match="sources: not on the push transport"):
        g.set_sources(nodes, w)
    g = Solver(spec, backend="hip", transport="sdma", world=4, rank=0, decomp="slab", device=0)
    with pytest.raises(RuntimeError, match="sources: not on the copy-engine transport"):
        g.set_sources(nodes, w)
    g = Solver(spec, backend="hip", transport="loopback", world=4, rank=0, decomp="slab", device=0, deep_min_planes=3,
               tb=False)
    assert g.native.mode() == "deep-halo"
    with pytest.raises(RuntimeError, match="sources: the two-step deep-halo passes"):
        g.set_sources(nodes, w)
    o = C.SolverOptions()
    o.fake_comm = True
    r = C.GpuSolver(spec.native(), o, 0, 2, None)  # (a rank of a two-rank job, no transport)
    with pytest.raises(RuntimeError, match="sources: a fake rank"):
        r.set_sources(nodes, w)
    s = Solver(spec, backend="hip", device=0)
    f = np.zeros((N + 1,) * 3)
    s.set_sources(nodes, w)
    with pytest.raises(RuntimeError, match="sources: not together with set_state"):
        s.set_state(f, f, 4)
    t = Solver(spec, backend="hip", device=0)
    t.set_state(f, f, 4)
    with pytest.raises(RuntimeError, match="sources: not together with set_state"):
        t.set_sources(nodes, w)
    for bad in ([[0, 5, 5]], [[5, N, 5]], [[5, 5, N + 3]]):
        with pytest.raises(ValueError, match="sources:.*not strictly inside the grid"):
            s.set_sources(bad, w)
        with pytest.raises(RuntimeError, match="sources:.*not strictly inside the grid"):
            s.native.set_sources(np.array(bad, dtype=np.int64), w)
    with pytest.raises(ValueError, match=r"sources: w must have shape \(K, Q\)"):
        s.set_sources(nodes, np.ones((K + 1, 1)))
    wb = w.copy()
    wb[2, 0] = np.nan
    with pytest.raises(ValueError, match="sources:.*non-finite"):
        s.set_sources(nodes, wb)
    with pytest.raises(RuntimeError, match="sources:.*not finite"):
        s.native.set_sources(nodes, wb)
    assert s.sources == 1  # (a refused list leaves the earlier one in place)
