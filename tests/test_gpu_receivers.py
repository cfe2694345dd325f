"""Receivers at solve level: GpuSolver / GpuGroup traces on the production schedules against the CPU solver's traces
(bit for bit) and, independently of the CPU record code, against fields: rows K and K - 1 are the solve's own
global_field(0 / 1) at the nodes, row n is global_field(0) of a K = n solve without receivers.

N in {40, 77}, K = 12 (temporal = 5: full passes and a short last one), tau = tau_max / 2, random phi and psi through
set_initial unless a case says otherwise. The groups run with poison_ghosts, so a cone enqueued before its inputs'
ghosts arrived, or reading a ghost the exchange does not deliver, records NaN."""
import functools

import numpy as np
import pytest

from receivers_common import (at_nodes, cpu_fields, cpu_traces, initial_data, receiver_set, same_bits, spec_for,
                              state_at)

from mpi_cuda_amd.solver import Solver

pytestmark = pytest.mark.gpu

K = 12
SIZES = [40, 77]


def _solver(N, Kk=K, **kw):
    return Solver(spec_for(N, Kk), backend="hip", device=0, **kw)


@functools.lru_cache(maxsize=None)
def _gpu_field(N, n):
    """u^n at every node from a one-rank GPU solve of K = n WITHOUT receivers (random data)."""
    s = _solver(N, n)
    s.set_initial(*initial_data(N))
    s.run()
    return s.global_field(0).numpy().copy()


def _check(s, N, nodes, want, what, rows_from=0):
    tr = s.traces().numpy()
    assert tr.shape == (K + 1, len(nodes)), what
    assert np.isnan(tr[:rows_from]).all(), what
    bad = np.argwhere(tr[rows_from:].view(np.int64) != want[rows_from:].view(np.int64))
    assert bad.size == 0, (what, len(bad), bad[:5].tolist(), int(np.isnan(tr[rows_from:]).sum()))
    # independent of the CPU record code: the solve's own stored fields
    assert same_bits(tr[K], at_nodes(s.global_field(0).numpy(), nodes)), what
    assert same_bits(tr[K - 1], at_nodes(s.global_field(1).numpy(), nodes)), what
    return tr


ONE_RANK = {"p2": dict(temporal=5), "single": dict(temporal=1), "lf2": dict(tb=False),
            "keep": dict(temporal=5, keep_prev=True)}


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("sched", list(ONE_RANK))
def test_one_rank_traces(gpu, N, sched):
    nodes, want = cpu_traces(N, K)
    s = _solver(N, **ONE_RANK[sched])
    s.set_initial(*initial_data(N))
    s.set_receivers(nodes)
    assert s.native.mode == ("single-step" if sched == "single" else "fused-single")
    s.run()
    assert not s.native.analytic_start
    if sched in ("p2", "keep"):
        assert s.native.stored_prev == (sched == "keep")
    tr = _check(s, N, nodes, want, f"N={N} {sched}")
    for n in (3, 7):
        assert same_bits(tr[n], at_nodes(_gpu_field(N, n), nodes)), n
        assert same_bits(tr[n], at_nodes(cpu_fields(N, n)[1], nodes)), n
    face = ((nodes == 0) | (nodes == N)).any(axis=1)
    assert same_bits(tr[:, face], np.zeros((K + 1, int(face.sum()))))


@pytest.mark.parametrize("N", SIZES)
def test_default_start_and_state(gpu, N):
    """The eigenmode start (init_first instead of the analytic pass), and set_state at n0 = 4: rows 3 and 4 are gathered
    from the uploaded fields, the rows below stay NaN."""
    nodes, want = cpu_traces(N, K, (1, 1, 1), "default")
    s = _solver(N)
    s.set_receivers(nodes)
    s.run()
    assert not s.native.analytic_start
    _check(s, N, nodes, want, "default start")
    _, want4 = cpu_traces(N, K, (1, 1, 1), "state4")
    _, full = cpu_traces(N, K)
    assert same_bits(want4[3:], full[3:])
    s.set_state(*state_at(N, 4), 4)
    s.run()
    _check(s, N, nodes, want4, "set_state", rows_from=3)


@pytest.mark.parametrize("Kk", [1, 2])
def test_short_solves(gpu, Kk):
    N = 40
    nodes = receiver_set(N)
    c = Solver(spec_for(N, Kk), backend="cpu")
    s = _solver(N, Kk)
    if Kk > 1:
        c.set_initial(*initial_data(N))
        s.set_initial(*initial_data(N))
    c.set_receivers(nodes)
    s.set_receivers(nodes)
    c.run()
    s.run()
    tr = s.traces().numpy()
    assert tr.shape == (Kk + 1, len(nodes)) and same_bits(tr, c.traces().numpy())
    assert same_bits(tr[Kk], at_nodes(s.global_field(0).numpy(), nodes))
    assert same_bits(tr[Kk - 1], at_nodes(s.global_field(1).numpy(), nodes))


GROUPS = {"slab4": (4, "slab", (4, 1, 1)), "block8": (8, "2x2x2", (2, 2, 2))}


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "seq"])
@pytest.mark.parametrize("transport", ["loopback", "rccl-self", "sdma"])
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("N", SIZES)
def test_group_traces(gpu, N, group, transport, overlap):
    world, decomp, dims = GROUPS[group]
    nodes, want = cpu_traces(N, K, dims)
    try:
        g = Solver(spec_for(N, K), backend="hip", transport=transport, world=world, rank=0, decomp=decomp, device=0,
                   overlap=overlap, poison_ghosts=True)
    except RuntimeError as e:  # (the copy engines exist for the LDS passes only: the N = 40 slabs run single steps)
        assert transport == "sdma" and "sdma transport" in str(e), e
        assert N == 40 and group == "slab4"
        return
    assert tuple(g.dims) == dims
    g.set_initial(*initial_data(N))
    g.set_receivers(nodes)
    what = f"N={N} {group} {transport} overlap={overlap} mode={g.native.mode()}"
    for i in range(2):  # (eager, then the captured group solve where the runtime captures groups)
        g.run()
        tr = _check(g, N, nodes, want, f"{what} run {i}")
    for n in (3, 7):
        assert same_bits(tr[n], at_nodes(_gpu_field(N, n), nodes)), (what, n)


def test_replay_batch_energy_and_removal(gpu):
    N = 77
    nodes, want = cpu_traces(N, K)
    plain = _solver(N)
    plain.set_initial(*initial_data(N))
    plain.run()
    s = _solver(N)
    s.set_initial(*initial_data(N))
    s.set_receivers(nodes)
    for i in range(2):  # eager capture + launch, then the replay
        s.run()
        _check(s, N, nodes, want, f"run {i}")
    assert s.native.graph_enabled
    rs, rp = s.run_batch(3), plain.run_batch(3)
    assert [r.extra["batched"] for r in rs] == [r.extra["batched"] for r in rp] == [True] * 3
    assert rs[-1].max_err == rp[-1].max_err
    _check(s, N, nodes, want, "run_batch")
    # energy(0) rebuilds u^{K-1} by relaunching the last unit: it records nothing and changes no trace
    assert not s.native.stored_prev
    before = s.traces().numpy().copy()
    assert s.energy(0) == plain.energy(0)
    assert same_bits(s.traces().numpy(), before) and same_bits(before, want)
    # a second list replaces the first; R = 0 restores the default solve
    s.set_receivers(nodes[:5])
    s.run()
    assert same_bits(s.traces().numpy(), want[:, :5])
    s.set_receivers(np.zeros((0, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        s.traces()
    fresh = _solver(N)
    d = _solver(N)
    d.set_receivers(nodes)
    d.run()
    assert not d.native.analytic_start
    d.set_receivers([])
    d.run()
    fresh.run()
    assert d.native.analytic_start and fresh.native.analytic_start
    for which in (0, 1):
        assert d.field_hash(which) == fresh.field_hash(which)
    assert same_bits(d.global_field(0).numpy(), fresh.global_field(0).numpy())


def test_refusals(gpu):
    N = 77
    nodes = receiver_set(N, (4, 1, 1))
    g = Solver(spec_for(N, K), backend="hip", transport="push", world=4, rank=0, decomp="slab", device=0)
    with pytest.raises(RuntimeError, match="push transport"):
        g.set_receivers(nodes)
    s = _solver(N)
    with pytest.raises(RuntimeError, match="outside the grid"):
        s.set_receivers([[1, 2, N + 1]])
    with pytest.raises(ValueError):
        s.traces()
