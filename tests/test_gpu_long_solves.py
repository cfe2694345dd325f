"""GPU solves of K = 203 steps at tau = 0.9 tau_max: ten times the step count of every other GPU test, so that the state
that grows with the number of units is used the way a real shot uses it — the ring of kTbRegions = 8 partial regions
wraps five times and more, the copy-engine flag table is walked to index 100, the error log, the trace buffer and the
sources' addend array have 200 rows, and the shot's wavefront crosses every rank face and comes back from the walls.

One rank (N = 40): every schedule x check cadence, keep_prev on and off, eigenmode and seeded random start, against
CpuSolver bit for bit (maxima and fields; 1e-12 for the fixed-order sums, as tests/test_gpu_solver.py), on the first
run, the graph replay and run_batch(3). The long shot of tests/test_long_solves_cpu.py with receivers: single steps bit
for bit, fused passes within long_reference.tolerance_long (the rule of sources_common.tolerance with the figures the
native CPU program prints for this shot); reciprocity; energy.

Groups on one GPU, from a random loaded state with receivers, every step checked, ghosts poisoned (rccl-self block ranks
excepted, as in tests/test_gpu_random_state.py), three solves in a row. The subset, chosen to stay under two minutes:
every transport on every layout it accepts at least once; pass depths 2 (the most units and exchanges: 101) and 5 (the
deepest ghosts) each on every layout; overlap and sequential exchange each on every transport.
  2 slabs, N = 66: loopback S5 overlap, sdma S5 seq, push S2 overlap, rccl-self S2 seq
  4 slabs, N = 66: loopback S2 seq, sdma S2 overlap, push S5 (runs 4) seq, rccl-self S5 overlap
  2x2x2,   N = 40: loopback S5 overlap, rccl-self S5 seq, sdma S2 overlap, sdma S5 seq, loopback S2 seq
  1x2x3,   N = 66: loopback S2 overlap, sdma S5 overlap, rccl-self S5 seq
(push takes slab ranks only; depth 2 runs K = 204: see test_groups_long.) With sources: 4 slabs and 2x2x2 at N = 40 over loopback and rccl-self, the only transports
that take sources, overlap on and off.
"""
import functools
import math

import numpy as np
import pytest
import torch

from long_reference import (EPS, K_LONG, bound, long_shot, long_spec, reciprocity_pair, tolerance_long)
from sources_common import lcg_fields, same_bits

from mpi_cuda_amd.solver import Solver

pytestmark = pytest.mark.gpu

K, N1 = K_LONG, 40
TB_REGIONS = 8  # (solver.hpp GpuSolver::kTbRegions)
SCHEDULES = {"S1": dict(temporal=1), "S2": dict(temporal=2), "S3": dict(temporal=3), "S4": dict(temporal=4),
             "S5": dict(temporal=5), "lf2": dict(tb=False), "tb4": dict(temporal=4, tiling_tb={"p2": False})}
DEPTH = {"S1": 1, "S2": 2, "S3": 3, "S4": 4, "S5": 5, "lf2": 2, "tb4": 4}


def _log_equal(r, want, what):
    assert r.steps == want.steps and r.finite, what
    assert r.max_err == want.max_err, what
    for n, a, b in zip(r.steps, r.rms_err, want.rms_err):
        assert math.isclose(a, b, rel_tol=1e-12), (what, n, a, b)


# ---- one rank, no sources ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_plain(check_every, start):
    c = Solver(long_spec(N1, False, K, check_every), backend="cpu")
    if start == "random":
        c.set_initial(*lcg_fields(N1))
    r = c.run()
    return r, c.owned_field(0), c.owned_field(1)


@pytest.mark.parametrize("check_every", [1, 2, 7, 0])
@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_one_rank_long(gpu, sched, check_every):
    """203 steps on one rank: error log, u^K and u^{K-1} equal CpuSolver's bit for bit, from the eigenmode (the analytic
    start pass included) and from seeded random data, with keep_prev on and off, on the first run, the graph replay and
    a pipelined batch of three. Catches a partial region read after the ring wrapped over it (a stale or overwritten
    region gives another step's error in the log), an error-log row written at the wrong step index, a pending reduction
    dropped at a wrap, a last pass whose dropped u^{K-1} is rebuilt from the wrong buffers after 40 rotations."""
    S = DEPTH[sched]
    steps = long_spec(N1, False, K, check_every).check_steps()
    if sched.startswith("S") and S >= 2 and check_every > 0:
        # units that hold a checked step each take a region: a unit of S steps holds at most ceil(S / check_every)
        assert math.ceil(len(steps) / math.ceil(S / check_every)) > 3 * TB_REGIONS
    for start in ("eigenmode", "random"):
        want, uK, uK1 = _cpu_plain(check_every, start)
        for keep_prev in (False, True):
            what = f"{sched} ce={check_every} {start} keep_prev={keep_prev}"
            s = Solver(long_spec(N1, False, K, check_every), backend="hip", device=0, keep_prev=keep_prev,
                       **SCHEDULES[sched])
            if start == "random":
                s.set_initial(*lcg_fields(N1))
            for run in ("first", "replay"):
                _log_equal(s.run(), want, (what, run))
                assert torch.equal(s.owned_field(0), uK), (what, run)
                assert torch.equal(s.owned_field(1), uK1), (what, run)
            assert s.native.graph_enabled
            h = s.field_hash(0), s.field_hash(1)
            for r in s.run_batch(3):
                _log_equal(r, want, (what, "batch"))
            assert (s.field_hash(0), s.field_hash(1)) == h, what
            assert torch.equal(s.owned_field(1), uK1), what


# ---- one rank, the long shot -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_shot(box):
    shot = long_shot(N1, box)
    c = Solver(long_spec(N1, box), backend="cpu")
    c.set_initial(np.zeros((N1 + 1,) * 3))
    c.set_sources(shot.sources, shot.w)
    c.set_receivers(shot.receivers)
    c.run()
    return c.global_field(0).numpy().copy(), c.global_field(1).numpy().copy(), c.traces().numpy().copy()


def _armed(s, box):
    shot = long_shot(N1, box)
    s.set_initial(np.zeros((N1 + 1,) * 3))
    s.set_sources(shot.sources, shot.w)
    s.set_receivers(shot.receivers)
    return s


def _three(s):
    return s.global_field(0).numpy().copy(), s.global_field(1).numpy().copy(), s.traces().numpy().copy()


def _close(got, box, what):
    tol = tolerance_long(box)
    for g, w, name in zip(got, _cpu_shot(box), ("u^K", "u^{K-1}", "traces")):
        assert g.shape == w.shape and not np.isnan(g).any(), (what, name)
        d = float(np.abs(g - w).max())
        print(f"LONGSOLVE {what} {name}: max |gpu - cpu| = {d:.3e} (tolerance {tol:.3e})")
        assert d <= tol, (what, name, d, tol)
    far = got[2][:, long_shot(N1, box).far]
    arrival = long_shot(N1, box).arrival
    assert not far[:arrival].any() and far[arrival] != 0.0, what  # (the cone adds exact zeros outside its ball)


@pytest.mark.parametrize("box", [False, True], ids=["cube", "box"])
def test_shot_single_steps_bit_identical(gpu, box):
    """temporal = 1: every unit is the CPU definition itself, 203 rows of traces and 203 addend rows. Catches an addend
    row or a trace row indexed by the unit instead of the step once the two differ by more than the short tests reach."""
    s = _armed(Solver(long_spec(N1, box), backend="hip", device=0, temporal=1), box)
    assert s.native.mode == "single-step"
    for run in range(2):
        s.run()
        for got, want in zip(_three(s), _cpu_shot(box)):
            assert same_bits(got, want), run


FUSED = {"p2_2": dict(temporal=2), "p2_3": dict(temporal=3), "p2_4": dict(temporal=4), "p2_5": dict(temporal=5),
         "tb4": dict(temporal=4, tiling_tb={"p2": False}), "lf2": dict(tb=False)}


@pytest.mark.parametrize("box", [False, True], ids=["cube", "box"])
@pytest.mark.parametrize("sched", list(FUSED))
def test_shot_fused_one_rank(gpu, sched, box):
    """Fused passes with k_source_cone and k_record_cone over 203 steps against CpuSolver within tolerance_long (the
    figures are the native CPU program's for this very shot: d_split 5.8e-16 / 6.5e-16, umax 9.98 / 8.58, so the
    tolerance is 16 eps umax = 3.5e-14 / 3.1e-14); the replay and a batch of three repeat the first run's bits. Catches a
    source correction or a cone record that uses the unit's index for the step, the addend array read past row K - 1 by
    the last unit, a trace row of the last, shorter unit written at the wrong step."""
    s = _armed(Solver(long_spec(N1, box), backend="hip", device=0, **FUSED[sched]), box)
    assert s.native.mode == "fused-single"
    s.run()
    first = _three(s)
    _close(first, box, f"{sched} box={box}")
    s.run()
    assert all(same_bits(a, b) for a, b in zip(_three(s), first))
    assert s.native.graph_enabled
    rs = s.run_batch(3)
    assert [r.extra["batched"] for r in rs] == [True] * 3
    assert all(same_bits(a, b) for a, b in zip(_three(s), first))


def test_reciprocity_on_the_gpu(gpu):
    """Source at A recorded at B against source at B recorded at A (box, zero start, temporal = 5), within
    long_reference.bound(K, umax): two GPU solves and no reference. Catches a cone correction or a cone record whose
    clipping at a wall (A is two nodes from three walls) differs from the pass's own."""
    A, B = reciprocity_pair(N1)
    w = long_shot(N1, True).w[:, :1]
    tr = []
    for src, rec in ((A, np.concatenate([B, A])), (B, np.concatenate([A, B]))):
        s = Solver(long_spec(N1, True), backend="hip", device=0, temporal=5)
        s.set_initial(np.zeros((N1 + 1,) * 3))
        s.set_sources(src, w)
        s.set_receivers(rec)
        s.run()
        tr.append(s.traces().numpy().copy())
    umax = max(float(np.abs(t).max()) for t in tr)
    d = float(np.abs(tr[0][:, 0] - tr[1][:, 0]).max())
    print(f"LONGSOLVE gpu reciprocity: max deviation {d:.3e} bound {bound(K, umax):.3e}")
    assert np.abs(tr[0][:, 0]).max() > 1e-3 * umax and d <= bound(K, umax)


def test_energy_after_the_long_solve(gpu):
    """k_energy after 203 steps of seeded random data: equal to the CPU value under the rule of
    tests/test_gpu_initial.py ((D + 8) 2^-53 sum |terms|), and E(K-1/2) = E(1/2) to a relative K 64 eps
    (tests/test_long_solves_cpu.py has the derivation)."""
    from mpi_cuda_amd._native import load

    C = load()
    spec = long_spec(N1, False)
    c = Solver(spec, backend="cpu")
    c.set_initial(*lcg_fields(N1))
    c.run()
    s = Solver(spec, backend="hip", device=0)
    s.set_initial(*lcg_fields(N1))
    s.run()
    e1, eK = s.energy(1), s.energy(0)
    ce = C.cpu_energy(spec.native(), s.native.layout, s.native.download(1), s.native.download(0))
    tol = (C.gpu_energy_depth(s.native.layout) + 8) * 2.0 ** -53 * ce["abs_terms"]
    print(f"LONGSOLVE gpu energy: E(1/2) {e1!r} E(K-1/2) {eK!r} cpu {c.energy(1)!r} {c.energy(0)!r} tol {tol:.3e}")
    assert ce["E"] == c.energy(0)  # (bit-identical fields)
    assert abs(eK - c.energy(0)) <= tol and abs(e1 - c.energy(1)) <= tol
    assert abs(eK - e1) / e1 <= K * 64 * EPS


# ---- groups on one GPU -------------------------------------------------------------------------------------------------
N0 = 2
LAYOUTS = {"s2": ("slab", 2, 66), "s4": ("slab", 4, 66), "c8": ("2x2x2", 8, 40), "b6": ("1x2x3", 6, 66)}


@functools.lru_cache(maxsize=None)
def _loaded(N, K_):
    """A random loaded state (u^1, u^2: zero on the walls) and CpuSolver's continuation to K_ with every step checked and
    receivers on both sides of the rank faces of every layout used at this N."""
    rng = np.random.default_rng(4000 + N)
    prev, cur = np.zeros((N + 1,) * 3), np.zeros((N + 1,) * 3)
    prev[1:N, 1:N, 1:N] = rng.standard_normal((N - 1,) * 3)
    cur[1:N, 1:N, 1:N] = rng.standard_normal((N - 1,) * 3)
    h, q = N // 2, N // 4
    rec = np.array([[h, h, h], [h - 1, h, h], [h, h - 1, h + 1], [q, h, 3], [q + 1, 2, h], [3 * q, N - 1, q], [1, 1, 1],
                    [N - 1, N - 1, N - 1], [0, h, h], [h, (2 * N) // 3, N // 3], [h, (2 * N) // 3 - 1, N // 3 - 1],
                    [N - 2, h, (2 * N) // 3]], dtype=np.int64)
    c = Solver(long_spec(N, False, K_), backend="cpu")
    c.set_state(prev, cur, N0)
    c.set_receivers(rec)
    r = c.run()
    return dict(prev=prev, cur=cur, rec=rec, log=r, uK=c.global_field(0), uK1=c.global_field(1),
                traces=c.traces().numpy().copy())


def _group_case(key, transport, S, overlap):
    return pytest.param(key, transport, S, overlap, id=f"{key}-{transport}-S{S}-{'ov' if overlap else 'seq'}")


GROUP_CASES = [
    _group_case("s2", "loopback", 5, True), _group_case("s2", "sdma", 5, False), _group_case("s2", "push", 2, True),
    _group_case("s2", "rccl-self", 2, False),
    _group_case("s4", "loopback", 2, False), _group_case("s4", "sdma", 2, True), _group_case("s4", "push", 5, False),
    _group_case("s4", "rccl-self", 5, True),
    _group_case("c8", "loopback", 5, True), _group_case("c8", "rccl-self", 5, False), _group_case("c8", "sdma", 2, True),
    _group_case("c8", "sdma", 5, False), _group_case("c8", "loopback", 2, False),
    _group_case("b6", "loopback", 2, True), _group_case("b6", "sdma", 5, True), _group_case("b6", "rccl-self", 5, False),
]


@pytest.mark.parametrize("key,transport,S,overlap", GROUP_CASES)
def test_groups_long(gpu, key, transport, S, overlap):
    """A group from the random loaded state to K = 203 (depth 2: K = 204 — ranks run passes of two steps and more, so
    passes of exactly 2 refuse the odd 201 steps left, and that refusal stays), three solves in a row: error log (maxima exact, sums 1e-12),
    u^K, u^{K-1} and the traces equal the undecomposed CpuSolver's, which the one-rank solves of every schedule equal
    too. Catches a copy-engine flag value reused across units or across the two parities (the third solve runs the first
    one's parity again: a wait satisfied by a stale word lets a pass read ghosts of an earlier exchange), a staging parity
    or epoch that drifts after tens of exchanges, a partial region of one rank's shells overwritten after a wrap, an
    error-log or trace row at the wrong step index on a rank whose units differ from rank 0's."""
    decomp, world, N = LAYOUTS[key]
    K_ = K + 1 if S == 2 else K
    G = _loaded(N, K_)
    slab = key.startswith("s")
    kw = dict(tb_min_planes=8) if slab else {}
    g = Solver(long_spec(N, False, K_), backend="hip", transport=transport, world=world, rank=0, decomp=decomp, device=0,
               temporal=S, overlap=overlap, poison_ghosts=slab or transport != "rccl-self", **kw)
    assert g.native.mode() == ("deep-tb" if slab else "deep-tb-block") and g.native.transport == transport
    assert g.native.temporal() == (4 if S == 5 and transport == "push" else S)
    assert g.native.overlapped() == overlap
    g.set_state(G["prev"], G["cur"], N0)
    if transport != "push":  # (the push transport takes no receivers)
        g.set_receivers(G["rec"])
    assert G["log"].steps == list(range(N0 + 1, K_ + 1))
    for run in range(3):
        _log_equal(g.run(), G["log"], (key, transport, run))
        assert torch.equal(g.global_field(0), G["uK"]), run
        assert torch.equal(g.global_field(1), G["uK1"]), run
        if transport != "push":
            assert same_bits(g.traces().numpy()[N0 - 1:], G["traces"][N0 - 1:]), run


_shot_bits = {}


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "seq"])
@pytest.mark.parametrize("transport", ["loopback", "rccl-self"])
@pytest.mark.parametrize("group", ["slab4tb", "block8"])
def test_groups_long_shot(gpu, group, transport, overlap):
    """The long shot on 4 slabs and on 2x2x2 blocks at N = 40: the sources sit on both sides of the rank faces at 20, so
    every unit's correction touches ghost planes of two to eight ranks, 41 exchanges in a row, and the wavefront crosses
    every rank face twice. Within tolerance_long of CpuSolver; the same bits on both transports, with either exchange
    order and on the second solve. Catches a source correction missing on (or applied twice to) a ghost plane after many
    exchanges: an error of the size of the addend, 1e13 tolerances, that poisoned ghosts turn into NaN."""
    world, decomp, kw = {"slab4tb": (4, "slab", dict(tb_min_planes=8)), "block8": (8, "2x2x2", {})}[group]
    g = Solver(long_spec(N1, False), backend="hip", transport=transport, world=world, rank=0, decomp=decomp, device=0,
               overlap=overlap, poison_ghosts=True, **kw)
    _armed(g, False)
    assert g.native.mode() == {"slab4tb": "deep-tb", "block8": "deep-tb-block"}[group]
    what = f"{group} {transport} overlap={overlap}"
    g.run()
    first = _three(g)
    _close(first, False, what)
    g.run()
    assert all(same_bits(a, b) for a, b in zip(_three(g), first)), what
    ref = _shot_bits.setdefault(group, first)
    assert all(same_bits(a, b) for a, b in zip(first, ref)), what
