"""k_energy and k_energy_reduce at kernel level (gpu_energy / gpu_energy_reduce): random fields with nonzero global
boundary nodes and NaN-poisoned ghosts, one-rank and rank layouts, cube and box, against the plain numpy reference of
tests/energy_reference.py. tests/test_energy_cpu.py runs the same reference against cpu_energy and checks, on the
reference alone, that a missing mask or one dropped edge moves the potential sum by more than 100 tolerances.

What a solve cannot show and these inputs do: after a solve the boundary nodes and the ghosts outside the grid hold
zeros, so an edge leaving the grid is 0·0 with or without its mask. Here the boundary is random and every ghost outside
the grid (and deeper than one layer, and the row padding) is NaN: a mask that lets such an edge through gives NaN, one
off by one the other way drops a term of typical size, and the box's three distinct 1/h² expose an axis mix-up.

Tolerances (derived, none measured; u = 2⁻⁵³, Σ|t| exactly rounded sums of the reference's own terms):
  * a summation tree of depth D over terms t is off by at most D·u·Σ|t| to first order; with the project's slack of 8:
      |kin − kin*| <= (D + 8)·u·A_k,  A_k = Σ|tk|;   |pot − pot*| <= (D + 8)·u·A_p,  A_p = Σ(|tx| + |ty| + |tz|),
    D = gpu_energy_depth(layout) = 1 + 8 + 6 + 3 + ceil(B / 1024) + 6 + 15. Each sum has its own bound.
  * one workgroup's partial: depth 1 + 8 + 6 + 3 (a pair's two nodes, 8 planes, 6 butterfly levels, 4 waves), so
    (1 + 8 + 6 + 3 + 8)·u·Σ|t| over the nodes of that workgroup: planes [8·by, 8·by + 8), flattened (row, pair) indices
    [256·bx, 256·bx + 256), pairs counted from kp0 = (zg + zs) // 2 (energy_reference.workgroup_map).
  * k_energy_reduce alone on n values x: (ceil(n / 1024) + 6 + 15 + 8)·u·Σ|x|.
  * additivity over the 8 ranks of 67, 2x2x2: the sum of the ranks' own tolerances.

Column alignment: zg + zs is odd on every layout that starts at global z = 0 — all one-rank layouts, c0 (rank 0 of
2x2x2) and s1 (rank 1 of 3x1x1): the row's first pair holds a ghost and the first owned node — and even on r13, c7 and
b4: the first pair holds two owned nodes. test_rank_layouts_cover_both_alignments asserts it.

Many partials: N = 160 is the smallest one-rank N whose layout has more than 1024 partials (21 x 51 = 1071; N = 159
has 1020), so k_energy_reduce's loop makes a second trip and ceil(B / 1024) = 2 enters D.
"""
import functools
import math

import numpy as np
import pytest
import torch

import energy_reference as er
from energy_reference import U

pytestmark = pytest.mark.gpu

ONE_RANK = [(N, box) for N in (40, 77, 130) for box in (False, True)]
RANK_CASES = [(k, box) for k in er.RANKS for box in (False, True)]
SLOTS_AFTER = 8  # NaN slots behind the partials: nothing may be written there
_ID = lambda v: {False: "cube", True: "box"}.get(v, str(v))  # noqa: E731


def _C():
    from mpi_cuda_amd._native import load

    return load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(case, B):
    """One gpu_energy call on fresh NaN-filled buffers: (out, partials with the SLOTS_AFTER slots behind them)."""
    a, b = torch.from_numpy(case.a).cuda(), torch.from_numpy(case.b).cuda()
    part = torch.full((B + SLOTS_AFTER, 2), float("nan"), dtype=torch.float64, device="cuda")
    out = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    _C().gpu_energy(case.lay, case.co, case.tau, a.data_ptr(), b.data_ptr(), part.data_ptr(), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), part.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _run(N, dims, rank, S, box, workgroups=True):
    """The reference and two kernel runs of one case, computed once and shared by the tests below (the fields
    themselves are not kept)."""
    C = _C()
    case = er.Case(C, N, dims, rank, S, box)
    t = er.terms(case)
    kin, pot, Ak, Ap = er.sums(t)
    B = C.gpu_energy_partials(case.lay)
    r = dict(what=case.what(), zc=case.zc, B=B, D=C.gpu_energy_depth(case.lay), kin=kin, pot=pot, Ak=Ak, Ap=Ap)
    assert r["D"] == 1 + 8 + 6 + 3 + math.ceil(B / 1024) + 6 + 15
    if workgroups:
        r["wg"], nb = er.workgroup_sums(case, t)
        assert nb == B  # exactly gpu_energy_partials(layout) partials
    r["out"], r["part"] = _launch(case, B)
    r["out2"], r["part2"] = _launch(case, B)
    return r


def _assert_sums(r):
    tol_k, tol_p = (r["D"] + 8) * U * r["Ak"], (r["D"] + 8) * U * r["Ap"]
    k, p = float(r["out"][0]), float(r["out"][1])
    print(f"{r['what']}: B={r['B']} D={r['D']} kin {k!r} ref {r['kin']!r} diff {k - r['kin']:.3e} tol {tol_k:.3e}; "
          f"pot {p!r} ref {r['pot']!r} diff {p - r['pot']:.3e} tol {tol_p:.3e}")
    assert math.isfinite(k) and math.isfinite(p), r["what"]
    assert abs(k - r["kin"]) <= tol_k, r["what"]
    assert abs(p - r["pot"]) <= tol_p, r["what"]
    # a second launch: identical bits, in the sums and in every partial
    assert np.array_equal(r["out"].view(np.int64), r["out2"].view(np.int64))
    assert np.array_equal(r["part"].view(np.int64), r["part2"].view(np.int64))
    return k, p, tol_k, tol_p


def _assert_partials(r):
    B, part = r["B"], r["part"]
    assert part.shape == (B + SLOTS_AFTER, 2)
    assert np.isnan(part[B:]).all(), "a partial written beyond gpu_energy_partials(layout)"
    unwritten = np.argwhere(~np.isfinite(part[:B]))
    assert unwritten.size == 0, (r["what"], "unwritten or non-finite partials", unwritten[:5].tolist())
    kin, pot, Ak, Ap = r["wg"]
    c = (er.WG_DEPTH + 8) * U
    for name, got, ref, A in (("kin", part[:B, 0], kin, Ak), ("pot", part[:B, 1], pot, Ap)):
        bad = np.argwhere(np.abs(got - ref) > c * A).reshape(-1)
        worst = float(np.max(np.abs(got - ref) / np.where(A > 0, c * A, 1.0)))
        print(f"{r['what']}: {name} partials: largest |diff| / tol = {worst:.3f} over {B}")
        assert bad.size == 0, (r["what"], name, len(bad), [(int(i), got[i], ref[i]) for i in bad[:5]])


@pytest.mark.parametrize("N,box", ONE_RANK, ids=_ID)
def test_one_rank_sums(gpu, N, box):
    """kin and pot of the whole grid as one rank (all four global-boundary masks at work: every ghost is NaN), each
    against its own bound; two launches give the same bits."""
    _assert_sums(_run(N, (1, 1, 1), 0, 1, box))


@pytest.mark.parametrize("N,box", ONE_RANK, ids=_ID)
def test_one_rank_partials(gpu, N, box):
    """Every workgroup's partial against the reference sum over its own planes and (row, pair) range: pins the
    thread -> node map, so errors of two workgroups cannot cancel; no slot unwritten, none written beyond B."""
    _assert_partials(_run(N, (1, 1, 1), 0, 1, box))


@pytest.mark.parametrize("key,box", RANK_CASES, ids=_ID)
def test_rank_layout_sums(gpu, key, box):
    """gx0 / gy0 / gz0 != 0, ghosts 5 deep in (x0 + xg)·plane, pairs straddling the first / last owned column, edges
    into a neighbour's ghost (real values one layer deep, NaN below)."""
    N, dims, rank = er.RANKS[key]
    _assert_sums(_run(N, dims, rank, er.RANK_S, box))


@pytest.mark.parametrize("key,box", RANK_CASES, ids=_ID)
def test_rank_layout_partials(gpu, key, box):
    N, dims, rank = er.RANKS[key]
    _assert_partials(_run(N, dims, rank, er.RANK_S, box))


def test_rank_layouts_cover_both_alignments(gpu):
    """zg + zs odd (the first pair of a row holds a ghost and an owned node) and even (two owned nodes) both occur."""
    zc = {k: _run(*er.RANKS[k], er.RANK_S, False)["zc"] % 2 for k in er.RANKS}
    assert zc == {"r13": 0, "c0": 1, "c7": 0, "b4": 0, "s1": 1}
    assert all(_run(N, (1, 1, 1), 0, 1, False)["zc"] % 2 == 1 for N in (40, 77, 130))


@pytest.mark.parametrize("box", [False, True], ids=_ID)
def test_additivity_over_ranks(gpu, box):
    """The 8 ranks of 67, 2x2x2: the fsum of the per-rank GPU sums equals the one-rank reference of the whole grid
    within the sum of the ranks' tolerances — every grid edge is counted exactly once across ranks."""
    N, dims = 67, (2, 2, 2)
    whole = er.Case(_C(), N, box=box)
    kin, pot, _, _ = er.sums(er.terms(whole))
    # (ranks 0 and 7 are c0 and c7 above: the same cached runs)
    parts = [_assert_sums(_run(N, dims, r, er.RANK_S, box) if r in (0, 7) else _run(N, dims, r, er.RANK_S, box, False))
             for r in range(8)]
    k, p = math.fsum(x[0] for x in parts), math.fsum(x[1] for x in parts)
    tol_k, tol_p = sum(x[2] for x in parts), sum(x[3] for x in parts)
    print(f"N={N} {dims} box={box}: kin {k!r} ref {kin!r} tol {tol_k:.3e}; pot {p!r} ref {pot!r} tol {tol_p:.3e}")
    assert abs(k - kin) <= tol_k
    assert abs(p - pot) <= tol_p


def test_many_partials(gpu):
    """More than 1024 partials: k_energy_reduce's `i += 1024` loop makes a second trip and energy_depth's
    ceil(B / 1024) term is 2. The smallest such one-rank N, on the box."""
    C = _C()

    def partials(N):
        p = er.make_spec(N, True).native()
        return C.gpu_energy_partials(C.make_layout(p, C.rank_box(p, C.Dims(1, 1, 1), 0)))

    N = min(n for n in range(131, 200) if partials(n) > 1024)
    assert N == 160 and partials(N) == 1071 > 1024
    r = _run(N, (1, 1, 1), 0, 1, True, False)
    assert r["B"] == 1071 and r["D"] == 41
    _assert_sums(r)
    assert np.isfinite(r["part"][:r["B"]]).all() and np.isnan(r["part"][r["B"]:]).all()


@pytest.mark.parametrize("kind", ["positive", "mixed"])
@pytest.mark.parametrize("n", [1, 63, 64, 1023, 1024, 1025, 3000, 32704])
def test_energy_reduce_alone(gpu, n, kind):
    """k_energy_reduce on n random partials at the front of a larger NaN-filled buffer (a read past n shows as NaN),
    both components against math.fsum; two launches give the same bits. 32704 = the partials of the 512³ grid."""
    rng = np.random.default_rng(n * 2 + (kind == "mixed"))
    if kind == "positive":
        x = rng.random((n, 2)) * np.array([1e12, 1e8]) + 1.0
    else:
        x = rng.standard_normal((n, 2)) * 10.0 ** rng.uniform(-3, 3, (n, 2))
    buf = torch.full((n + 1024 + 64, 2), float("nan"), dtype=torch.float64)
    buf[:n] = torch.from_numpy(x)
    dev = buf.cuda()
    outs = []
    for _ in range(2):
        out = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
        _C().gpu_energy_reduce(dev.data_ptr(), n, out.data_ptr(), _stream())
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64))
    depth = math.ceil(n / 1024) + 6 + 15
    for c in (0, 1):
        ref, A = math.fsum(x[:, c].tolist()), math.fsum(np.abs(x[:, c]).tolist())
        tol = (depth + 8) * U * A
        got = float(outs[0][c])
        print(f"n={n} {kind} [{c}]: {got!r} ref {ref!r} diff {got - ref:.3e} tol {tol:.3e}")
        assert math.isfinite(got) and abs(got - ref) <= tol
