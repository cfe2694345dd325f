"""cpu_energy on rank layouts with random, NaN-poisoned inputs against the plain numpy reference of
tests/energy_reference.py (its docstring has the inputs, the terms and how the tolerances are derived), the reference's
own sensitivity to a missing mask or a dropped edge, and the launch geometry the GPU tests rely on.

Tolerances: |kin − kin*| <= (D + 8)·u·A_k and |pot − pot*| <= (D + 8)·u·A_p, each sum on its own; D = cpu_energy's own
depth (nz + ny + nx, its three nested accumulators), A_k / A_p from the reference.
"""
import math

import pytest

import energy_reference as er
from energy_reference import U
from mpi_cuda_amd._native import load

# (160 on the box: the GPU tests' many-partials case, here for its sensitivity check)
ONE_RANK = [(N, box) for N in (40, 77, 130) for box in (False, True)] + [(160, True)]
RANK_CASES = [(k, box) for k in er.RANKS for box in (False, True)]
_ID = lambda v: {False: "cube", True: "box"}.get(v, str(v))  # noqa: E731


def _check(C, case, with_sensitivity=True):
    t = er.terms(case)
    kin, pot, Ak, Ap = er.sums(t)
    assert math.isfinite(kin) and math.isfinite(pot) and kin > 0 and Ak == kin and Ap > abs(pot)
    e = C.cpu_energy(case.prob, case.lay, case.a, case.b)
    D = int(e["depth"])
    assert D == sum(case.n)
    tol_k, tol_p = (D + 8) * U * Ak, (D + 8) * U * Ap
    print(f"{case.what()}: D={D} kin {e['kin']!r} ref {kin!r} diff {e['kin'] - kin:.3e} tol {tol_k:.3e}; "
          f"pot {e['pot']!r} ref {pot!r} diff {e['pot'] - pot:.3e} tol {tol_p:.3e}")
    assert math.isfinite(e["kin"]) and math.isfinite(e["pot"])
    assert abs(e["kin"] - kin) <= tol_k
    assert abs(e["pot"] - pot) <= tol_p
    if with_sensitivity:
        # against the wider of the CPU and the GPU tolerance of this layout, so it holds for both
        er.check_sensitivity(case, t, pot, (max(D, C.gpu_energy_depth(case.lay)) + 8) * U * Ap)
    return e["kin"], e["pot"], tol_k, tol_p


@pytest.mark.parametrize("N,box", ONE_RANK, ids=_ID)
def test_cpu_energy_one_rank_random_nonzero_boundary(N, box):
    """The whole grid as one rank: every ghost lies outside the grid and holds NaN, the boundary nodes are nonzero, so
    the three masks alone keep the result finite and right."""
    _check(load(), er.Case(load(), N, box=box))


@pytest.mark.parametrize("key,box", RANK_CASES, ids=_ID)
def test_cpu_energy_rank_layouts(key, box):
    """gx0 / gy0 / gz0 != 0, ghosts up to 5 deep (NaN below the first layer), edges into a neighbour's ghost."""
    N, dims, rank = er.RANKS[key]
    _check(load(), er.Case(load(), N, dims, rank, er.RANK_S, box))


@pytest.mark.parametrize("box", [False, True], ids=_ID)
def test_cpu_energy_is_additive_over_ranks(box):
    """The 8 ranks of 67, 2x2x2: the sum of the per-rank sums equals the one-rank reference of the whole grid within
    the sum of the ranks' tolerances, so every grid edge is counted exactly once across ranks."""
    C = load()
    N, dims = 67, (2, 2, 2)
    whole = er.Case(C, N, box=box)
    kin, pot, _, _ = er.sums(er.terms(whole))
    parts = [_check(C, er.Case(C, N, dims, r, er.RANK_S, box), with_sensitivity=False) for r in range(8)]
    assert abs(math.fsum(p[0] for p in parts) - kin) <= sum(p[2] for p in parts)
    assert abs(math.fsum(p[1] for p in parts) - pot) <= sum(p[3] for p in parts)


def test_column_alignments_and_launch_geometry():
    """Both alignments of the first owned column occur among the layouts (zg + zs odd: the row's first pair holds a
    ghost and an owned node; even: two owned nodes), the reference's workgroup map has gpu_energy_partials(layout)
    entries on every layout, and 160 is the smallest one-rank N with more than 1024 partials."""
    C = load()
    parity = {}
    for key, (N, dims, rank) in er.RANKS.items():
        lay = er.rank_layout(C, er.make_spec(N).native(), dims, rank, er.RANK_S)
        zc = int(lay.zg + lay.zs)
        parity[key] = zc % 2
        assert er.workgroup_map((int(lay.nx), int(lay.ny), int(lay.nz)), zc)[1] == C.gpu_energy_partials(lay), key
    assert parity == {"r13": 0, "c0": 1, "c7": 0, "b4": 0, "s1": 1}

    def partials(N):
        p = er.make_spec(N).native()
        return C.gpu_energy_partials(C.make_layout(p, C.rank_box(p, C.Dims(1, 1, 1), 0)))

    assert min(N for N in range(130, 200) if partials(N) > 1024) == 160 and partials(160) == 1071
