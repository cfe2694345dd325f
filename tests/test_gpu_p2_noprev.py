"""The pair-tiled pass without its u^{n+S-1} store (out1 = null: a solve's last pass, UnitPlan::drop_prev), at kernel
level through gpu_leapfrog_p2_boxes: two launches from identical inputs, one with out1 set and one with out1 = 0.
u^{n+S} and every partial must agree bit for bit, and a buffer standing in for the absent out1 must keep every byte.
S = 2..5 load passes and the S = 2..4 analytic starts, N = 40 and 77 (partial tiles, odd pair boundaries), unchunked
and x-chunked, the last two levels checked or none, the cube and a rectangular box."""
import math

import pytest
import torch

from mpi_cuda_amd.ops import stencil as ops

pytestmark = pytest.mark.gpu

PASSES = [(2, False), (3, False), (4, False), (5, False), (2, True), (3, True), (4, True)]  # (stages, analytic start)


def _problem(C, N, box):
    prob = C.Problem(N, 1e-3, 20, 1.0, Ly=1.25, Lz=0.8) if box else C.Problem(N, 1e-3, 20, 1.0)
    lay = C.make_layout(prob, C.rank_box(prob, C.parse_dims("slab", 1, N), 0))
    return prob, C.Coeffs.from_problem(prob), lay


def _rand_interior(lay, seed):  # (as tests/test_gpu_kernels.py: random interior, zero boundary and ghosts)
    torch.manual_seed(seed)
    g = torch.zeros((int(lay.nx) + 2, int(lay.ny) + 2, int(lay.nz) + 2), dtype=torch.float64)
    g[2:-2, 2:-2, 2:-2] = torch.randn(int(lay.nx) - 2, int(lay.ny) - 2, int(lay.nz) - 2, dtype=torch.float64)
    return ops.from_grid(lay, g)


def _pattern(n, salt):
    """n doubles, each with its own bit pattern (finite or not: they are only compared as bits)"""
    return (torch.arange(n, dtype=torch.int64) * 0x1E3779B97F4A7C15 % (1 << 62) + salt).view(torch.float64)


def _bits(t):
    return t.cpu().view(torch.int64)


def _tiling(C, stages, chunked):
    t = C.LeapfrogTbTiling()
    t.stages, t.p2, t.target_blocks = stages, True, 256 if chunked else 1
    return t


@pytest.mark.parametrize("N,box", [(40, False), (77, False), (77, True)])
@pytest.mark.parametrize("stages,analytic", PASSES)
@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("checked", [True, False])
def test_p2_without_prev_store(gpu, N, box, stages, analytic, chunked, checked):
    C = gpu
    prob, co, lay = _problem(C, N, box)
    cbox = C.compute_box(lay)
    assert C.gpu_leapfrog_p2_supported(lay, cbox, stages)
    t = _tiling(C, stages, chunked)
    grid = C.gpu_leapfrog_p2_partials(lay, cbox, t)
    if chunked:
        nblocks, per = C.p2_launch_blocks([cbox], t)
        assert per[0][3] > 1, "the x-chunked case must really be chunked"
    n0 = 1 if analytic else 5
    ct = [math.cos(prob.a_t * (n0 + k) * prob.tau) for k in range(1, stages + 1)]
    mask = (0b11 << (stages - 2)) if checked else 0
    s = ops.sin_table_ext(prob).cuda()
    total = int(lay.total)
    prev = cur = None
    if not analytic:
        prev, cur = _rand_interior(lay, N * 13 + stages).cuda(), _rand_interior(lay, N * 17 + stages).cuda()
        prev0, cur0 = prev.clone(), cur.clone()
    out = []
    stand_in0 = _pattern(total, 7)
    stand_in = stand_in0.cuda()  # what a pass that still stored the level somewhere would have to hit: never passed
    for with_prev in (True, False):
        o1 = _pattern(total, 1).cuda()
        o2 = _pattern(total, 2).cuda()
        part = torch.full((stages * grid, 2), float("nan"), dtype=torch.float64, device="cuda")
        C.gpu_leapfrog_p2_boxes(lay, co, prev.data_ptr() if prev is not None else 0,
                                cur.data_ptr() if cur is not None else 0, o1.data_ptr() if with_prev else 0,
                                o2.data_ptr(), [cbox], s.data_ptr(), ct, mask, part.data_ptr() if mask else 0, t,
                                ops._stream(), analytic_start=analytic, level_stride=grid, grid_blocks=grid)
        torch.cuda.synchronize()
        out.append((_bits(o1), _bits(o2), _bits(part)))
    (a1, a2, ap), (b1, b2, bp) = out
    assert torch.equal(a2, b2), "u^{n+S} differs between the launches with and without out1"
    assert torch.equal(ap, bp), "partials differ between the launches with and without out1"
    assert not torch.equal(a1, _bits(_pattern(total, 1))), "the reference launch stored no u^{n+S-1}"
    assert not torch.equal(a2, _bits(_pattern(total, 2))), "the launches stored no u^{n+S}"
    # out1 = 0: nothing stored for that level — the second launch's own out1 tensor was never passed, nor the stand-in
    assert torch.equal(b1, _bits(_pattern(total, 1)))
    assert torch.equal(_bits(stand_in), _bits(stand_in0)), "a byte of the buffer standing in for out1 changed"
    if checked:  # the checked levels' partials were written (no NaN left in their slots), the others were not touched
        pf = bp.view(torch.float64).reshape(stages, grid, 2)
        for k in range(1, stages + 1):
            assert bool(torch.isnan(pf[k - 1]).any()) == (not (mask >> (k - 1) & 1))
    if not analytic:
        assert torch.equal(_bits(prev), _bits(prev0)) and torch.equal(_bits(cur), _bits(cur0))


@pytest.mark.parametrize("analytic", [False, True])
def test_p2_null_out1_refuses_ghost_planes(gpu, analytic):
    """The launcher refuses out1 = null together with ghost_x1 (a host check, before anything is launched)."""
    C = gpu
    prob, co, lay = _problem(C, 40, False)
    cbox = C.compute_box(lay)
    stages = 4
    t = _tiling(C, stages, False)
    t.ghost_x1 = 1
    total = int(lay.total)
    bufs = [torch.zeros(total, dtype=torch.float64, device="cuda") for _ in range(3)]
    s = ops.sin_table_ext(prob).cuda()
    with pytest.raises(Exception, match="out1 = null"):
        C.gpu_leapfrog_p2_boxes(lay, co, bufs[0].data_ptr(), bufs[1].data_ptr(), 0, bufs[2].data_ptr(), [cbox],
                                s.data_ptr(), [0.5] * stages, 0, 0, t, ops._stream(), analytic_start=analytic)
    torch.cuda.synchronize()
    # ... and k_leapfrog_tb, which always stores both levels, refuses a null out1 altogether
    t2 = _tiling(C, stages, False)
    t2.p2 = False
    with pytest.raises(Exception, match="out1 = null"):
        C.gpu_leapfrog_tb(lay, co, bufs[0].data_ptr(), bufs[1].data_ptr(), 0, bufs[2].data_ptr(), cbox, s.data_ptr(),
                          [0.5] * stages, 0, 0, t2, ops._stream(), analytic_start=analytic)
    torch.cuda.synchronize()
