"""k_sponge_box at kernel level: launch_sponge_box on NaN-poisoned one-rank layouts with seeded random inputs.

N = 24 (cube) and N = 40 (box 1 x 1.3 x 0.7), steps = 2..5. The two input levels hold random values on the box grown by
`steps` (clipped to the interior) and NaN everywhere else — on and outside the global boundary, in the row padding, and on
every interior node the contract says is not read; the outputs hold a sentinel. Boxes: a corner where three layers
meet (odd extents, a partial tile on every axis), a single face's slab, a slab merged over the whole x range, and the
boxes sponge_boxes returns for all six faces. After the launch the outputs on the box equal `steps` damped cpu_leapfrog
steps bit for bit, every other element of both output buffers keeps its sentinel (margins around the allocations
included), and the inputs keep their bits."""
import functools

import numpy as np
import pytest
import torch

from sources_common import BOX, same_bits

pytestmark = pytest.mark.gpu

MARGIN = 4096
SENTINEL = -1234.5
CONFIGS = {"N24-cube": (24, False, 6), "N40-box": (40, True, 8)}


def _C():
    from mpi_cuda_amd._native import load

    return load()


class Case:
    def __init__(self, key):
        C = _C()
        self.N, box, self.W = CONFIGS[key]
        N = self.N
        sp = C.Sponge(self.W, 0.0, 63)
        self.prob = (C.Problem(N, 0.9 / (N * 3.2), 9, BOX[0], Ly=BOX[1], Lz=BOX[2], sponge=sp) if box
                     else C.Problem(N, 0.9 / (N * 1.8), 9, 1.0, sponge=sp))
        assert self.prob.cfl_ok
        self.co = C.Coeffs.from_problem(self.prob)
        self.lay = l = C.make_layout(self.prob, C.rank_box(self.prob, C.Dims(1, 1, 1), 0))
        self.s_ext = C.sin_table_ext(self.prob)
        self.tables = torch.from_numpy(C.sponge_tables(self.prob).copy()).cuda()
        rng = np.random.default_rng(1000 + N)
        i = np.arange(1, N)
        self.off = (int(l.off(0, 0, 0)) + i[:, None, None] * int(l.plane) + i[None, :, None] * int(l.pitch)
                    + i[None, None, :])  # offsets of the interior nodes 1..N-1
        self.clean = []
        for _ in range(2):
            f = np.zeros(int(l.total))
            f[self.off] = rng.standard_normal(self.off.shape)
            self.clean.append(f)

    @functools.lru_cache(maxsize=None)
    def levels(self, steps):
        """(u^{n+steps-1}, u^{n+steps}) of `steps` damped CPU steps from the clean inputs over the whole interior."""
        C = _C()
        old, cur = self.clean[0].copy(), self.clean[1].copy()
        for _ in range(steps):
            C.cpu_leapfrog(self.lay, self.co, cur, old, C.compute_box(self.lay), self.s_ext, sponge=self.prob)
            old, cur = cur, old
        return old, cur

    def boxes(self, kind, steps):
        C, N, W = _C(), self.N, self.W
        if kind == "corner":
            return [C.LBox(1, W + steps, 1, W + steps - 1, 1, W + steps + 2)]
        if kind == "face":  # the y+ slab, its x range cut as sponge_boxes cuts it
            return [C.LBox(W + steps - 1, N - (W + steps - 1) + 1, N - (W + steps - 1) + 1, N, 1, N)]
        if kind == "merged":  # a z slab over the whole x range (opposite x slabs merged into one interval)
            return [C.LBox(1, N, 3, N - 2, N - 7, N)]
        return C.sponge_boxes(self.prob, self.lay, steps)


@functools.lru_cache(maxsize=None)
def _case(key):
    return Case(key)


def _guarded(f):
    buf = torch.full((len(f) + 2 * MARGIN,), float("nan"), dtype=torch.float64)
    buf[MARGIN:-MARGIN] = torch.from_numpy(f)
    return buf.cuda()


@pytest.mark.parametrize("kind", ["corner", "face", "merged", "all6"])
@pytest.mark.parametrize("steps", [2, 3, 4, 5])
@pytest.mark.parametrize("key", list(CONFIGS))
def test_sponge_box_bitexact(key, steps, kind):
    C, c = _C(), _case(key)
    N, l = c.N, c.lay
    boxes = c.boxes(kind, steps)
    assert boxes and all(not b.empty() for b in boxes)
    # what may be read: the boxes grown by `steps`, clipped to the interior
    readable = np.zeros((N - 1,) * 3, dtype=bool)
    written = np.zeros((N - 1,) * 3, dtype=bool)
    for b in boxes:
        r = [(max(lo - steps, 1), min(hi + steps, N)) for lo, hi in ((b.x0, b.x1), (b.y0, b.y1), (b.z0, b.z1))]
        readable[r[0][0] - 1:r[0][1] - 1, r[1][0] - 1:r[1][1] - 1, r[2][0] - 1:r[2][1] - 1] = True
        sl = (slice(b.x0 - 1, b.x1 - 1), slice(b.y0 - 1, b.y1 - 1), slice(b.z0 - 1, b.z1 - 1))
        assert not written[sl].any()  # (disjoint)
        written[sl] = True
    if kind == "all6":  # exactly the slabs d < W + steps - 1
        d = np.minimum(np.arange(1, N), N - np.arange(1, N))
        near = d < c.W + steps - 1
        assert np.array_equal(written, near[:, None, None] | near[None, :, None] | near[None, None, :])
    ins = []
    for f in c.clean:
        p = np.full(int(l.total), np.nan)
        p[c.off[readable]] = f[c.off[readable]]
        ins.append(p)
    prev, cur = _guarded(ins[0]), _guarded(ins[1])
    out1 = torch.full((int(l.total) + 2 * MARGIN,), SENTINEL, dtype=torch.float64).cuda()
    out2 = out1.clone()
    st = torch.cuda.current_stream().cuda_stream
    e = 8 * MARGIN
    for b in boxes:
        C.gpu_sponge_box(l, c.co, c.tables.data_ptr(), prev.data_ptr() + e, cur.data_ptr() + e, out1.data_ptr() + e,
                         out2.data_ptr() + e, b, steps, st)
    torch.cuda.synchronize()
    want1, want2 = c.levels(steps)
    for got, want in ((out1, want1), (out2, want2)):
        exp = np.full(int(l.total) + 2 * MARGIN, SENTINEL)
        exp[MARGIN + c.off[written]] = want[c.off[written]]
        assert same_bits(got.cpu().numpy(), exp)
    for buf, p in ((prev, ins[0]), (cur, ins[1])):
        exp = np.full(int(l.total) + 2 * MARGIN, np.nan)
        exp[MARGIN:-MARGIN] = p
        assert same_bits(buf.cpu().numpy(), exp)
    assert np.isfinite(want2[c.off[written]]).all() and np.isfinite(want1[c.off[written]]).all()
