"""k_record_cone / k_record_gather at kernel level on rank layouts with random, poisoned inputs.

One rank of a decomposition (N = 77: one rank; slab 4x1x1 rank 1 with xg = 5; block 2x2x2 rank 3 with ghost depth 5 on
every axis; each as cube and as box 1 x 1.3 x 0.7) gets random global u^{n-1}, u^n cut to its ghosts. Every element a
pass of s steps may not read holds NaN: ghosts deeper than s (u^n) / s - 1 (u^{n-1}), every node on or outside the
global boundary, the row padding and the zero slot. For s = 2..5 the cone's rows must equal s native CPU single steps of
the undecomposed grid bit for bit at every owned receiver of the common set and every level, hold no NaN (a read beyond
the ball or the contract shows as one), and leave the slots of receivers not given to the launch, and every other row,
NaN. A wrong cone (cube instead of ball, a mirrored axis, a y/z ratio on the wrong axis, a boundary node computed) or a
read outside the allocation's valid part fails here."""
import functools

import numpy as np
import pytest
import torch

from receivers_common import receiver_set, same_bits

from mpi_cuda_amd.ops import stencil as ops

pytestmark = pytest.mark.gpu

N = 77
TAU_FRACTION = 0.5
EDGES = (1.0, 1.3, 0.7)
# name: (dims, rank, ghost depths)
LAYOUTS = {"one": ((1, 1, 1), 0, (1, 1, 1)), "slab": ((4, 1, 1), 1, (5, 1, 1)), "block": ((2, 2, 2), 3, (5, 5, 5))}
N0 = 3  # the inputs are u^{N0-1}, u^{N0}


def _C():
    from mpi_cuda_amd._native import load

    return load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _problem(box):
    C = _C()
    p0 = C.Problem(N, 1e-4, 20, EDGES[0], Ly=EDGES[1], Lz=EDGES[2]) if box else C.Problem(N, 1e-4, 20, 1.0)
    tau = TAU_FRACTION * p0.tau_max
    return C.Problem(N, tau, 20, EDGES[0], Ly=EDGES[1], Lz=EDGES[2]) if box else C.Problem(N, tau, 20, 1.0)


@functools.lru_cache(maxsize=None)
def _global(box):
    """Random global u^{n-1}, u^n (zero faces) and the five levels after them by native CPU single steps, as dense
    (N+1)^3 arrays: computed once per grid and shared."""
    C = _C()
    prob = _problem(box)
    co = C.Coeffs.from_problem(prob)
    gl = C.make_layout(prob, C.rank_box(prob, C.Dims(1, 1, 1), 0))
    full = C.compute_box(gl)
    s = ops.sin_table_ext(prob)
    torch.manual_seed(500 + (7 if box else 0))

    def rand_field():
        g = torch.zeros((N + 3,) * 3, dtype=torch.float64)
        g[2:-2, 2:-2, 2:-2] = torch.randn((N - 1,) * 3, dtype=torch.float64)
        return ops.from_grid(gl, g)

    prev, cur = rand_field(), rand_field()
    dense = lambda f: ops.to_grid(gl, f)[1:-1, 1:-1, 1:-1].numpy().copy()  # noqa: E731
    out = dict(prob=prob, co=co, prev=dense(prev), cur=dense(cur))
    a, b = prev.clone(), cur.clone()
    levels = []
    for _ in range(5):
        ops.leapfrog(gl, co, b, a, [full], s)
        a, b = b, a
        levels.append(dense(b))
    out["levels"] = levels
    return out


class Rank:
    def __init__(self, key, box):
        C = _C()
        self.dims, self.rank, self.g = LAYOUTS[key]
        self.G = _global(box)
        prob = self.G["prob"]
        self.D = C.Dims(*self.dims)
        self.lay = C.make_layout(prob, C.rank_box(prob, self.D, self.rank), 16, *self.g)
        l = self.lay
        self.n = [int(l.nx), int(l.ny), int(l.nz)]
        self.g0 = [int(l.gx0), int(l.gy0), int(l.gz0)]
        self.shape = (self.n[0] + 2 * self.g[0], self.n[1] + 2 * self.g[1], int(l.pitch))
        self.zc = self.g[2] + int(l.zs)
        self.nodes = receiver_set(N, self.dims)
        self.table = C.plan_receivers(prob, self.D, self.rank, l, self.nodes)  # (slot, x, y, z, off)
        assert len(self.table) >= 8

    def cut(self, glob, keep):
        """Padded local array: the nodes strictly inside the global grid and at most `keep` deep in the ghosts hold the
        global values; EVERYTHING else (deeper ghosts, nodes on or outside the global boundary, padding) is NaN."""
        idx, ok = [], []
        for a in range(3):
            i = np.arange(-self.g[a], self.n[a] + self.g[a])
            gi = i + self.g0[a]
            ok.append((gi > 0) & (gi < N) & (i >= -keep) & (i < self.n[a] + keep))
            idx.append(np.clip(gi, 0, N))
        sub = glob[np.ix_(*idx)]
        mask = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
        f = np.full(self.shape, np.nan)
        f[:, :, self.zc - self.g[2]: self.zc + self.n[2] + self.g[2]] = np.where(mask, sub, np.nan)
        return torch.from_numpy(f.reshape(-1)).cuda()


CASES = [(k, box) for k in LAYOUTS for box in (False, True)]


@pytest.mark.parametrize("key,box", CASES)
def test_record_cone_equals_cpu_steps(gpu, key, box):
    C = _C()
    R = Rank(key, box)
    G = R.G
    rtotal = len(R.nodes)
    slots = R.table[:, 0]
    want_nodes = R.nodes[slots]
    own = len(R.table)
    half = own // 2
    for s in (2, 3, 4, 5):
        prev, cur = R.cut(G["prev"], s - 1), R.cut(G["cur"], s)
        for lo, hi in ((0, own), (half, own)):  # every owned receiver; then only the second half of the table
            tab = torch.from_numpy(np.ascontiguousarray(R.table[lo:hi])).cuda()
            trace = torch.full((N0 + 7, rtotal), float("nan"), dtype=torch.float64, device="cuda")
            C.gpu_record_cone(R.lay, G["co"], prev.data_ptr(), cur.data_ptr(), N0, s, tab.data_ptr(), hi - lo,
                              trace.data_ptr(), rtotal, _stream())
            torch.cuda.synchronize()
            got = trace.cpu().numpy()
            exp = np.full_like(got, np.nan)
            for k in range(1, s + 1):
                lv = G["levels"][k - 1]
                exp[N0 + k, slots[lo:hi]] = lv[want_nodes[lo:hi, 0], want_nodes[lo:hi, 1], want_nodes[lo:hi, 2]]
            what = f"{key} box={box} s={s} receivers [{lo}, {hi})"
            assert not np.isnan(got[N0 + 1: N0 + s + 1][:, slots[lo:hi]]).any(), what
            bad = np.argwhere(got.view(np.int64) != exp.view(np.int64))
            assert bad.size == 0, (what, len(bad), bad[:5].tolist())
            if lo == 0:
                full5 = got  # (the last one kept: s = 5 over every owned receiver)
    got = full5
    # receivers on a global face: +0.0 at every level (they are in the table of a rank that touches the boundary)
    face = ((want_nodes == 0) | (want_nodes == N)).any(axis=1)
    assert face.any()
    assert same_bits(got[N0 + 1: N0 + 6][:, slots[face]], np.zeros((5, int(face.sum()))))


@pytest.mark.parametrize("key", list(LAYOUTS))
def test_record_gather_exact(gpu, key):
    """k_record_gather: row n of the trace = the field at the table's offsets, every other element untouched."""
    C = _C()
    R = Rank(key, False)
    rtotal = len(R.nodes)
    gen = torch.Generator().manual_seed(9)
    f = torch.randn(int(R.lay.total), dtype=torch.float64, generator=gen)
    tab = torch.from_numpy(np.ascontiguousarray(R.table)).cuda()
    trace = torch.full((6, rtotal), float("nan"), dtype=torch.float64, device="cuda")
    C.gpu_record_gather(f.cuda().data_ptr(), 4, tab.data_ptr(), len(R.table), trace.data_ptr(), rtotal, _stream())
    torch.cuda.synchronize()
    exp = np.full((6, rtotal), np.nan)
    exp[4, R.table[:, 0]] = f.numpy()[R.table[:, 4]]
    assert same_bits(trace.cpu().numpy(), exp)


def test_record_cone_refuses_shallow_ghosts(gpu):
    """A pass of s steps on a split axis with fewer than s ghost layers: refused on the host, nothing is launched."""
    C = _C()
    G = _global(False)
    D = C.Dims(4, 1, 1)
    lay = C.make_layout(G["prob"], C.rank_box(G["prob"], D, 1), 16, 2, 1, 1)
    with pytest.raises(Exception, match="ghosts that deep"):
        C.gpu_record_cone(lay, G["co"], 0, 0, 3, 3, 0, 1, 0, 1, _stream())
