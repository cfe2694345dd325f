"""k_source_cone at kernel level on rank layouts holding random data, NaN-poisoned where nothing may be touched.

One rank of a decomposition at N = 40 (one rank; slab 4x1x1 rank 1 with 5 ghost planes; block 2x2x2 rank 3 with ghost
depth 5 on every axis; each as cube and as box 1 x 1.3 x 0.7) gets two random local arrays — NaN on and outside the
global boundary and in the row padding — inside a larger buffer whose margins are NaN. Sources: the centre; (1, 1, 1),
clipped by three faces; a node next to the upper face; balls straddling the 32 x 32 tile edge; two at L1 distance 2 (two
colour classes) and two far apart (one class); a node listed twice; and, per split axis of the rank, nodes in its ghost
layers and nodes OUTSIDE its allocation whose ball reaches in. For s = 1..5 both outputs must equal field +
cpu_source_response bit for bit, applied in class order to the nodes inside the allocation and the global interior, and
every other element of the buffers — poison, margins — must keep its bits. The trace rows get the response at the owned
receivers inside each level's ball and keep their bits at the receivers just outside."""
import functools

import numpy as np
import pytest
import torch

from sources_common import BOX, receivers_around, same_bits

pytestmark = pytest.mark.gpu

N, K = 40, 9
N0 = 2  # the pass advances u^{N0} -> u^{N0 + s}
LAYOUTS = {"one": ((1, 1, 1), 0, (1, 1, 1)), "slab": ((4, 1, 1), 1, (5, 1, 1)), "block": ((2, 2, 2), 3, (5, 5, 5))}
MARGIN = 4096
COMMON = [[20, 20, 20], [1, 1, 1], [39, 17, 22], [31, 32, 9], [12, 31, 32], [20, 21, 21], [20, 20, 20]]


def _C():
    from mpi_cuda_amd._native import load

    return load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _problem(box):
    C = _C()
    return C.Problem(N, 0.005, K, BOX[0], Ly=BOX[1], Lz=BOX[2]) if box else C.Problem(N, 0.005, K, 1.0)


class Rank:
    def __init__(self, key, box):
        C = _C()
        self.dims, self.rank, self.g = LAYOUTS[key]
        self.prob = _problem(box)
        self.co = C.Coeffs.from_problem(self.prob)
        self.D = C.Dims(*self.dims)
        b = C.rank_box(self.prob, self.D, self.rank)
        self.lay = l = C.make_layout(self.prob, b, 16, *self.g)
        self.n = [int(l.nx), int(l.ny), int(l.nz)]
        self.g0 = [int(l.gx0), int(l.gy0), int(l.gz0)]
        lo, hi = self.g0, [self.g0[a] + self.n[a] for a in range(3)]
        mid = [(lo[a] + hi[a]) // 2 for a in range(3)]
        v = [list(n) for n in COMMON]
        for a in range(3):
            if self.dims[a] == 1:
                continue
            # in the ghost layers (2 deep), and 2 / 1 nodes beyond the allocation's last ghost layer
            for x in (lo[a] - 2, lo[a] - self.g[a] - 2, hi[a] + 1, hi[a] + self.g[a] + 1):
                n = list(mid)
                n[a] = x
                v.append(n)
        split = [a for a in range(3) if self.dims[a] > 1]
        if split:  # beyond the allocation's corner on every split axis at once
            n = list(mid)
            for a in split:
                n[a] = lo[a] - self.g[a] - 1
            v.append(n)
        v = np.array(v, dtype=np.int64)
        self.nodes = v[((v > 0) & (v < N)).all(axis=1)]
        self.table, self.class_begin = C.plan_sources(self.prob, self.D, self.rank, l, self.nodes, 4)
        self.recv_nodes = receivers_around(self.nodes, N)
        self.rtable = C.plan_receivers(self.prob, self.D, self.rank, l, self.recv_nodes)
        # the local index ranges of the allocation and their global nodes
        self.idx = [np.arange(-self.g[a], self.n[a] + self.g[a]) for a in range(3)]
        self.total = int(l.total)

    def inside(self, x, y, z):
        return all(-self.g[a] <= v < self.n[a] + self.g[a] for a, v in enumerate((x, y, z)))

    def field(self, seed):
        """Random values at every allocation node strictly inside the global grid, NaN everywhere else."""
        l = self.lay
        f = np.full(self.total, np.nan)
        rng = np.random.default_rng(seed)
        ok = [(self.idx[a] + self.g0[a] > 0) & (self.idx[a] + self.g0[a] < N) for a in range(3)]
        for i, x in enumerate(self.idx[0]):
            for j, y in enumerate(self.idx[1]):
                if not (ok[0][i] and ok[1][j]):
                    continue
                z = self.idx[2][ok[2]]
                o = int(l.off(int(x), int(y), int(z[0])))
                f[o:o + len(z)] = rng.standard_normal(len(z))
        return f


def _guarded(f):
    buf = torch.full((len(f) + 2 * MARGIN,), float("nan"), dtype=torch.float64)
    buf[MARGIN:-MARGIN] = torch.from_numpy(f)
    return buf.cuda()


def _cells(s_radius):
    r = s_radius
    return [(a, b, c) for a in range(-r, r + 1) for b in range(-r, r + 1) for c in range(-r, r + 1)
            if abs(a) + abs(b) + abs(c) <= r]


def _expected(R, f0, f1, a, n, s, start, trace):
    """field + cpu_source_response in table (class) order on the nodes inside the allocation and the global interior;
    trace rows n + k get level k's response at the owned receivers within distance k - 1."""
    C = _C()
    e0, e1, et = f0.copy(), f1.copy(), trace.copy()
    l = R.lay
    for slot, x, y, z, off in R.table.tolist():
        node = R.nodes[slot].tolist()
        col = a[0:1, slot] if start else a[n:n + s, slot]
        last, prev = C.cpu_source_response(R.prob, R.co, node, np.ascontiguousarray(col), start, s)
        for (i, j, k) in _cells(s - 1):
            g = (node[0] + i, node[1] + j, node[2] + k)
            if not all(0 < v < N for v in g) or not R.inside(x + i, y + j, z + k):
                continue
            o = int(l.off(x + i, y + j, z + k))
            assert o == off + i * int(l.plane) + j * int(l.pitch) + k
            e0[o] += last[i + 5, j + 5, k + 5]
            if abs(i) + abs(j) + abs(k) <= s - 2:
                e1[o] += prev[i + 5, j + 5, k + 5]
        if start:
            continue
        for k in range(1, s + 1):
            lv = C.cpu_source_response(R.prob, R.co, node, np.ascontiguousarray(a[n:n + k, slot]), False, k)[0]
            for rslot, rx, ry, rz, _ in R.rtable.tolist():
                d = (rx - x, ry - y, rz - z)
                if sum(abs(v) for v in d) <= k - 1:
                    et[n + k, rslot] += lv[d[0] + 5, d[1] + 5, d[2] + 5]
    return e0, e1, et


def _launch(R, f0, f1, a, n, s, start, trace):
    C = _C()
    b0, b1 = _guarded(f0), _guarded(f1)
    tab = torch.from_numpy(np.ascontiguousarray(R.table)).cuda()
    rtab = torch.from_numpy(np.ascontiguousarray(R.rtable)).cuda()
    ad, tr = torch.from_numpy(a).cuda(), torch.from_numpy(trace).cuda()
    nrec = 0 if start else len(R.rtable)
    C.gpu_source_cone(R.lay, R.co, b1.data_ptr() + 8 * MARGIN, b0.data_ptr() + 8 * MARGIN, n, s, start, tab.data_ptr(),
                      list(R.class_begin), ad.data_ptr(), a.shape[1], rtab.data_ptr() if nrec else 0, nrec,
                      tr.data_ptr() if nrec else 0, trace.shape[1], _stream())
    torch.cuda.synchronize()
    return b0.cpu().numpy(), b1.cpu().numpy(), tr.cpu().numpy()


def _pad(f):
    return np.concatenate([np.full(MARGIN, np.nan), f, np.full(MARGIN, np.nan)])


CASES = [(k, box) for k in LAYOUTS for box in (False, True)]


@pytest.mark.parametrize("key,box", CASES)
def test_source_cone_equals_cpu_response(gpu, key, box):
    R = Rank(key, box)
    Q = len(R.nodes)
    assert len(R.table) >= 3 and len(R.rtable) >= 6
    rng = np.random.default_rng(11)
    a = np.ascontiguousarray(rng.integers(-8, 9, size=(K, Q)) / 4.0)
    f0, f1 = R.field(1), R.field(2)
    touched = 0
    for s in (1, 2, 3, 4, 5):
        trace = rng.standard_normal((N0 + 7, len(R.recv_nodes)))
        e0, e1, et = _expected(R, f0, f1, a, N0, s, False, trace)
        g0, g1, gt = _launch(R, f0, f1, a, N0, s, False, trace)
        what = f"{key} box={box} s={s}"
        for got, exp, name in ((g0, _pad(e0), "out_last"), (g1, _pad(e1), "out_prev")):
            bad = np.flatnonzero(got.view(np.int64) != exp.view(np.int64))
            assert bad.size == 0, (what, name, len(bad), (bad[:5] - MARGIN).tolist())
        assert same_bits(gt, et), what
        touched += int((gt != trace).sum())
        assert (e0 != f0)[~np.isnan(f0)].any() and (s == 1 or (e1 != f1)[~np.isnan(f1)].any()), what
        assert same_bits(e1, f1) if s == 1 else True
    assert touched > 0  # (some receiver was inside a cone)
    # the start level: u^1 += a[0] / 2 at the source nodes inside the allocation, nothing else
    e0, e1, _ = _expected(R, f0, f1, a, 0, 1, True, np.zeros((1, 1)))
    g0, g1, _ = _launch(R, f0, f1, a, 0, 1, True, np.zeros((2, len(R.recv_nodes))))
    assert same_bits(g0, _pad(e0)) and same_bits(g1, _pad(f1)) and same_bits(e1, f1)


def test_colour_classes_and_outside_sources(gpu):
    """The plan the kernel tests run on: distance-2 and duplicate sources in separate classes, far ones together; a slab
    rank keeps sources outside its allocation (local x below -xg), and drops the ones whose ball cannot reach it."""
    R = Rank("one", False)
    cls = {}
    for c in range(len(R.class_begin) - 1):
        for row in R.table[R.class_begin[c]:R.class_begin[c + 1]].tolist():
            cls[row[0]] = c
    assert len(cls) == len(R.nodes)
    assert cls[0] == cls[1] == cls[2] == 0  # centre, (1,1,1), upper face: far apart
    assert len({cls[0], cls[5], cls[6]}) == 3  # centre, its distance-2 neighbour, the centre again
    S = Rank("slab", False)
    x = S.table[:, 1]
    assert (x < -S.g[0]).any() and (x >= S.n[0] + S.g[0]).any() and ((x >= -S.g[0]) & (x < 0)).any()
    assert len(S.table) < len(S.nodes)


def test_source_cone_refusals(gpu):
    C = _C()
    R = Rank("slab", False)
    with pytest.raises(Exception, match="both output levels"):
        C.gpu_source_cone(R.lay, R.co, 0, 8, 2, 2, False, 0, [0, 0], 0, 1, 0, 0, 0, 1, _stream())
    lay = C.make_layout(R.prob, C.rank_box(R.prob, R.D, 1), 16, 2, 1, 1)
    with pytest.raises(Exception, match="ghosts that deep"):
        C.gpu_source_cone(lay, R.co, 8, 8, 2, 3, False, 0, [0, 0], 0, 1, 0, 0, 0, 1, _stream())
    with pytest.raises(Exception, match="1..5 steps"):
        C.gpu_source_cone(R.lay, R.co, 8, 8, 2, 6, False, 0, [0, 0], 0, 1, 0, 0, 0, 1, _stream())
