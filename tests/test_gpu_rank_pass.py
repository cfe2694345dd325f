"""The LDS multi-step passes (k_leapfrog_p2, k_leapfrog_tb), k_box_copy and k_field_hash on RANK layouts with RANDOM
data, each against a reference computed independently of it.

The multi-rank solves start from the analytic state — a separable sine product, mirror-symmetric about the middle of
every axis and unchanged by swapping equal axes — so a lo/hi or y/z mix-up in a region table, a ghost store or a pack
offset can move bit-identical data there. Here the global fields are random: one rank of a decomposition gets the
global u^{n-1}, u^n cut to its S-deep ghosts, runs one pass, and its whole padded output arrays are compared with S
native CPU single steps of the undecomposed grid, bit for bit.

Ghost nodes the pass must not read hold NaN (beyond the global boundary; u^{n-1} deeper than S - 1), the outputs are
pre-filled with random sentinels, and every node outside the box must keep its sentinel bits. Writes beyond the box
that the kernels make by design are pinned in `_expected`:
  * the pair-tiled pass stores whole 16-byte pairs, so a box of odd z width that ends at the rank's last updated node
    also writes the node after it (a z ghost or the global boundary): u^{n+S-1} there is the true value; u^{n+S} is +0
    on the global boundary and UNSPECIFIED in a neighbour's ghost (level S one node beyond the box depends on inputs
    beyond the S-deep contract; the next exchange, at least 2 deep, overwrites it);
  * ghost_x1 stores u^{n+S-1} on plane x0 - 1 / x1 over the same (y, z) nodes.
"""
import functools
import math

import numpy as np
import pytest
import torch

from mpi_cuda_amd.ops import stencil as ops

pytestmark = pytest.mark.gpu

TAU = 1e-3
EDGES = (1.0, 1.3, 0.7)
# (N, dims, rank): neighbours on all six sides with 33-node extents; opposite corners with odd extents; unequal ny / nz;
# a slab rank between two others
RANKS = {"r13": (100, (3, 3, 3), 13), "c0": (67, (2, 2, 2), 0), "c7": (67, (2, 2, 2), 7), "b4": (70, (1, 2, 3), 4),
         "s1": (66, (3, 1, 1), 1)}


def _C():
    from mpi_cuda_amd._native import load

    return load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _problem(N, box):
    C = _C()
    return C.Problem(N, TAU, 20, EDGES[0], Ly=EDGES[1], Lz=EDGES[2]) if box else C.Problem(N, TAU, 20, 1.0)


# ---- the global reference: random u^{n-1}, u^n on the whole grid and five native CPU steps, once per grid
@functools.lru_cache(maxsize=None)
def _global(N, box=False):
    C = _C()
    prob = _problem(N, box)
    co = C.Coeffs.from_problem(prob)
    gl = C.make_layout(prob, C.rank_box(prob, C.Dims(1, 1, 1), 0))
    full = C.compute_box(gl)
    s = ops.sin_table_ext(prob)
    torch.manual_seed(N * 31 + (7 if box else 0))

    def rand_field():
        g = torch.zeros((N + 3,) * 3, dtype=torch.float64)
        g[2:-2, 2:-2, 2:-2] = torch.randn((N - 1,) * 3, dtype=torch.float64)
        return ops.from_grid(gl, g)

    prev, cur = rand_field(), rand_field()
    ct = [math.cos(prob.a_t * (5 + k) * prob.tau) for k in range(1, 6)]
    a, b = prev.clone(), cur.clone()
    flat = []
    for k in range(1, 6):
        ops.leapfrog(gl, co, b, a, [full], s)
        a, b = b, a
        flat.append(b.clone())
    if not box:  # the plain fp64 torch reference of the last step (uniform grids)
        ref = ops.ref_leapfrog_grid(ops.to_grid(gl, flat[3]), ops.to_grid(gl, flat[2]), co.ihx2, co.ihy2, co.ihz2,
                                    co.tau2, full)
        torch.testing.assert_close(ops.to_grid(gl, flat[4]), ref, rtol=0, atol=1e-9)
    dense = lambda f: ops.to_grid(gl, f)[1:-1, 1:-1, 1:-1].numpy().copy()  # noqa: E731
    return dict(prob=prob, co=co, gl=gl, s=s, ct=ct, prev=dense(prev), cur=dense(cur), flat=flat,
                levels=[dense(f) for f in flat])


def _cpu_error(G, lay, boxes, k):
    """CPU error of global level u^{n+k} over the rank-local boxes (max of the maxima, sum of the sums)."""
    C = _C()
    mx, sm = 0.0, 0.0
    for b in boxes:
        gb = C.LBox(b.x0 + lay.gx0, b.x1 + lay.gx0, b.y0 + lay.gy0, b.y1 + lay.gy0, b.z0 + lay.gz0, b.z1 + lay.gz0)
        m, q = C.cpu_error(G["gl"], G["flat"][k - 1].numpy(), gb, G["s"].numpy(), G["ct"][k - 1])
        mx, sm = max(mx, m), sm + q
    return mx, sm


# ---- a rank of a decomposition
class Rank:
    def __init__(self, key, S, box=False):
        C = _C()
        self.N, self.dims, self.rank = RANKS[key]
        self.S = S
        self.G = _global(self.N, box)
        self.s_gpu = self.G["s"].cuda()
        D = C.Dims(*self.dims)
        self.D = D
        slab = self.dims[1] == 1 and self.dims[2] == 1
        # ghost depths as make_rank_schedule sets them: S on x when x is split, on y / z when split on a block rank
        g = [S if self.dims[0] > 1 else 1, S if (not slab and self.dims[1] > 1) else 1,
             S if (not slab and self.dims[2] > 1) else 1]
        self.lay = C.make_layout(self.G["prob"], C.rank_box(self.G["prob"], D, self.rank), 16, *g)
        self.full = C.compute_box(self.lay)
        self.nb = [[C.neighbor_rank(D, self.rank, a, side) >= 0 for side in (0, 1)] for a in range(3)]
        f = self.full.as_tuple()
        r = []
        for a in range(3):
            r += [f[2 * a] - (S - 1 if self.nb[a][0] else 0), f[2 * a + 1] + (S - 1 if self.nb[a][1] else 0)]
        self.real = C.LBox(*r)  # RankSchedule::sreal
        l = self.lay
        self.g = [int(l.xg), int(l.yg), int(l.zg)]
        self.n = [int(l.nx), int(l.ny), int(l.nz)]
        self.g0 = [int(l.gx0), int(l.gy0), int(l.gz0)]
        self.shape = (self.n[0] + 2 * self.g[0], self.n[1] + 2 * self.g[1], int(l.pitch))
        self.zc = self.g[2] + int(l.zs)  # column of local node z = 0

    def nodes(self, f):
        """(x, y, z) view of the nodes (ghosts included) of a padded array of shape self.shape."""
        return f[:, :, self.zc - self.g[2]: self.zc + self.n[2] + self.g[2]]

    def sl(self, b):
        """index of local box b (LBox or 6-tuple) in the `nodes` view"""
        x0, x1, y0, y1, z0, z1 = b if isinstance(b, tuple) else b.as_tuple()
        g = self.g
        return (slice(x0 + g[0], x1 + g[0]), slice(y0 + g[1], y1 + g[1]), slice(z0 + g[2], z1 + g[2]))

    def cut(self, glob, keep=None):
        """Padded local array from a global (N+1)^3 field: every node inside the domain (ghosts included); NaN beyond
        the global boundary and, with `keep`, in ghosts deeper than `keep` nodes; row padding 0."""
        N = self.N
        idx, ok = [], []
        for a in range(3):
            i = np.arange(-self.g[a], self.n[a] + self.g[a])
            good = (i + self.g0[a] >= 0) & (i + self.g0[a] <= N)
            if keep is not None:
                good &= (i >= -keep) & (i < self.n[a] + keep)
            idx.append(np.clip(i + self.g0[a], 0, N))
            ok.append(good)
        sub = glob[np.ix_(*idx)]
        mask = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
        f = np.zeros(self.shape)
        self.nodes(f)[...] = np.where(mask, sub, np.nan)
        return f

    def inputs(self):
        G, S = self.G, self.S
        prev = torch.from_numpy(self.cut(G["prev"], keep=S - 1)).reshape(-1).cuda()
        cur = torch.from_numpy(self.cut(G["cur"], keep=S)).reshape(-1).cuda()
        return prev, cur

    def sentinels(self, seed):
        gen = torch.Generator().manual_seed(seed)
        o1 = torch.randn(int(self.lay.total), dtype=torch.float64, generator=gen)
        o2 = torch.randn(int(self.lay.total), dtype=torch.float64, generator=gen)
        return o1, o2

    def splits(self, w):
        C = _C()
        shells, interior = C.deep_split(self.full, self.nb, w, 32)
        return list(shells), interior


def _tiling(S, p2, target, ghost_x1=0, xcd_remap=True):
    t = _C().LeapfrogTbTiling()
    t.stages, t.p2, t.target_blocks, t.ghost_x1, t.xcd_remap = S, p2, target, ghost_x1, xcd_remap
    return t


def _expected(R, sent1, sent2, boxes, p2, ghost_x1=0):
    """What the output arrays must hold after a pass over `boxes`: (exp1, exp2, free) — `free`: the nodes of out2
    whose value is unspecified (module docstring), as a boolean array over the nodes."""
    G, S = R.G, R.S
    e1, e2 = sent1.numpy().reshape(R.shape).copy(), sent2.numpy().reshape(R.shape).copy()
    l1 = R.nodes(R.cut(G["levels"][S - 2]))
    l2 = R.nodes(R.cut(G["levels"][S - 1]))
    free = np.zeros(l1.shape, dtype=bool)
    f = R.full.as_tuple()
    for b in boxes:
        x0, x1, y0, y1, z0, z1 = b.as_tuple()
        odd = p2 and z1 == f[5] and (z1 - z0) % 2 == 1
        w = R.sl((x0, x1, y0, y1, z0, z1 + (1 if odd else 0)))
        R.nodes(e1)[w] = l1[w]
        R.nodes(e2)[w] = l2[w]
        if odd and R.g0[2] + z1 < R.N:  # a neighbour's ghost, not the global boundary
            free[R.sl((x0, x1, y0, y1, z1, z1 + 1))] = True
        if (ghost_x1 & 1) and x0 == f[0]:
            w = R.sl((x0 - 1, x0, y0, y1, z0, z1 + (1 if odd else 0)))
            R.nodes(e1)[w] = l1[w]
        if (ghost_x1 & 2) and x1 == f[1]:
            w = R.sl((x1, x1 + 1, y0, y1, z0, z1 + (1 if odd else 0)))
            R.nodes(e1)[w] = l1[w]
    return e1, e2, free


def _assert_fields(R, o1, o2, exp, what):
    e1, e2, free = exp
    g1, g2 = o1.cpu().numpy().reshape(R.shape), o2.cpu().numpy().reshape(R.shape)
    # (`free`: level S one node beyond the box depends on u^n S + 1 nodes beyond it, outside the contract — with the
    # poisoned inputs of this test it is NaN; any value is allowed there and nowhere else)
    e2 = e2.copy()
    R.nodes(e2)[free] = R.nodes(g2)[free]
    for name, g, e in (("out1", g1, e1), ("out2", g2, e2)):
        bad = np.argwhere(g.view(np.int64) != e.view(np.int64))
        assert bad.size == 0, (what, name, len(bad), bad[:5].tolist(), R.g, R.zc)


def _assert_errors(R, part, stride, count, mask, boxes, what):
    C = _C()
    for k in range(1, R.S + 1):
        if not mask >> (k - 1) & 1:
            continue
        out = torch.empty(2, dtype=torch.float64, device="cuda")
        C.gpu_reduce(part[(k - 1) * stride:].data_ptr(), count, out.data_ptr(), _stream())
        m, q = (float(v) for v in out.cpu())
        em, eq = _cpu_error(R.G, R.lay, boxes, k)
        print(f"{what} level {k}: max {m!r} / {em!r}  sum {q!r} / {eq!r}")
        assert m == em, (what, k)
        assert math.isclose(q, eq, rel_tol=1e-12), (what, k)


def _run_box(R, box, p2, target, mask, seed, ghost_x1=0, prev_cur=None, pack=None):
    """One launch_leapfrog_tb over `box` with the slot geometry GpuSolver::tb_args uses; returns (out1, out2)."""
    C = _C()
    S, lay, G = R.S, R.lay, R.G
    t = _tiling(S, p2, target, ghost_x1)
    tmax = _tiling(S, p2, target)
    slot = C.tb_slot_blocks(lay, R.full, tmax, True)
    prev, cur = prev_cur if prev_cur is not None else R.inputs()
    s1, s2 = R.sentinels(seed)
    o1, o2 = s1.cuda(), s2.cuda()
    part = torch.full((S * slot, 2), float("nan"), dtype=torch.float64, device="cuda")
    kw = dict(pack_zf=pack[0], pack_w=pack[1]) if pack else {}
    C.gpu_leapfrog_tb(lay, G["co"], prev.data_ptr(), cur.data_ptr(), o1.data_ptr(), o2.data_ptr(), box,
                      R.s_gpu.data_ptr(), G["ct"][:S], mask, part.data_ptr() if mask else 0, t, _stream(),
                      real=R.real, level_stride=slot, grid_blocks=slot, **kw)
    torch.cuda.synchronize()
    what = f"rank {R.rank} of {R.dims} N={R.N} S={S} p2={p2} target={target} mask={mask:#b} box={box.as_tuple()}"
    _assert_fields(R, o1, o2, _expected(R, s1, s2, [box], p2 and not pack, ghost_x1), what)
    _assert_errors(R, part, slot, slot, mask, [box], what)
    return o1, o2


def _masks(S):
    full = (1 << S) - 1
    return [full, 0b10101 & full, 0]


P2_CASES = [(k, S) for k in RANKS for S in (2, 3, 4, 5)]
TB_CASES = [(k, S) for k in RANKS for S in (2, 3, 4)]


def _pass_case(key, S, p2):
    R = Rank(key, S)
    C = _C()
    assert (not p2) or C.gpu_leapfrog_p2_supported(R.lay, R.full, S)
    pc = R.inputs()
    shells, interior = R.splits(S)
    assert shells and len(shells) < 8
    subs = shells + ([interior] if not interior.empty() else [])
    for b in subs:
        assert (not p2) or C.gpu_leapfrog_p2_supported(R.lay, b, S)
    seed = 0
    for target in (1, 256):
        for mask in _masks(S):
            seed += 1
            _run_box(R, R.full, p2, target, mask, seed, prev_cur=pc)
        for b in subs:
            seed += 1
            _run_box(R, b, p2, target, _masks(S)[0 if target == 256 else 1], seed, prev_cur=pc)


@pytest.mark.parametrize("key,S", P2_CASES)
def test_p2_rank_pass_equals_global_cpu_steps(gpu, key, S):
    """k_leapfrog_p2 on one rank (S-deep ghosts, `real` wider than the box, the whole compute box and every shell /
    interior box of deep_split, with and without x chunks, check masks all / odd / none) against S CPU steps of the
    undecomposed random grid. Catches: a mirrored or axis-swapped region (lo/hi, y/z) in the halo loads, the stage-real
    ranges or the box tables; a read of a ghost beyond the contract or beyond the global boundary (NaN); a store
    outside the box (sentinels); an error partial of a node outside the box."""
    _pass_case(key, S, True)


@pytest.mark.parametrize("key,S", TB_CASES)
def test_tb_rank_pass_equals_global_cpu_steps(gpu, key, S):
    """The same for k_leapfrog_tb (one node per thread, S <= 4; it stores exactly the box). Catches the same defects
    in its zero-slot loads and real ranges."""
    _pass_case(key, S, False)


@pytest.mark.parametrize("p2", [True, False])
def test_rank_pass_box_form(gpu, p2):
    """The rectangular-box instantiations (Ly, Lz != Lx) on a rank layout: rank 4 of 1x2x3, S = 4. Catches a y/z ratio
    applied to the wrong axis, which the cube cannot show."""
    R = Rank("b4", 4, box=True)
    assert R.G["co"].box
    pc = R.inputs()
    shells, interior = R.splits(4)
    for i, b in enumerate([R.full] + shells + ([interior] if not interior.empty() else [])):
        _run_box(R, b, p2, 256 if i % 2 == 0 else 1, 0b1111, 100 + i, prev_cur=pc)


# ---- several boxes in one launch
def _run_boxes(R, boxes, target, mask, seed, pc, grid_pad=5):
    C = _C()
    S, lay, G = R.S, R.lay, R.G
    t = _tiling(S, True, target, xcd_remap=False)  # (as GpuSolver::tb_pass_boxes)
    nblocks, per = C.p2_launch_blocks(boxes, t)
    grid = nblocks + grid_pad  # a padded grid: the extra workgroups must write (0, 0) partials
    s1, s2 = R.sentinels(seed)
    o1, o2 = s1.cuda(), s2.cuda()
    part = torch.full((S * grid, 2), float("nan"), dtype=torch.float64, device="cuda")
    C.gpu_leapfrog_p2_boxes(lay, G["co"], pc[0].data_ptr(), pc[1].data_ptr(), o1.data_ptr(), o2.data_ptr(), boxes,
                            R.s_gpu.data_ptr(), G["ct"][:S], mask, part.data_ptr(), t, _stream(), real=R.real,
                            level_stride=grid, grid_blocks=grid)
    torch.cuda.synchronize()
    what = f"rank {R.rank} of {R.dims} N={R.N} S={S} {len(boxes)} boxes target={target}"
    _assert_fields(R, o1, o2, _expected(R, s1, s2, boxes, True), what)
    _assert_errors(R, part, grid, grid, mask, boxes, what)
    return o1, o2, per


@pytest.mark.parametrize("key,S,target", [("r13", 5, 256), ("r13", 5, 3), ("r13", 3, 3), ("c0", 4, 256),
                                          ("c7", 5, 3), ("b4", 2, 256), ("s1", 5, 256)])
def test_p2_shell_boxes_in_one_launch(gpu, key, S, target):
    """launch_leapfrog_p2_boxes over all shell boxes of a rank (no XCD remap, a padded shared partial slot): equal to
    one launch per box and to the global reference, nodes of no box untouched, the slot's partials reduce to the CPU
    error over the union. target 3: boxes whose work share is below their tile count keep their tiles (the regime in
    which the combined grid outgrows target_blocks; these 33-node ranks have only two to four one-by-two-tile shells,
    so the share falls below the tiles at 3, not at 12). Catches: a dropped or doubled box slot (blk0 offsets), a box
    running with another box's chunk length, unwritten partials of the padding workgroups."""
    R = Rank(key, S)
    C = _C()
    pc = R.inputs()
    shells, _ = R.splits(S)
    assert 2 <= len(shells) <= 6
    o1, o2, per = _run_boxes(R, shells, target, (1 << S) - 1, 7, pc)
    blk = 0
    for nty, ntz, xlen, nxc, blk0 in per:  # the blk0 are the prefix sums
        assert blk0 == blk
        blk += nty * ntz * nxc
    if target == 3:
        work = [math.ceil((b.y1 - b.y0) / 32) * math.ceil((b.z1 - b.z0) / 32) * (b.x1 - b.x0) for b in shells]
        assert any(int(target * w / sum(work)) < p[0] * p[1] for w, p in zip(work, per))
        assert blk > target
    # one launch per box into the same (sentinel-seeded) arrays gives the same bits
    s1, s2 = R.sentinels(7)
    q1, q2 = s1.cuda(), s2.cuda()
    t = _tiling(S, True, target)
    for b in shells:
        C.gpu_leapfrog_tb(R.lay, R.G["co"], pc[0].data_ptr(), pc[1].data_ptr(), q1.data_ptr(), q2.data_ptr(), b,
                          R.s_gpu.data_ptr(), R.G["ct"][:S], 0, 0, t, _stream(), real=R.real)
    torch.cuda.synchronize()
    _, _, free = _expected(R, s1, s2, shells, True)
    a2, b2 = o2.cpu().numpy().reshape(R.shape).copy(), q2.cpu().numpy().reshape(R.shape).copy()
    R.nodes(a2)[free] = 0.0
    R.nodes(b2)[free] = 0.0
    assert torch.equal(o1.cpu(), q1.cpu()) and np.array_equal(a2.view(np.int64), b2.view(np.int64))


# ---- ghost_x1
@pytest.mark.parametrize("S", [2, 5])
@pytest.mark.parametrize("bits", [1, 2, 3])
def test_p2_ghost_plane_stores(gpu, S, bits):
    """ghost_x1 on the slab rank: plane x0 - 1 (bit 0) / x1 (bit 1) of out1 holds global u^{n+S-1} after a pass over
    a box that touches that face, and a box that does not touch it stores nothing there (`_expected` pins both).
    Catches: the two bits or the two planes swapped, a ghost plane stored from the wrong level, a shell storing the
    other face's plane."""
    R = Rank("s1", S)
    pc = R.inputs()
    shells, interior = R.splits(S)
    assert len(shells) == 2 and shells[0].x0 == R.full.x0 and shells[1].x1 == R.full.x1 and not interior.empty()
    for i, (b, target) in enumerate([(R.full, 256), (R.full, 1), (shells[0], 256), (shells[1], 256), (interior, 256)]):
        _run_box(R, b, True, target, (1 << S) - 1, 40 + i, ghost_x1=bits, prev_cur=pc)


# ---- the fused z-face pack
@pytest.mark.parametrize("key,S,w", [("r13", 4, 4), ("r13", 3, 2), ("c0", 4, 3), ("c7", 2, 2), ("b4", 3, 3)])
def test_tb_fused_zface_pack(gpu, key, S, w):
    """TbPack (k_leapfrog_tb): the pass stores the owned nodes of the two z-face message parts of the next exchange
    (depth w: u^{n+S} w deep, u^{n+S-1} w - 1 deep) into the send staging; entries on the global boundary are never
    written. Compared with the DeepPlan send regions gathered from the global levels. Catches: the low and high face
    or the two fields swapped, a band of the wrong width, a y/z transposed part, a write outside the parts."""
    C = _C()
    R = Rank(key, S)
    plan = C.make_deep_plan(R.lay, R.D, R.rank, w)
    total = int(plan.total)
    gen = torch.Generator().manual_seed(S * 10 + w)
    init = torch.randn(total, dtype=torch.float64, generator=gen)
    buf = init.cuda()
    exp = init.numpy().copy()
    zf = [0, 0, 0, 0]
    lv = {0: R.nodes(R.cut(R.G["levels"][S - 1])), 1: R.nodes(R.cut(R.G["levels"][S - 2]))}
    inner = [(np.arange(R.n[a]) + R.g0[a] >= 1) & (np.arange(R.n[a]) + R.g0[a] <= R.N - 1) for a in range(3)]
    for q in plan.peers:
        if q.dir[0] != 0 or q.dir[1] != 0:
            continue
        for part in q.parts:
            off = int(q.buf_off + part.off)
            zf[2 * (1 if q.dir[2] > 0 else 0) + part.field] = buf.data_ptr() + 8 * off
            x0, x1, y0, y1, z0, z1 = part.send.as_tuple()
            vals = lv[part.field][R.sl(part.send)]
            real = inner[0][x0:x1, None, None] & inner[1][None, y0:y1, None] & inner[2][None, None, z0:z1]
            cnt = vals.size
            exp[off:off + cnt] = np.where(real, vals, exp[off:off + cnt].reshape(vals.shape)).reshape(-1)
    assert any(zf)
    _run_box(R, R.full, False, 256, (1 << S) - 1, 60 + w, pack=(zf, w))
    got = buf.cpu().numpy()
    bad = np.argwhere(got.view(np.int64) != exp.view(np.int64))
    assert bad.size == 0, (len(bad), bad[:5].tolist())


# ---- k_box_copy against a numpy gather
@pytest.mark.parametrize("s", [2, 3, 4, 5])
@pytest.mark.parametrize("key", list(RANKS))
def test_box_copy_matches_numpy_gather(gpu, key, s):
    """k_box_copy in its three modes against the DeepPlan regions walked in numpy (part.send / part.recv, part.off,
    peer.buf_off): pack = the concatenation of the send regions, staging outside every region untouched; unpack changes
    only the receive regions, to the buffer's values; poison makes exactly those nodes NaN; skip_zfaces leaves the
    (0, 0, +-1) parts alone. Catches: a mirrored send / receive region, the two fields swapped, y/z transposed element
    order, a part at the wrong offset."""
    C = _C()
    R = Rank(key, s)
    plan = C.make_deep_plan(R.lay, R.D, R.rank, s)
    total = int(plan.total)
    assert total > 0
    gen = torch.Generator().manual_seed(s)
    us = torch.randn(int(R.lay.total), dtype=torch.float64, generator=gen)
    us1 = torch.randn(int(R.lay.total), dtype=torch.float64, generator=gen)
    sent = torch.randn(total, dtype=torch.float64, generator=gen)
    fields = {0: R.nodes(us.numpy().reshape(R.shape)), 1: R.nodes(us1.numpy().reshape(R.shape))}
    parts = [(q, p) for q in plan.peers for p in q.parts]
    for skip in (False, True):
        tab = C.make_box_copy_table(plan, False, skip)
        try:
            buf, d0, d1 = sent.cuda(), us.cuda(), us1.cuda()
            C.launch_box_copy(R.lay, tab, 0, d0.data_ptr(), d1.data_ptr(), buf.data_ptr(), _stream())
            torch.cuda.synchronize()
        finally:
            C.free_box_copy_table(tab)
        exp = sent.numpy().copy()
        for q, p in parts:
            if skip and q.dir[0] == 0 and q.dir[1] == 0:
                continue
            v = fields[p.field][R.sl(p.send)].reshape(-1)
            o = int(q.buf_off + p.off)
            exp[o:o + v.size] = v
        assert np.array_equal(buf.cpu().numpy().view(np.int64), exp.view(np.int64)), skip
    for mode in (1, 2):
        tab = C.make_box_copy_table(plan, True, False)
        try:
            a, b = us.cuda(), us1.cuda()
            buf = sent.cuda()
            C.launch_box_copy(R.lay, tab, mode, a.data_ptr(), b.data_ptr(), buf.data_ptr() if mode == 1 else 0,
                              _stream())
            torch.cuda.synchronize()
        finally:
            C.free_box_copy_table(tab)
        e = {0: us.numpy().reshape(R.shape).copy(), 1: us1.numpy().reshape(R.shape).copy()}
        for q, p in parts:
            w = R.sl(p.recv)
            o = int(q.buf_off + p.off)
            n = R.nodes(e[p.field])[w].size
            R.nodes(e[p.field])[w] = sent.numpy()[o:o + n].reshape(R.nodes(e[p.field])[w].shape) if mode == 1 \
                else np.nan
        for f, g in ((0, a), (1, b)):
            assert np.array_equal(g.cpu().numpy().view(np.int64), e[f].reshape(-1).view(np.int64)), (mode, f)


# ---- k_field_hash against its definition
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix64(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xbf58476d1ce4e5b9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def _hash_ref(R, f):
    """Sum over the owned nodes of mix64(bits ^ mix64(global index)) mod 2^64 (kernels.hpp launch_field_hash)."""
    owned = R.nodes(f.reshape(R.shape))[R.sl((0, R.n[0], 0, R.n[1], 0, R.n[2]))]
    n1 = np.uint64(R.N + 1)
    gx = (np.arange(R.n[0]) + R.g0[0]).astype(np.uint64)[:, None, None]
    gy = (np.arange(R.n[1]) + R.g0[1]).astype(np.uint64)[None, :, None]
    gz = (np.arange(R.n[2]) + R.g0[2]).astype(np.uint64)[None, None, :]
    idx = (gx * n1 + gy) * n1 + gz
    with np.errstate(over="ignore"):
        h = _mix64(np.ascontiguousarray(owned).view(np.uint64) ^ _mix64(idx))
        return int(h.sum(dtype=np.uint64))


def _hash_gpu(R, f):
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    _C().launch_field_hash(R.lay, f.data_ptr(), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return int(out.cpu().numpy().view(np.uint64)[0])


@pytest.mark.parametrize("key", list(RANKS))
def test_field_hash_matches_definition(gpu, key):
    """k_field_hash against a numpy statement of its definition on rank layouts with random fields, and its
    sensitivity: one ulp in any single owned node (first / last plane, first / last node of a row, the node next to the
    pitch padding) or two nodes swapped changes it; ghost and padding nodes do not. Catches: an unhashed plane, row or
    row end, dropped mantissa bits, a hash that ignores the node's position, ghosts hashed as owned nodes."""
    R = Rank(key, 4)
    gen = torch.Generator().manual_seed(5)
    f = torch.randn(int(R.lay.total), dtype=torch.float64, generator=gen)
    base = _hash_ref(R, f.numpy())
    assert _hash_gpu(R, f.cuda()) == base
    nx, ny, nz = R.n
    owned = [(0, 0, 0), (nx - 1, ny - 1, nz - 1), (0, ny // 2, 0), (nx // 2, 0, nz - 1), (nx - 1, 0, nz // 2),
             (nx // 2, ny - 1, 1), (nx // 2, ny // 2, nz - 1)]
    seen = {base}
    for x, y, z in owned:
        g = f.clone()
        o = int(R.lay.off(x, y, z))
        g[o] = float(np.nextafter(g[o].item(), np.inf))
        h = _hash_gpu(R, g.cuda())
        assert h == _hash_ref(R, g.numpy()) and h not in seen, (x, y, z)
        seen.add(h)
    g = f.clone()
    a, b = int(R.lay.off(0, 0, 0)), int(R.lay.off(nx - 1, ny - 1, nz - 1))
    g[a], g[b] = f[b].item(), f[a].item()
    assert _hash_gpu(R, g.cuda()) == _hash_ref(R, g.numpy()) != base
    # ghosts (every side) and row padding are not hashed
    g = f.clone()
    own = np.zeros(R.shape, dtype=bool)
    R.nodes(own)[R.sl((0, nx, 0, ny, 0, nz))] = True
    g[torch.from_numpy(~own.reshape(-1))] = 12345.678
    assert _hash_gpu(R, g.cuda()) == base
