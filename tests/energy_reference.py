"""Plain numpy reference of the discrete energy sums of two stored levels on a rank layout, shared by
tests/test_energy_cpu.py (cpu_energy) and tests/test_gpu_energy_kernel.py (k_energy, k_energy_reduce).

Inputs. u^n, u^{n+1} ~ N(0, 1) on all (N + 1)³ nodes of the global grid, the global boundary nodes included (zeros there
would make every edge that leaves the grid 0·0 and hide the masks). `Case` cuts a rank's padded local arrays from them:
the neighbours' values in the ghosts one layer deep and inside the grid; NaN in every ghost outside the global grid, in
ghosts deeper than one layer and in the row padding. A mask that lets an outside edge through, or a read beyond the
one-layer contract that reaches a sum, gives NaN; a mask off by one the other way drops a term of typical size.

Terms. fp64 elementwise numpy in the documented operation order (cpu.hpp cpu_energy, k_energy's header):
    tk = ((b - a)·(1/τ))²,  tx = ((b_x+ - b)·(a_x+ - a))·ihx2 (ty, tz likewise),  node potential (tx + ty) + tz,
an edge kept when g + i + 1 <= N on its axis, over the owned nodes only. numpy does not contract and the native code is
built with -ffp-contract=off, so every term equals the native one bit for bit and only the summation order differs.

Sums. math.fsum (exactly rounded): kin* = Σ tk, pot* = Σ node potentials, A_k = Σ |tk|, A_p = Σ (|tx| + |ty| + |tz|).
A summation tree of depth D over terms t is off by at most D·u·Σ|t| to first order (u = 2⁻⁵³); with the project's slack
of 8 the tests allow (D + 8)·u·A_k on the kinetic and (D + 8)·u·A_p on the potential sum, each on its own. A_k and A_p
come from this reference, never from the code under test.
"""
import functools
import math

import numpy as np

from mpi_cuda_amd import ProblemSpec

U = 2.0 ** -53
BOX = (1.0, 1.3, 0.7)
# (N, dims, rank) as RANKS in tests/test_gpu_rank_pass.py, ghosts S = 5 deep by that file's rule (`ghost_depths`):
# all six neighbours; opposite corners with odd extents (c7 touches the three upper global faces); ny != nz; a slab rank
# between two others (xg = 5, yg = zg = 1)
RANKS = {"r13": (100, (3, 3, 3), 13), "c0": (67, (2, 2, 2), 0), "c7": (67, (2, 2, 2), 7), "b4": (70, (1, 2, 3), 4),
         "s1": (66, (3, 1, 1), 1)}
RANK_S = 5
# k_energy's launch geometry (kernels_initial.hip): 256 threads, one (row, pair) each, 8 planes per workgroup
WG_THREADS = 256
WG_PLANES = 8
WG_DEPTH = 1 + 8 + 6 + 3  # a pair's two nodes, 8 planes, 6 butterfly levels, 4 waves


def make_spec(N, box=False, K=20):
    kw = dict(Ly=BOX[1], Lz=BOX[2]) if box else {}
    return ProblemSpec(N=N, tau=0.5 * ProblemSpec(N=N, L=1.0, **kw).tau_max, K=K, L=1.0, **kw)


@functools.lru_cache(maxsize=4)
def global_fields(N):
    rng = np.random.default_rng(9000 + N)
    return rng.standard_normal((N + 1,) * 3), rng.standard_normal((N + 1,) * 3)


def ghost_depths(dims, S):
    """Ghost depths as make_rank_schedule sets them: S on x when x is split, on y / z when split on a block rank."""
    slab = dims[1] == 1 and dims[2] == 1
    return [S if dims[0] > 1 else 1, S if (not slab and dims[1] > 1) else 1, S if (not slab and dims[2] > 1) else 1]


def rank_layout(C, prob, dims, rank, S):
    return C.make_layout(prob, C.rank_box(prob, C.Dims(*dims), rank), 16, *ghost_depths(dims, S))


class Case:
    """One rank of a decomposition of the N grid (cube or BOX) with the global random fields cut to its layout."""

    def __init__(self, C, N, dims=(1, 1, 1), rank=0, S=1, box=False):
        self.N, self.dims, self.rank, self.box = N, dims, rank, box
        self.spec = make_spec(N, box)
        self.tau = self.spec.tau
        self.prob = self.spec.native()
        self.co = C.Coeffs.from_problem(self.prob)
        self.lay = l = rank_layout(C, self.prob, dims, rank, S)
        self.g = [int(l.xg), int(l.yg), int(l.zg)]
        self.n = [int(l.nx), int(l.ny), int(l.nz)]
        self.g0 = [int(l.gx0), int(l.gy0), int(l.gz0)]
        self.shape = (self.n[0] + 2 * self.g[0], self.n[1] + 2 * self.g[1], int(l.pitch))
        self.zc = self.g[2] + int(l.zs)  # column of local node z = 0
        assert int(l.total) == self.shape[0] * self.shape[1] * self.shape[2]
        # 1/h_d² on its own axis (what the box exposes): (N / L_d)² up to the few roundings of either evaluation
        edges = BOX if box else (1.0, 1.0, 1.0)
        self.ih2 = (self.co.ihx2, self.co.ihy2, self.co.ihz2)
        for v, L in zip(self.ih2, edges):
            assert abs(v - (N / L) ** 2) <= 8 * np.spacing((N / L) ** 2)
        ua, ub = global_fields(N)
        self.a, self.b = self.cut(ua), self.cut(ub)

    def what(self):
        return f"rank {self.rank} of {self.dims} N={self.N} {'box' if self.box else 'cube'} g={self.g} zc={self.zc}"

    def cut(self, glob, fill=np.nan):
        """Padded local array (flat) from a global (N+1)³ field: the owned nodes and the ghosts one layer deep that lie
        inside the global grid; `fill` everywhere else (deeper ghosts, outside the grid, row padding)."""
        idx, ok = [], []
        for a in range(3):
            i = np.arange(-self.g[a], self.n[a] + self.g[a])
            ok.append((i + self.g0[a] >= 0) & (i + self.g0[a] <= self.N) & (i >= -1) & (i < self.n[a] + 1))
            idx.append(np.clip(i + self.g0[a], 0, self.N))
        mask = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
        f = np.full(self.shape, fill)
        f[:, :, self.zc - self.g[2]: self.zc + self.n[2] + self.g[2]] = np.where(mask, glob[np.ix_(*idx)], fill)
        return f.reshape(-1)

    def view(self, f, dx=0, dy=0, dz=0):
        """The owned nodes of a padded flat array, shifted by (dx, dy, dz)."""
        g, n = self.g, self.n
        return f.reshape(self.shape)[g[0] + dx: g[0] + dx + n[0], g[1] + dy: g[1] + dy + n[1],
                                     self.zc + dz: self.zc + dz + n[2]]

    def edge_masks(self):
        """Per axis: the owned nodes whose edge to the upper neighbour stays inside the global grid."""
        return [np.arange(self.n[a]) + self.g0[a] + 1 <= self.N for a in range(3)]


def terms(case, a=None, b=None, masks=True):
    """The per-node terms tk, tx, ty, tz over the owned nodes (each an (nx, ny, nz) array)."""
    a = case.a if a is None else a
    b = case.b if b is None else b
    a0, b0 = case.view(a), case.view(b)
    inv_tau = 1.0 / case.tau
    v = (b0 - a0) * inv_tau
    out = {"tk": v * v}
    m = case.edge_masks()
    shape_of = [(-1, 1, 1), (1, -1, 1), (1, 1, -1)]
    with np.errstate(invalid="ignore"):
        for ax, name in enumerate(("tx", "ty", "tz")):
            d = [0, 0, 0]
            d[ax] = 1
            t = ((case.view(b, *d) - b0) * (case.view(a, *d) - a0)) * case.ih2[ax]
            out[name] = np.where(m[ax].reshape(shape_of[ax]), t, 0.0) if masks else t
    return out


def node_potential(t):
    return (t["tx"] + t["ty"]) + t["tz"]


def abs_potential(t):
    return (np.abs(t["tx"]) + np.abs(t["ty"])) + np.abs(t["tz"])


def fsum(x):
    return math.fsum(np.asarray(x).reshape(-1).tolist())


def sums(t):
    """(kin*, pot*, A_k, A_p), each exactly rounded."""
    return fsum(t["tk"]), fsum(node_potential(t)), fsum(np.abs(t["tk"])), fsum(abs_potential(t))


def workgroup_map(n, zc):
    """k_energy's thread -> node map per its header, for n = (nx, ny, nz) owned nodes and zc = zg + zs: the partial
    index [by·gx + bx] of every owned node, with by = x // 8 and bx = (y·npairs + (column // 2 - kp0)) // 256, pairs
    counted from kp0 = (zg + zs) // 2. Returns (index array of shape (nx, ny, nz), number of partials)."""
    nx, ny, nz = n
    kp0 = zc // 2
    npairs = (nz - 1 + zc) // 2 - kp0 + 1
    gx = -(-(ny * npairs) // WG_THREADS)
    gy = -(-nx // WG_PLANES)
    pair = (np.arange(nz) + zc) // 2 - kp0
    q = np.arange(ny)[:, None] * npairs + pair[None, :]
    wg = (np.arange(nx) // WG_PLANES)[:, None, None] * gx + (q // WG_THREADS)[None, :, :]
    return wg, gx * gy


def workgroup_sums(case, t):
    """Per workgroup: (kin*, pot*, A_k, A_p) as four arrays of length B, each entry exactly rounded."""
    wg, B = workgroup_map(case.n, case.zc)
    order = np.argsort(wg.reshape(-1), kind="stable")
    cuts = np.searchsorted(wg.reshape(-1)[order], np.arange(B + 1))
    out = []
    for arr in (t["tk"], node_potential(t), np.abs(t["tk"]), abs_potential(t)):
        flat = arr.reshape(-1)[order].tolist()
        out.append(np.array([math.fsum(flat[cuts[i]: cuts[i + 1]]) for i in range(B)]))
    return out, B


def check_sensitivity(case, t, pot, tol_p):
    """On the reference alone: what a missing mask or a dropped edge would do to pot*, against this case's tolerance.

    * Masks omitted, zeros in place of the NaNs: every edge that leaves the global grid then contributes a·b/h² instead
      of 0. On a layout with such edges the sum must move by more than 100·tol_p; a layout that touches no upper global
      face has none (its three masks are all true), and there the sum must not move at all.
    * One single edge left out, per axis the last edge that stays inside the grid (the one a mask off by one would
      drop), at the middle of the other two axes: the sum must move by more than 100·tol_p.
    """
    ua, ub = global_fields(case.N)
    loose = terms(case, case.cut(ua, 0.0), case.cut(ub, 0.0), masks=False)
    assert all(np.isfinite(loose[k]).all() for k in loose)
    moved = abs(fsum(node_potential(loose)) - pot)
    m = case.edge_masks()
    outside = sum(int((~m[a]).sum()) for a in range(3))
    assert outside == sum(1 for a in range(3) if case.g0[a] + case.n[a] == case.N + 1)
    if outside:
        assert moved > 100 * tol_p, (case.what(), moved, tol_p)
    else:
        assert moved == 0.0, (case.what(), moved)
    mid = [n // 2 for n in case.n]
    for ax, name in enumerate(("tx", "ty", "tz")):
        at = list(mid)
        at[ax] = int(np.nonzero(m[ax])[0][-1])
        one = {k: v for k, v in t.items()}
        one[name] = t[name].copy()
        assert one[name][tuple(at)] != 0.0
        one[name][tuple(at)] = 0.0
        moved = abs(fsum(node_potential(one)) - pot)
        assert moved > 100 * tol_p, (case.what(), name, at, moved, tol_p)
