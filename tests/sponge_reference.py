"""The damped leapfrog of the sponge layers written out in numpy ``longdouble``, with point sources and receivers, and the
discrete energy of two levels. It shares no code with the solver: nothing here imports the native extension or
``mpi_cuda_amd``'s solvers; a spec is read through ``N``, ``tau`` and ``edges`` only, the sponge is the plain triple
``(width, sigma, faces)`` (``faces``: bits 0..5 = x-, x+, y-, y+, z-, z+).

    u_tt + 2 sigma(x) u_t = Laplace(u),  u_t centred in time:
    (1 + g) u^{n+1} = 2 u^n - (1 - g) u^{n-1} + tau^2 Delta_h u^n,   g = sigma(x) tau

    g at a node = the largest of its three 1-D values; for a node d nodes from a damped face of axis a, 1 <= d < W:
    g_a = (tau sigma_a) ((W - d) / W)^2, else 0;   default sigma_a = 3 ln(1000) / (2 W h_a)

The 1-D values are formed in float64 in the order the formula is written (they are the scheme's coefficients, data of
the problem like tau), everything after that in longdouble. Forcing is added after the damped step, as after the plain
one (``long_reference.longdouble_solve``).
"""
import collections
import math

import numpy as np

from long_reference import EPS, LD, bound  # noqa: F401  (re-exported for the tests)

SpongeSolve = collections.namedtuple("SpongeSolve", "uK uK1 traces umax u0 u1")


def sponge_g1d(spec, sponge):
    """The three 1-D tables g_a[0..N] in float64."""
    W, sigma, faces = int(sponge[0]), float(sponge[1]), int(sponge[2])
    N = int(spec.N)
    out = []
    for a in range(3):
        h = float(spec.edges[a]) / N
        sig = sigma if sigma > 0.0 else (3.0 * math.log(1000.0)) / ((2.0 * W) * h)
        ts = float(spec.tau) * sig
        g = np.zeros(N + 1)
        for i in range(1, N):
            for side in (0, 1):
                d = i if side == 0 else N - i
                if (faces >> (2 * a + side)) & 1 and d < W:
                    q = float(W - d) / float(W)
                    g[i] = max(g[i], ts * (q * q))
        out.append(g)
    return out


def sponge_g(spec, sponge):
    """g on the (N+1)^3 nodes (float64): the largest of the node's three 1-D values."""
    gx, gy, gz = sponge_g1d(spec, sponge)
    return np.maximum(np.maximum(gx[:, None, None], gy[None, :, None]), gz[None, None, :])


def damped_solve(phi, psi, spec, K, sponge=None, sources=None, w=None, receivers=None):
    """``long_reference.longdouble_solve`` with the damped step; ``sponge = None``: the undamped scheme (Dirichlet walls
    alone). Returns ``SpongeSolve(uK, uK1, traces, umax, u0, u1)``."""
    N, K = int(spec.N), int(K)
    tau = LD(spec.tau)
    h = [LD(e) / N for e in spec.edges]
    ih2 = [1 / (v * v) for v in h]
    inner = (slice(1, N),) * 3
    g = None if sponge is None else np.asarray(sponge_g(spec, sponge), dtype=LD)[inner]

    def lap(u):
        c = u[inner]
        return ((u[2:, 1:N, 1:N] - 2 * c + u[:N - 1, 1:N, 1:N]) * ih2[0]
                + (u[1:N, 2:, 1:N] - 2 * c + u[1:N, :N - 1, 1:N]) * ih2[1]
                + (u[1:N, 1:N, 2:] - 2 * c + u[1:N, 1:N, :N - 1]) * ih2[2])

    def interior(f):
        out = np.zeros((N + 1,) * 3, dtype=LD)
        if f is not None:
            out[inner] = np.asarray(f, dtype=LD).reshape((N + 1,) * 3)[inner]
        return out

    u0, v0 = interior(phi), interior(psi)
    u1 = np.zeros_like(u0)
    u1[inner] = u0[inner] + tau * v0[inner] + (tau * tau / 2) * lap(u0)
    src = None if sources is None or len(sources) == 0 else np.asarray(sources, dtype=np.int64).reshape(-1, 3)
    if src is not None:
        a = (tau * tau) * np.asarray(w, dtype=LD).reshape(K, len(src)) / (h[0] * h[1] * h[2])
        assert ((src >= 1) & (src <= N - 1)).all()

    def force(u, row, scale):
        if src is not None:
            for q, (i, j, k) in enumerate(src):
                u[i, j, k] += scale * a[row, q]

    force(u1, 0, LD(1) / 2)
    rec = None if receivers is None or len(receivers) == 0 else np.asarray(receivers, dtype=np.int64).reshape(-1, 3)
    traces = None
    if rec is not None:
        traces = np.zeros((K + 1, len(rec)), dtype=LD)
        traces[0] = u0[rec[:, 0], rec[:, 1], rec[:, 2]]
        traces[1] = u1[rec[:, 0], rec[:, 1], rec[:, 2]]
    umax = max(np.abs(u0).max(), np.abs(u1).max())
    prev, cur = u0, u1
    for n in range(1, K):
        nxt = np.zeros_like(cur)
        if g is None:
            nxt[inner] = 2 * cur[inner] - prev[inner] + (tau * tau) * lap(cur)
        else:
            nxt[inner] = (2 * cur[inner] - (1 - g) * prev[inner] + (tau * tau) * lap(cur)) / (1 + g)
        force(nxt, n, LD(1))
        if rec is not None:
            traces[n + 1] = nxt[rec[:, 0], rec[:, 1], rec[:, 2]]
        umax = max(umax, np.abs(nxt).max())
        prev, cur = cur, nxt
    return SpongeSolve(cur, prev, traces, float(umax), u0, u1)


Energy = collections.namedtuple("Energy", "E sens abs_terms")


def energy(a, b, spec):
    """E^{n+1/2} = V/2 [ sum ((b - a)/tau)^2 + sum_d h_d^-2 sum_edges (b_p - b_q)(a_p - a_q) ] of a = u^n, b = u^{n+1} in
    longdouble, every grid edge once. ``sens``: the first-order bound of |dE| per unit of max-norm error in each of a and
    b — V/2 [ sum 4 |b - a| / tau^2 + sum_d h_d^-2 sum_edges 2 (|b_p - b_q| + |a_p - a_q|) ] — and ``abs_terms`` = V/2 sum
    |terms|, the scale of a float64 summation's error."""
    N = int(spec.N)
    a = np.asarray(a, dtype=LD).reshape((N + 1,) * 3)
    b = np.asarray(b, dtype=LD).reshape((N + 1,) * 3)
    tau = LD(spec.tau)
    h = [LD(e) / N for e in spec.edges]
    half_v = h[0] * h[1] * h[2] / 2
    kin = ((b - a) / tau) ** 2
    tot, sens, ab = kin.sum(), (4 * np.abs(b - a) / (tau * tau)).sum(), kin.sum()
    for d in range(3):
        db, da = np.diff(b, axis=d), np.diff(a, axis=d)
        tot += (db * da).sum() / (h[d] * h[d])
        ab += np.abs(db * da).sum() / (h[d] * h[d])
        sens += (2 * (np.abs(db) + np.abs(da))).sum() / (h[d] * h[d])
    return Energy(half_v * tot, float(half_v * sens), float(half_v * ab))


def energy_tolerance(e, K, umax, depth):
    """What a float64 solve's energy may differ from the reference's ``e``: the rounding rule's field error 16 K^2 eps umax
    through ``e.sens``, plus the float64 evaluation of the sum itself (four roundings per term and ``depth`` additions on
    its longest path, each at most eps of the absolute terms)."""
    return bound(K, umax) * e.sens + (4 + depth) * EPS * e.abs_terms
