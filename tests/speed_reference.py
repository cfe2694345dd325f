"""Reference for solves with a variable wave speed, u_tt = c(x)^2 Laplace(u): the leapfrog scheme written out with numpy
slices in ``longdouble`` with a per-node c^2, the sponge update, sources and receivers, and the weighted discrete energy.

Nothing here imports the native extension or the solver's stencil code; a spec is read through ``N``, ``tau``, ``K`` and
``edges`` only. The media of the tests (``two_layer``, ``random_medium``) live here too, so that the CPU and the GPU tests
solve the same problems."""
import collections

import numpy as np

from long_reference import LD

SpeedSolve = collections.namedtuple("SpeedSolve", "uK uK1 traces umax e_start e_end")


def two_layer(N):
    """c = 1 for x-index < split, 2 from there on; the split plane is not a symmetry plane of the grid."""
    c = np.ones((N + 1,) * 3)
    c[(2 * N) // 5 + 1:] = 2.0
    return c


def random_medium(N, seed=7):
    """Seeded, c in [0.5, 2] per node."""
    return np.random.default_rng(seed).uniform(0.5, 2.0, (N + 1,) * 3)


def sponge_g(spec, width, sigma, faces=63):
    """g = sigma_a tau ((W - d) / W)^2 for a node d < W nodes from a damped face of axis a, the largest over the axes, in
    longdouble; sigma <= 0 selects 3 ln(1000) / (2 W h_a) (problem.hpp sponge_tables' profile, stated again)."""
    N = int(spec.N)
    g = np.zeros((N + 1,) * 3, dtype=LD)
    i = np.arange(N + 1)
    for a in range(3):
        h = LD(spec.edges[a]) / N
        sg = LD(sigma) if sigma > 0 else 3 * np.log(LD(1000)) / (2 * width * h)
        t = np.zeros(N + 1, dtype=LD)
        for side in range(2):
            if not (faces >> (2 * a + side)) & 1:
                continue
            d = i if side == 0 else N - i
            q = (LD(width) - d) / LD(width)
            t = np.maximum(t, np.where((d >= 1) & (d < width), LD(spec.tau) * sg * q * q, 0))
        t[0] = t[N] = 0
        shape = [1, 1, 1]
        shape[a] = N + 1
        g = np.maximum(g, t.reshape(shape))
    return g


def weighted_energy(a, b, c, spec):
    """E = V / 2 [ sum ((b - a) / tau)^2 / c^2 + sum_d h_d^-2 sum_edges (b_p - b_q)(a_p - a_q) ] in longdouble."""
    N = int(spec.N)
    h = [LD(e) / N for e in spec.edges]
    inner = (slice(1, N),) * 3
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    v = (b[inner] - a[inner]) / LD(spec.tau)
    kin = (v * v / (np.asarray(c, dtype=LD)[inner] ** 2)).sum()
    pot = LD(0)
    for d in range(3):
        pot += (np.diff(b, axis=d) * np.diff(a, axis=d)).sum() / (h[d] * h[d])
    return float((h[0] * h[1] * h[2]) / 2 * (kin + pot))


def speed_solve(phi, psi, c, spec, K, sources=None, w=None, receivers=None, sponge=None):
    """Leapfrog for u_tt = c^2 Laplace(u) + sum_q w_q(t) delta(x - x_q) (+ sponge layers), Dirichlet walls, longdouble:

        u^1 = phi + tau psi + c^2 tau^2 / 2 Delta_h phi
        w   = 2 u^n - u^{n-1} + c^2 tau^2 Delta_h u^n;   u^{n+1} = (w + g u^{n-1}) / (1 + g)   (g = 0 without a sponge)

    The forcing is not multiplied by c^2: a^m = tau^2 w[m] / (h_x h_y h_z), half of a^0 on u^1. ``sponge`` = (width,
    sigma, faces). Returns the last two levels, the traces, max |u| and the weighted energies E^{1/2}, E^{K-1/2}."""
    N, K = int(spec.N), int(K)
    tau = LD(spec.tau)
    h = [LD(e) / N for e in spec.edges]
    ih2 = [1 / (v * v) for v in h]
    inner = (slice(1, N),) * 3
    c2 = (np.asarray(c, dtype=LD).reshape((N + 1,) * 3) ** 2)[inner]
    g = None if sponge is None else sponge_g(spec, *sponge)[inner]

    def lap(u):
        m = u[inner]
        return ((u[2:, 1:N, 1:N] - 2 * m + u[:N - 1, 1:N, 1:N]) * ih2[0]
                + (u[1:N, 2:, 1:N] - 2 * m + u[1:N, :N - 1, 1:N]) * ih2[1]
                + (u[1:N, 1:N, 2:] - 2 * m + u[1:N, 1:N, :N - 1]) * ih2[2])

    def interior(f):
        out = np.zeros((N + 1,) * 3, dtype=LD)
        if f is not None:
            out[inner] = np.asarray(f, dtype=LD).reshape((N + 1,) * 3)[inner]
        return out

    u0, v0 = interior(phi), interior(psi)
    u1 = np.zeros_like(u0)
    u1[inner] = u0[inner] + tau * v0[inner] + c2 * (tau * tau / 2) * lap(u0)
    src = None if sources is None or len(sources) == 0 else np.asarray(sources, dtype=np.int64).reshape(-1, 3)
    if src is not None:
        a = (tau * tau) * np.asarray(w, dtype=LD).reshape(K, len(src)) / (h[0] * h[1] * h[2])

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
    e_start = weighted_energy(u0, u1, c, spec)
    prev, cur = u0, u1
    for n in range(1, K):
        nxt = np.zeros_like(cur)
        nxt[inner] = 2 * cur[inner] - prev[inner] + c2 * (tau * tau) * lap(cur)
        if g is not None:
            nxt[inner] = (nxt[inner] + g * prev[inner]) / (1 + g)
        force(nxt, n, LD(1))
        if rec is not None:
            traces[n + 1] = nxt[rec[:, 0], rec[:, 1], rec[:, 2]]
        umax = max(umax, np.abs(nxt).max())
        prev, cur = cur, nxt
    return SpeedSolve(cur, prev, traces, float(umax), e_start, weighted_energy(prev, cur, c, spec))
