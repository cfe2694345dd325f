"""Reference for order-4 solves: the leapfrog scheme with the five-point fourth-order second difference per axis and the odd
reflection at the Dirichlet walls, written out with numpy slices in ``longdouble`` on an array padded by two nodes per side,
and the scheme's discrete dispersion relation.

Nothing here imports the native extension or the solver's stencil code; a spec is read through ``N``, ``tau``, ``K`` and
``edges`` only. ``coef`` and ``wall`` exist so that a test can show that a deliberately wrong operator (15 for 16, +centre
for -centre at the wall) lands far outside its bound."""
import numpy as np

from long_reference import BOX, LD


def order4_spec(N, box, K, check_every=1, frac=0.9):
    """tau = frac * (sqrt(3) / 2) * tau_max: ``frac`` of the fourth-order stability limit."""
    from mpi_cuda_amd.models.wave3d import ProblemSpec

    kw = dict(L=BOX[0], Ly=BOX[1], Lz=BOX[2]) if box else dict(L=1.0)
    tau_max = ProblemSpec(N=N, tau=1.0, K=K, **kw).tau_max
    return ProblemSpec(N=N, tau=frac * (np.sqrt(3.0) / 2.0) * tau_max, K=K, check_every=check_every, order=4, **kw)


def lap4(u, h, coef=16, wall=-1):
    """sum_d (-u[i-2] + coef u[i-1] - 30 u[i] + coef u[i+1] - u[i+2]) / (12 h_d^2) on the interior of a (N+1)^3 longdouble
    array whose faces hold 0; the nodes -1 and N + 1 are ``wall`` times the nodes 1 and N - 1 (odd reflection: -1), the
    nodes -2 and N + 2 are never used by an interior node."""
    N = u.shape[0] - 1
    e = np.zeros((N + 5,) * 3, dtype=LD)
    c = slice(2, N + 3)
    e[c, c, c] = u
    e[1, c, c], e[N + 3, c, c] = wall * u[1], wall * u[N - 1]
    e[c, 1, c], e[c, N + 3, c] = wall * u[:, 1], wall * u[:, N - 1]
    e[c, c, 1], e[c, c, N + 3] = wall * u[:, :, 1], wall * u[:, :, N - 1]
    i = slice(3, N + 2)  # the interior nodes 1 .. N - 1 in the padded array

    def sh(ax, k):
        s = [i, i, i]
        s[ax] = slice(3 + k, N + 2 + k)
        return e[tuple(s)]

    out = np.zeros((N - 1,) * 3, dtype=LD)
    for ax in range(3):
        out += (-sh(ax, -2) + coef * sh(ax, -1) - 30 * sh(ax, 0) + coef * sh(ax, 1) - sh(ax, 2)) / (12 * h[ax] * h[ax])
    return out


def order4_solve(phi, psi, spec, K, coef=16, wall=-1, levels=False):
    """u^1 = phi + tau psi + tau^2 / 2 D4 phi, u^{n+1} = 2 u^n - u^{n-1} + tau^2 D4 u^n in longdouble. Returns (u^K, u^{K-1},
    max |u| over the solve) and, with ``levels``, the list of all levels."""
    N = int(spec.N)
    tau = LD(spec.tau)
    h = [LD(ed) / N for ed in spec.edges]
    inner = (slice(1, N),) * 3

    def interior(f):
        out = np.zeros((N + 1,) * 3, dtype=LD)
        if f is not None:
            out[inner] = np.asarray(f, dtype=LD).reshape((N + 1,) * 3)[inner]
        return out

    u0, v0 = interior(phi), interior(psi)
    u1 = np.zeros_like(u0)
    u1[inner] = u0[inner] + tau * v0[inner] + (tau * tau / 2) * lap4(u0, h, coef, wall)
    umax = max(np.abs(u0).max(), np.abs(u1).max())
    prev, cur = u0, u1
    all_levels = [u0, u1]
    for _ in range(1, int(K)):
        nxt = np.zeros_like(cur)
        nxt[inner] = 2 * cur[inner] - prev[inner] + (tau * tau) * lap4(cur, h, coef, wall)
        umax = max(umax, np.abs(nxt).max())
        prev, cur = cur, nxt
        if levels:
            all_levels.append(cur)
    return (cur, prev, float(umax)) + ((all_levels,) if levels else ())


def eigenmode4(spec):
    """sin(pi i / N) sin(pi j / N) sin(pi k / N) in longdouble, faces exactly 0."""
    N = int(spec.N)
    s = np.sin(np.pi * np.arange(N + 1, dtype=LD) / N)
    s[0] = s[N] = 0
    return s[:, None, None] * s[None, :, None] * s[None, None, :]


def dispersion_factor(spec, n):
    """cos(omega_h n tau) with sin^2(omega_h tau / 2) = tau^2 / 4 sum_d (30 - 32 cos(pi / N) + 2 cos(2 pi / N)) / (12 h_d^2):
    the eigenmode of the scheme stays phi times this (odd reflection is exact for the sine mode)."""
    N = int(spec.N)
    tau = LD(spec.tau)
    th = LD(np.pi) if False else np.arccos(LD(-1)) / N
    sym = (30 - 32 * np.cos(th) + 2 * np.cos(2 * th)) / 12
    lam = sum(sym / (LD(ed) / N) ** 2 for ed in spec.edges)
    half = np.arcsin(np.sqrt(tau * tau / 4 * lam))
    return np.cos(2 * half * n)
