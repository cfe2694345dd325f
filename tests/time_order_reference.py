"""Reference for time_order = 4 solves: the modified-equation scheme

    u^{n+1} = 2 u^n - u^{n-1} + tau^2 L u^n + tau^4 / 12 L (L u^n),
    u^1     = phi + tau^2 / 2 L phi + tau^4 / 24 L (L phi) + tau (psi + tau^2 / 6 L psi),

L the fourth-order Laplacian with the odd reflection at the Dirichlet walls, written with numpy slices in ``longdouble``:
L is applied to a dense (N+1)^3 array, the result is put into a second dense array with zero faces, and L is applied to
that array again. The closed forms of the scheme for the eigenmode are here too.

Nothing here imports the native extension or the solver's stencil code; a spec is read through ``N``, ``tau``, ``K`` and
``edges`` only. ``c4``, ``reflect_v`` and ``psi3`` exist so that a test can show that a deliberately wrong scheme (tau^4 / 24
for tau^4 / 12 in the step, L u not reflected at the walls in the second application, the psi term without its
tau^3 / 6 part) lands far outside its bound."""
import numpy as np

from long_reference import BOX, LD
from order4_reference import lap4


def time_order_spec(N, box, K, check_every=1, frac=0.9, time_order=4):
    """tau = frac of the scheme's stability limit: 3/2 tau_max for time order 4, sqrt(3)/2 tau_max for (4, 2)."""
    from mpi_cuda_amd.models.wave3d import ProblemSpec

    kw = dict(L=BOX[0], Ly=BOX[1], Lz=BOX[2]) if box else dict(L=1.0)
    tau_max = ProblemSpec(N=N, tau=1.0, K=K, **kw).tau_max
    lim = 1.5 if time_order == 4 else np.sqrt(3.0) / 2.0
    return ProblemSpec(N=N, tau=frac * lim * tau_max, K=K, check_every=check_every, order=4, time_order=time_order, **kw)


def _dense(N, interior_values):
    out = np.zeros((N + 1,) * 3, dtype=LD)
    out[1:N, 1:N, 1:N] = interior_values
    return out


def lap_twice(u, h, reflect_v=True):
    """(L u, L L u) on the interior. The second application sees L u as a grid function with zero faces whose value
    beyond a wall is minus its mirror value (``reflect_v``; False: zero there, the mutation)."""
    N = u.shape[0] - 1
    a = lap4(u, h)
    return a, lap4(_dense(N, a), h, wall=-1 if reflect_v else 0)


def time_order_solve(phi, psi, spec, K, c4=12, reflect_v=True, psi3=True):
    """Returns (u^K, u^{K-1}, max |u| over the solve) in longdouble."""
    N = int(spec.N)
    tau = LD(spec.tau)
    h = [LD(ed) / N for ed in spec.edges]
    inner = (slice(1, N),) * 3

    def interior(f):
        out = np.zeros((N + 1,) * 3, dtype=LD)
        if f is not None:
            out[inner] = np.asarray(f, dtype=LD).reshape((N + 1,) * 3)[inner]
        return out

    u0 = interior(phi)
    a, b = lap_twice(u0, h, reflect_v)
    u1 = np.zeros_like(u0)
    u1[inner] = u0[inner] + (tau**2 / 2) * a + (tau**4 / 24) * b
    if psi is not None:
        v0 = interior(psi)
        q = v0[inner] + ((tau**2 / 6) * lap4(v0, h) if psi3 else 0)
        u1[inner] += tau * q
    umax = max(np.abs(u0).max(), np.abs(u1).max())
    prev, cur = u0, u1
    for _ in range(1, int(K)):
        a, b = lap_twice(cur, h, reflect_v)
        nxt = np.zeros_like(cur)
        nxt[inner] = 2 * cur[inner] - prev[inner] + tau**2 * a + (tau**4 / c4) * b
        umax = max(umax, np.abs(nxt).max())
        prev, cur = cur, nxt
    return cur, prev, float(umax)


def z_of(spec):
    """z = tau^2 lambda_h of the eigenmode (1, 1, 1): lambda_h = sum_d (30 - 32 cos(pi / N) + 2 cos(2 pi / N)) / (12 h_d^2)."""
    N = int(spec.N)
    th = np.arccos(LD(-1)) / N
    sym = (30 - 32 * np.cos(th) + 2 * np.cos(2 * th)) / 12
    return LD(spec.tau) ** 2 * sum(sym / (LD(ed) / N) ** 2 for ed in spec.edges)


def first_step_factor(spec):
    """u^1 = (1 - z / 2 + z^2 / 24) phi for the eigenmode and psi = 0."""
    z = z_of(spec)
    return 1 - z / 2 + z * z / 24


def dispersion_factor(spec, n, time_order=4):
    """cos(n omega_h tau): 2 cos(omega_h tau) = 2 - z + z^2 / 12 (time order 4) or 2 - z (time order 2). The eigenmode of
    the scheme stays phi times this, the first step's factor being the same cosine."""
    z = z_of(spec)
    c = 1 - z / 2 + (z * z / 24 if time_order == 4 else 0)
    return np.cos(n * np.arccos(c))


def closed_form_error(spec, n, time_order=4):
    """max over the grid of |u^n - u_a(t_n)| for the eigenmode with max |phi| = 1 (N even): |cos(n omega_h tau) -
    cos(a_t n tau)|."""
    a_t = np.arccos(LD(-1)) * np.sqrt(sum(1 / LD(ed) ** 2 for ed in spec.edges))
    return abs(dispersion_factor(spec, n, time_order) - np.cos(a_t * (n * LD(spec.tau))))


def joint_refinement_spec(N, time_order, T=0.5, frac=0.9):
    """The fewest steps K that reach T with tau = T / K <= frac of the scheme's limit, on the unit cube."""
    from mpi_cuda_amd.models.wave3d import ProblemSpec

    lim = (1.5 if time_order == 4 else np.sqrt(3.0) / 2.0) * ProblemSpec(N=N).tau_max
    K = int(np.ceil(T / (frac * lim)))
    return ProblemSpec(N=N, tau=T / K, K=K, check_every=1, order=4, time_order=time_order)
