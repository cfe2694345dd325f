"""References for whole solves of hundreds of steps that share nothing with the solver's stencil code.

* ``closed_form_factor``: the discrete dispersion relation. The eigenmode phi = prod_d sin(pi x_d / L_d) is an
  eigenvector of -Delta_h with eigenvalue Lambda = sum_d (4 / h_d^2) sin^2(pi h_d / (2 L_d)), so leapfrog from u^0 = phi,
  u_t = 0 gives u^n = phi cos(n omega) with cos(omega) = 1 - tau^2 Lambda / 2, evaluated at 60 digits.
* ``longdouble_solve``: the leapfrog scheme written out with numpy slices in ``longdouble`` (64-bit mantissa on x86) on
  the dense (N+1)^3 grid, with point sources and receivers.
* ``bound``: the rounding bound every comparison of a float64 solve with these references uses.
* the shared long cases (``long_spec``, ``long_shot``, ``ricker16``): K = 203 steps at tau = 0.9 tau_max, the shot that
  the CPU and the GPU long-solve tests both run.

Nothing here imports the native extension, ``mpi_cuda_amd.ops`` or ``mpi_cuda_amd.models``' solvers; a spec is read through
its attributes ``N``, ``tau``, ``K`` and ``edges`` only.
"""
import collections
import functools

import numpy as np

EPS = 2.0 ** -52
K_LONG = 203
BOX = (1.0, 1.3, 0.7)
LD = np.longdouble


def bound(K, umax):
    """16 K^2 eps umax. A step makes about a dozen roundings of size eps umax per node (the three second differences,
    their sum, the coefficient product, 2u - u_prev, the final sum; the rounded coefficients themselves), taken as 16. A
    stable leapfrog answers one injected error e at step m with at most (n - m) e / sin(omega) at step n (the response of
    mode omega to a unit kick is sin((n - m) omega) / sin(omega)); at tau = 0.9 tau_max, cos(omega) >= 1 - 2 * 0.81, so
    1 / sin(omega) < 1.3 for the stiffest mode, and the slow modes' linear growth (n - m) is the envelope. Summed over the
    K steps that is K^2 / 2 of them; the factor 16 K^2 leaves the remaining factor 2 to the 1.3 and to the start step."""
    return 16.0 * float(K) ** 2 * EPS * float(umax)


# ---- the dispersion relation -------------------------------------------------------------------------------------------
def _mp():
    try:
        import mpmath
    except ImportError:
        return None
    return mpmath


def _decimal_pi_sin(D, x_over_pi_num, x_over_pi_den):
    """(pi, sin(pi num / den)) as Decimals in the current context: Machin's formula and the sine's Taylor series."""

    def atan_inv(q):  # atan(1 / q)
        q = D(q)
        term, total, k, q2 = 1 / q, 1 / q, 1, q * q
        while True:
            term = -term / q2
            add = term / (2 * k + 1)
            if add == 0 or abs(add) < D(10) ** -75:
                return total
            total += add
            k += 1

    pi = 4 * (4 * atan_inv(5) - atan_inv(239))
    x = pi * x_over_pi_num / x_over_pi_den
    term, total, k = x, x, 1
    while abs(term) > D(10) ** -75:
        term = -term * x * x / ((2 * k) * (2 * k + 1))
        total += term
        k += 1
    return pi, total


def _two_cos_omega(spec, use_mpmath=True):
    """2 cos(omega) = 2 - tau^2 Lambda at high precision, as an mpmath.mpf or a Decimal."""
    mp = _mp() if use_mpmath else None
    N = int(spec.N)
    if mp is not None:
        mp.mp.dps = 60
        s2 = mp.sin(mp.pi / (2 * N)) ** 2  # (h_d / L_d = 1 / N on every axis)
        lam = mp.fsum(4 * s2 / (mp.mpf(e) / N) ** 2 for e in spec.edges)
        return 2 - mp.mpf(spec.tau) ** 2 * lam
    import decimal

    with decimal.localcontext() as ctx:
        ctx.prec = 80
        D = decimal.Decimal
        _, s = _decimal_pi_sin(D, 1, 2 * N)
        lam = sum(4 * s * s / (D(float(e)) / N) ** 2 for e in spec.edges)
        return +(2 - D(float(spec.tau)) ** 2 * lam)


def closed_form_factor(spec, n, use_mpmath=True):
    """cos(n omega) of the eigenmode solve, cos(omega) = 1 - tau^2 Lambda / 2, for a cube or a box (``spec.edges``),
    computed at 60 digits or more and returned as a ``numpy.longdouble``: mpmath's cos(n acos(.)) if mpmath imports, else
    (or with ``use_mpmath=False``) the three-term recurrence T_{n+1} = (2 - tau^2 Lambda) T_n - T_{n-1}, T_0 = 1,
    T_1 = 1 - tau^2 Lambda / 2 in 80-digit ``decimal`` arithmetic."""
    return _factors(_SpecKey.of(spec), int(n), bool(use_mpmath and _mp() is not None))[int(n)]


_SpecKey = collections.namedtuple("_SpecKey", "N tau edges")
_SpecKey.of = staticmethod(lambda spec: _SpecKey(int(spec.N), float(spec.tau), tuple(float(e) for e in spec.edges)))


@functools.lru_cache(maxsize=None)
def _factors(key, n_max, use_mpmath):
    """cos(n omega) for n = 0..n_max (one evaluation serves every step of a log)."""
    c2 = _two_cos_omega(key, use_mpmath)
    if use_mpmath:
        mp = _mp()
        mp.mp.dps = 60
        omega = mp.acos(c2 / 2)
        return [LD(mp.nstr(mp.cos(k * omega), 30)) for k in range(n_max + 1)]
    import decimal

    with decimal.localcontext() as ctx:
        ctx.prec = 80
        t = [decimal.Decimal(1), c2 / 2]
        for _ in range(n_max):
            t.append(c2 * t[-1] - t[-2])
        return [LD(format(v, ".30e")) for v in t[:n_max + 1]]


def analytic_factor(spec, n):
    """cos(a_t n tau), a_t = pi sqrt(sum_d 1 / L_d^2): the time factor of the PDE's own solution, which the solver's
    printed errors are measured against; 60 digits (mpmath) or longdouble, returned as a longdouble."""
    mp = _mp()
    if mp is not None:
        mp.mp.dps = 60
        a_t = mp.pi * mp.sqrt(mp.fsum(1 / mp.mpf(e) ** 2 for e in spec.edges))
        return LD(mp.nstr(mp.cos(a_t * n * mp.mpf(spec.tau)), 30))
    a_t = LD(np.pi) * np.sqrt(sum(1 / LD(e) ** 2 for e in spec.edges))  # (pi to double: 1e-16 relative in the argument)
    return np.cos(a_t * n * LD(spec.tau))


def eigenmode(spec):
    """phi = prod_d sin(pi i_d / N) on the (N+1)^3 nodes in longdouble, exactly 0 on the six faces."""
    N = int(spec.N)
    s = np.sin(LD(np.arange(N + 1)) * (LD("3.14159265358979323846264338327950288") / N))
    s[0] = s[N] = 0
    return s[:, None, None] * s[None, :, None] * s[None, None, :]


# ---- the scheme in longdouble ------------------------------------------------------------------------------------------
LongSolve = collections.namedtuple("LongSolve", "uK uK1 traces umax")


def longdouble_solve(phi, psi, spec, K, sources=None, w=None, receivers=None):
    """Leapfrog for u_tt = Laplace(u) + sum_q w_q(t) delta(x - x_q), homogeneous Dirichlet walls, in ``longdouble``:

        Delta_h u = sum_d (u[+e_d] - 2 u + u[-e_d]) / h_d^2,   h_d = L_d / N        (interior nodes; faces stay 0)
        u^0 = phi,   u^1 = phi + tau psi + tau^2 / 2 Delta_h phi
        u^{n+1} = 2 u^n - u^{n-1} + tau^2 Delta_h u^n                                (n = 1 .. K - 1)

    Forcing, as csrc/src/cpu_solver.cpp (``CpuSolver::run`` / ``source_addend``) and ``Solver.set_sources`` define it:
    sample m of source q becomes the addend a^m_q = tau^2 w[m][q] / (h_x h_y h_z) (the delta is 1 / cell volume at the
    node); u^1 gets a^0 / 2 at the node after the first step, and u^{m+1} gets a^m after the step m -> m + 1, a node
    listed twice being added twice. ``phi`` / ``psi`` are (N+1)^3 arrays whose face values are ignored (None: zero),
    ``sources`` a (Q, 3) integer array, ``w`` (K, Q), ``receivers`` (R, 3).

    Returns ``LongSolve(uK, uK1, traces, umax)``: the last two levels as longdouble arrays, row n of ``traces`` = u^n at
    the receivers for n = 0..K ((K+1, R); None without receivers), and the largest |u| over all levels."""
    N, K = int(spec.N), int(K)
    tau = LD(spec.tau)
    h = [LD(e) / N for e in spec.edges]
    ih2 = [1 / (v * v) for v in h]
    inner = (slice(1, N),) * 3

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
        nxt[inner] = 2 * cur[inner] - prev[inner] + (tau * tau) * lap(cur)
        force(nxt, n, LD(1))
        if rec is not None:
            traces[n + 1] = nxt[rec[:, 0], rec[:, 1], rec[:, 2]]
        umax = max(umax, np.abs(nxt).max())
        prev, cur = cur, nxt
    return LongSolve(cur, prev, traces, float(umax))


def max_dev(got, want):
    """max |got - want| with the float64 result lifted to longdouble (the subtraction itself adds nothing)."""
    return float(np.abs(np.asarray(got, dtype=LD) - want).max())


# ---- the shared long cases ---------------------------------------------------------------------------------------------
def long_spec(N, box, K=K_LONG, check_every=1):
    """N intervals, cube or box 1 x 1.3 x 0.7, tau = 0.9 tau_max (tau_max = 1 / sqrt(sum_d 1 / h_d^2))."""
    from mpi_cuda_amd import ProblemSpec

    kw = dict(L=BOX[0], Ly=BOX[1], Lz=BOX[2]) if box else dict(L=1.0)
    tau_max = ProblemSpec(N=N, tau=1.0, K=K, **kw).tau_max
    return ProblemSpec(N=N, tau=0.9 * tau_max, K=K, check_every=check_every, **kw)


def ricker16(f0, t0, tau, K, amp=1.0):
    """K samples amp (1 - 2 a^2) exp(-a^2), a = pi f0 (m tau - t0), rounded to multiples of 2^-16: the last bits of exp do
    not reach the samples, so the native program that prints the fused tolerance's figures (csrc/tests/test_sources.cpp)
    builds the same numbers with its own exp, and the samples' sum is exact in any order (its check)."""
    t = np.arange(K) * tau - t0
    a = (np.pi * f0) * t
    return np.rint(amp * ((1.0 - 2.0 * (a * a)) * np.exp(-(a * a))) * 65536.0) / 65536.0


LongShot = collections.namedtuple("LongShot", "sources w receivers far arrival")


@functools.lru_cache(maxsize=None)
def long_shot(N, box, K=K_LONG):
    """Two Ricker sources and receivers from the source node to the far corner. N = 24: the sources sit two and three
    nodes from three walls; N = 40: around the grid's centre, on both sides of the rank faces at 20 of 4 slabs and of
    2x2x2 blocks. f0 = N / 10 and N / 8 (wavelengths of 10 and 8 nodes of h_x), t0 = 1.5 / f0: both wavelets have died
    out after 3 / f0 = 30 h_x <= 60 steps, well inside K. A disturbance moves one node of L1 distance per step, so the
    receiver ``far`` (column index) at L1 distance >= 56 from both sources is exactly 0.0 up to row ``arrival`` - 1 >= 56
    of its trace. Returns the node lists, w (K, 2), and those two numbers."""
    tau = long_spec(N, box, K).tau
    src, far_node = {24: ([[2, 3, 2], [3, 2, 4]], [22, 22, 22]), 40: ([[19, 20, 21], [21, 19, 20]], [39, 38, 39])}[N]
    src = np.array(src, dtype=np.int64)
    f0 = (N / 10.0, N / 8.0)
    w = np.stack([ricker16(f0[0], 1.5 / f0[0], tau, K, 1.0), ricker16(f0[1], 1.5 / f0[1], tau, K, -0.75)], axis=1)
    rec = np.array([src[0], src[0] + [1, 0, 0], src[1] + [0, -1, 2], [N // 2, N // 2, N // 2], [1, N // 2, N - 1],
                    [N - 1, N - 1, N - 1], [N // 2, N, N // 3], far_node, [N // 3, 2 * N // 3, N // 2]], dtype=np.int64)
    far = 7
    dist = int(np.abs(src - np.array(far_node)).sum(axis=1).min())
    first = int(np.nonzero(np.abs(w).sum(axis=1))[0][0])  # (the first non-zero sample: rounded-away tails are 0.0)
    assert dist > 50
    return LongShot(src, np.ascontiguousarray(w), rec, far, dist + 1 + first)


# printed by the native program for long_shot(40, box) (csrc/tests/test_sources.cpp check_split "long-cube" / "long-box";
# tests/test_sources_native.py compares them with its output): the rounding of the split identity on the CPU over 40
# passes of 5 steps and one of 2, and max |u| over the levels at every pass boundary (the shot's largest values occur
# while the wavelets fire; the two last levels alone are 15 times smaller)
D_SPLIT_LONG = {False: 5.7592819402429996e-16, True: 6.5225602696727947e-16}
UMAX_LONG = {False: 9.9821598569082859, True: 8.5848720945734058}


def tolerance_long(box):
    """sources_common.tolerance's rule for the long shot: max(8 d_split, 16 eps umax)."""
    return max(8.0 * D_SPLIT_LONG[box], 16.0 * EPS * UMAX_LONG[box])


def reciprocity_pair(N):
    """A next to a corner of the box (2, 3, 2 nodes from three walls), B off-centre in the interior."""
    return np.array([[2, 3, 2]], dtype=np.int64), np.array([[N // 2 + 3, N // 3, (2 * N) // 3]], dtype=np.int64)
