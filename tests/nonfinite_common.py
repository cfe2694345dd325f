"""Shared by the non-finite tests: a numpy statement of the error check that shares no code with stencil.hpp, the plant
values and positions, and the comparisons that hold where NaN is expected.

The contract (docs/ARCHITECTURE.md, "Non-finite fields"): the maximum is taken over the nodes whose error is not NaN (0
if there are none; +Inf is an ordinary value of it), the sum of squares carries every NaN and every overflow, and a
step is finite iff both are.

The check, as the kernels and the CPU path evaluate it: e = |u - ((s_x * s_y) * ct) * s_z| with plain products in that
order, which numpy reproduces bit for bit (each product and the difference are single IEEE operations).

  * expected maximum = np.fmax.reduce(e, initial=0.0): fmax drops NaN, and a maximum is exact in any order.
  * expected sum of squares: sum of e * e in longdouble (64-bit mantissa), non-finite terms included.

Bound of a finite float64 sum against it, `sum_bound`: 2 n 2^-53 sum e^2 for n nodes. The terms e_i^2 are non-negative.
Each accumulation step acc' = fma(e, e, acc) rounds the exact e^2 + acc once, so it is one rounded addition of exact
terms (the squares themselves are not rounded); adding two partial sums is one rounded addition too. Any summation tree
over n terms then makes n - 1 rounded additions, and with non-negative terms every intermediate value is at most the
full sum, so the result errs by at most ((1 + u)^(n-1) - 1) sum <= 1.06 (n - 1) u sum for n u < 0.01, u = 2^-53; the
longdouble reference (u' = 2^-64, squares rounded once more) adds less than n u' sum. Together below 2 n u sum.
"""
import math

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
PLANTS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf"), "1e200": 1e200, "3.0": 3.0}


def ref_error(u, sx, sy, sz, ct):
    """(max, sum of squares as longdouble, n) of the check over a dense block u[x, y, z] with the sine factors of its
    nodes along the three axes."""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(all="ignore"):
        row = (np.asarray(sx)[:, None] * np.asarray(sy)[None, :]) * ct
        e = np.abs(u - row[:, :, None] * np.asarray(sz)[None, None, :])
        mx = float(np.fmax.reduce(e.reshape(-1), initial=0.0))
        el = e.astype(LD)
        sm = (el * el).sum(dtype=LD)
    return mx, sm, e.size


def ref_error_box(lay, u_flat, box, s_ext, ct):
    """The same over local box `box` of a padded flat field in layout `lay` (s_ext[g + 1] = the sine at global node g)."""
    from mpi_cuda_amd.ops.stencil import grid_view
    import torch

    g = grid_view(lay, torch.as_tensor(u_flat)).numpy()  # index i = local node i - 1
    s = np.asarray(s_ext, dtype=np.float64)
    blk = g[box.x0 + 1:box.x1 + 1, box.y0 + 1:box.y1 + 1, box.z0 + 1:box.z1 + 1]
    sx = s[int(lay.gx0) + box.x0 + 1:int(lay.gx0) + box.x1 + 1]
    sy = s[int(lay.gy0) + box.y0 + 1:int(lay.gy0) + box.y1 + 1]
    sz = s[int(lay.gz0) + box.z0 + 1:int(lay.gz0) + box.z1 + 1]
    return ref_error(blk, sx, sy, sz, ct)


def klass(v):
    """'nan', '+inf', '-inf' or 'finite', of the value as a float64: a longdouble sum above DBL_MAX is '+inf', which is
    what the contract says of a float64 sum whose terms overflow."""
    v = float(v)
    if math.isnan(v):
        return "nan"
    if math.isinf(v):
        return "+inf" if v > 0 else "-inf"
    return "finite"


def sum_bound(n, total):
    return 2.0 * n * U * float(total)


def assert_pair_matches_ref(got, ref, what=""):
    """A reduced (max, sum) against ref_error's triple: the maximum bit-equal and never NaN, the sum of the reference's
    class and, where finite, within sum_bound."""
    mx, sm, n = ref
    assert not math.isnan(got[0]), (what, got)
    assert np.float64(got[0]).view(np.int64) == np.float64(mx).view(np.int64), (what, got[0], mx)
    assert klass(got[1]) == klass(sm), (what, got[1], sm)
    if klass(sm) == "finite":
        assert abs(LD(got[1]) - sm) <= sum_bound(n, sm), (what, got[1], float(sm), sum_bound(n, sm))


def assert_pair_same_class(got, want, what="", rel_tol=1e-12):
    """A reduced GPU (max, sum) against the CPU's: the maximum bit-equal and not NaN, the sum of the same class and,
    where finite, within the suite's summation-order tolerance."""
    assert not math.isnan(got[0]) and not math.isnan(want[0]), (what, got, want)
    assert np.float64(got[0]).view(np.int64) == np.float64(want[0]).view(np.int64), (what, got, want)
    assert klass(got[1]) == klass(want[1]), (what, got, want)
    if klass(want[1]) == "finite":
        assert math.isclose(got[1], want[1], rel_tol=rel_tol), (what, got, want)


def same_class_bits(a, b):
    """The NaN masks are equal and the bits are equal everywhere else (CPU and GPU NaNs differ in sign and payload)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~na])


def positions(box, seed=0):
    """Nodes (x, y, z) of the box (x0, x1, y0, y1, z0, z1), half-open: its 8 corners, the node next to each corner along
    z inside the box, the middle of its 6 faces, and 10 seeded random interior nodes. Pure integer arithmetic; duplicates
    removed, order kept."""
    x0, x1, y0, y1, z0, z1 = box
    xs, ys, zs = (x0, x1 - 1), (y0, y1 - 1), (z0, z1 - 1)
    out = [(x, y, z) for x in xs for y in ys for z in zs]
    # the node after the low corner and the node before the high corner along z: with the corner itself, both halves of
    # the first and of the last 16-byte pair, on even and odd z extents
    out += [(x, y, z) for x in xs for y in ys for z in (z0 + 1, z1 - 2) if z0 <= z < z1]
    mx, my, mz = (x0 + x1 - 1) // 2, (y0 + y1 - 1) // 2, (z0 + z1 - 1) // 2
    out += [(x0, my, mz), (x1 - 1, my, mz), (mx, y0, mz), (mx, y1 - 1, mz), (mx, my, z0), (mx, my, z1 - 1)]
    s = 0x2545F4914F6CDD1D ^ (seed * 0x9E3779B97F4A7C15 & ((1 << 64) - 1))
    for _ in range(10):
        p = []
        for lo, hi in ((x0, x1), (y0, y1), (z0, z1)):
            s = (s * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
            p.append(lo + 1 + (s >> 33) % max(hi - lo - 2, 1) if hi - lo > 2 else lo)
        out.append(tuple(p))
    seen, uniq = set(), []
    for p in out:
        if p not in seen:
            seen.add(p)
            uniq.append(p)
    return uniq


# ---- whole solves that blow up -------------------------------------------------------------------------------------------
N_BLOW = 24
OVERFLOW = {"10x": (10.0, 160), "3x": (3.0, 260)}  # tau / tau_max, K


def blowup_spec(key):
    """N = 24, tau = 10 (3) tau_max, K = 160 (260), every step checked: run with force=True from lcg_fields(24)."""
    from mpi_cuda_amd import ProblemSpec

    f, K = OVERFLOW[key]
    tau_max = ProblemSpec(N=N_BLOW, tau=1.0, K=K).tau_max
    return ProblemSpec(N=N_BLOW, tau=f * tau_max, K=K, check_every=1)


def assert_overflow_phases(r, N=N_BLOW):
    """The four phases of a genuine overflow in an error log: the sum of squares becomes Inf while the maximum is
    finite, the maximum becomes Inf, the sum becomes NaN, and the maximum — never NaN — ends at 0.0 (every node NaN).
    The largest finite sum lies below DBL_MAX / 2: summation order moves a sum by about 1e-12 relative and cannot carry
    it across that gap, so every backend overflows at the same step. Returns the first steps of the three events."""
    import sys

    st, mx, rms = np.array(r.steps), np.array(r.max_err), np.array(r.rms_err)
    assert r.finite is False and not np.isnan(mx).any()
    sum_inf, max_inf, sum_nan = np.isposinf(rms), np.isposinf(mx), np.isnan(rms)
    assert sum_inf.any() and max_inf.any() and sum_nan.any()
    first = int(st[sum_inf][0]), int(st[max_inf][0]), int(st[sum_nan][0])
    assert first[0] < first[1] < first[2], first
    assert np.isfinite(mx[st < first[1]]).all() and np.isfinite(rms[st < first[0]]).all()
    assert mx[-1] == 0.0 and sum_nan[-1]
    # once a step is non-finite, every later checked step is
    bad = ~(np.isfinite(mx) & np.isfinite(rms))
    assert bad[np.argmax(bad):].all()
    with np.errstate(over="ignore"):
        largest = float((rms[np.isfinite(rms)].astype(LD) ** 2).max() * (N - 1) ** 3)
    assert largest < sys.float_info.max / 2, largest
    return first


def assert_log_same_class(r, want, what="", rel_tol=1e-12):
    """An error log against CpuSolver's: the same steps, finite False, maxima bit-equal (never NaN), the rms column of the
    same class at every step and within rel_tol where finite."""
    assert r.steps == want.steps, what
    assert r.finite is False and want.finite is False, what
    assert not np.isnan(np.array(want.max_err)).any(), what
    assert same_class_bits(r.max_err, want.max_err) and not np.isnan(np.array(r.max_err)).any(), (what, r.max_err, want.max_err)
    for n, a, b in zip(r.steps, r.rms_err, want.rms_err):
        assert klass(a) == klass(b), (what, n, a, b)
        if klass(b) == "finite":
            assert math.isclose(a, b, rel_tol=rel_tol), (what, n, a, b)


def first_nonfinite_step(r):
    for n, m, e in zip(r.steps, r.max_err, r.rms_err):
        if not (math.isfinite(m) and math.isfinite(e)):
            return n
    return None


def save_initial(prefix, spec, phi, psi):
    """PREFIX.phi / PREFIX.psi dumps for the CLIs' --initial."""
    from mpi_cuda_amd.utils import dump as dumpio

    for part, f in (("phi", phi), ("psi", psi)):
        dumpio.save(f"{prefix}.{part}", f, N=spec.N, L=spec.edges[0], tau=spec.tau, step=0, box=spec.edges)
