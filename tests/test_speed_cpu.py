"""CpuSolver with a speed field c(x) over K = 203 steps at tau = 0.9 tau_max / c_max (N = 24 cube, N = 40 box 1 x 1.3 x
0.7; a two-layer medium c = 1 | 2 split at a non-symmetric plane, and a seeded random medium c in [0.5, 2]) against the
numpy longdouble leapfrog of tests/speed_reference.py, which shares no code with the solver. Every deviation is held to
long_reference.bound = 16 K^2 eps umax; the weighted energy to K 64 eps, as the constant-speed energy test. Plus the two
exact identities of the scheme (c = 1: the speedless bits; c = 2 at tau: the bits of c = 1 at 2 tau) and the refusals."""
import dataclasses
import functools

import numpy as np
import pytest

from long_reference import BOX, EPS, K_LONG, bound, long_shot, max_dev
from sources_common import lcg_fields, same_bits
from speed_reference import random_medium, speed_solve, two_layer

from mpi_cuda_amd import ProblemSpec
from mpi_cuda_amd.solver import Solver

K = K_LONG
MEDIA = {"layers": two_layer, "random": random_medium}
CASES = [pytest.param(N, box, m, id=f"N{N}-{'box' if box else 'cube'}-{m}") for N, box in ((24, False), (40, True))
         for m in MEDIA]


def speed_spec(N, box, cmax, K_=K, frac=0.9, check_every=1):
    kw = dict(L=BOX[0], Ly=BOX[1], Lz=BOX[2]) if box else dict(L=1.0)
    tau_max = ProblemSpec(N=N, tau=1.0, K=K_, **kw).tau_max
    return ProblemSpec(N=N, tau=frac * tau_max / cmax, K=K_, check_every=check_every, **kw)


def _held(what, dev, bnd):
    print(f"SPEED {what}: max deviation {dev:.3e} bound {bnd:.3e} ratio {dev / bnd:.2e}")
    assert dev <= bnd, (what, dev, bnd)


def _fields(s):
    return s.global_field(0).numpy(), s.global_field(1).numpy()


@functools.lru_cache(maxsize=None)
def _reference(N, box, medium):
    c = MEDIA[medium](N)
    spec = speed_spec(N, box, 2.0)
    phi, psi = lcg_fields(N)
    rec = long_shot(N, box).receivers
    return c, spec, phi, psi, rec, speed_solve(phi, psi, c, spec, K, receivers=rec)


@pytest.mark.parametrize("N,box,medium", CASES)
def test_reference_alone_stays_inside_the_bound(N, box, medium):
    """Before the bound is relied on: the reference's own float64 rendering (the same numpy slices in float64) stays inside
    it against the longdouble one, so the bound is not below what a correct float64 leapfrog of this medium does."""
    c, spec, phi, psi, rec, ref = _reference(N, box, medium)
    import speed_reference as sr

    saved = sr.LD
    sr.LD = np.float64
    try:
        f64 = speed_solve(phi, psi, c, spec, K, receivers=rec)
    finally:
        sr.LD = saved
    _held(f"reference float64 {medium} N={N} u^K", max_dev(f64.uK, ref.uK), bound(K, ref.umax))
    _held(f"reference float64 {medium} N={N} traces", max_dev(f64.traces, ref.traces), bound(K, ref.umax))


@pytest.mark.parametrize("N,box,medium", CASES)
def test_random_data_against_longdouble(N, box, medium):
    """Random phi, psi: u^K, u^{K-1} and the traces. A coefficient taken from a neighbouring node, c instead of c^2, a
    first step with the constant coefficient or a medium transposed lands orders of magnitude outside."""
    c, spec, phi, psi, rec, ref = _reference(N, box, medium)
    s = Solver(spec, backend="cpu", speed=c)
    s.set_initial(phi, psi)
    s.set_receivers(rec)
    s.run()
    uK, uK1 = _fields(s)
    b = bound(K, ref.umax)
    _held(f"{medium} N={N} box={box} u^K", max_dev(uK, ref.uK), b)
    _held(f"{medium} N={N} box={box} u^K-1", max_dev(uK1, ref.uK1), b)
    _held(f"{medium} N={N} box={box} traces", max_dev(s.traces().numpy(), ref.traces), b)
    # weighted energy: conserved to K 64 eps, relative; and equal to the reference's
    e0, e1 = s.energy(1), s.energy(0)
    drift = abs(e1 - e0) / e0
    print(f"SPEED {medium} N={N} energy drift {drift:.3e} bound {K * 64 * EPS:.3e}")
    assert drift <= K * 64 * EPS
    assert abs(e0 - ref.e_start) <= K * 64 * EPS * e0 and abs(e1 - ref.e_end) <= K * 64 * EPS * e0
    # (the longdouble reference conserves its own weighted energy too: the weight 1/c^2 is the right one)
    assert abs(ref.e_end - ref.e_start) <= K * 64 * EPS * ref.e_start


@pytest.mark.parametrize("N,box,medium", CASES)
def test_shot_against_longdouble(N, box, medium):
    """Two Ricker sources, receivers, zero start: the forcing is not multiplied by c^2."""
    c = MEDIA[medium](N)
    spec = speed_spec(N, box, 2.0)
    shot = long_shot(N, box)
    w = shot.w  # (its samples depend on long_spec's tau; here they are just K x 2 finite numbers)
    zero = np.zeros((N + 1,) * 3)
    ref = speed_solve(zero, None, c, spec, K, sources=shot.sources, w=w, receivers=shot.receivers)
    s = Solver(spec, backend="cpu", speed=c)
    s.set_initial(zero)
    s.set_sources(shot.sources, w)
    s.set_receivers(shot.receivers)
    s.run()
    b = bound(K, ref.umax)
    _held(f"shot {medium} N={N} u^K", max_dev(_fields(s)[0], ref.uK), b)
    _held(f"shot {medium} N={N} traces", max_dev(s.traces().numpy(), ref.traces), b)
    assert ref.umax > 0


@pytest.mark.parametrize("N,box", [(24, False), (40, True)])
def test_sponge_against_longdouble(N, box):
    c = two_layer(N)
    W = 6
    spec = dataclasses.replace(speed_spec(N, box, 2.0), sponge=(W, 0.0, 63))
    phi, psi = lcg_fields(N)
    ref = speed_solve(phi, psi, c, spec, K, sponge=(W, 0.0, 63))
    s = Solver(spec, backend="cpu", speed=c)
    s.set_initial(phi, psi)
    s.run()
    b = bound(K, ref.umax)
    _held(f"sponge N={N} u^K", max_dev(_fields(s)[0], ref.uK), b)
    _held(f"sponge N={N} u^K-1", max_dev(_fields(s)[1], ref.uK1), b)
    assert ref.e_end < 0.5 * ref.e_start  # (the layers do absorb)


@pytest.mark.parametrize("N,box", [(24, False), (40, True)])
@pytest.mark.parametrize("initial", [False, True])
def test_unit_speed_is_the_speedless_solve(N, box, initial):
    spec = speed_spec(N, box, 1.0, K_=21, check_every=2)
    a, b = Solver(spec, backend="cpu"), Solver(spec, backend="cpu", speed=np.ones((N + 1,) * 3))
    if initial:
        for s in (a, b):
            s.set_initial(*lcg_fields(N))
    ra, rb = a.run(), b.run()
    for x, y in zip(_fields(a), _fields(b)):
        assert same_bits(x, y)
    assert ra.max_err == rb.max_err and ra.rms_err == rb.rms_err


@pytest.mark.parametrize("N,box", [(24, False), (40, True)])
def test_speed_two_is_twice_the_time_step(N, box):
    """c = 2 at tau equals c = 1 at 2 tau bit for bit: scaling lam by 4 is exact in every product. psi is scaled by 1/2."""
    spec = speed_spec(N, box, 2.0, K_=21)
    twice = dataclasses.replace(spec, tau=2.0 * spec.tau)
    phi, psi = lcg_fields(N)
    a, b = Solver(twice, backend="cpu"), Solver(spec, backend="cpu", speed=np.full((N + 1,) * 3, 2.0))
    a.set_initial(phi, 0.5 * psi)
    b.set_initial(phi, psi)
    a.run(), b.run()
    for x, y in zip(_fields(a), _fields(b)):
        assert same_bits(x, y)


def test_refusals():
    N = 24
    spec = speed_spec(N, False, 2.0, K_=9)
    c = two_layer(N)
    with pytest.raises(Exception, match="speed: CFL"):
        Solver(spec, backend="cpu", speed=2.5 * c)
    Solver(spec, backend="cpu", speed=2.5 * c, force=True)
    for bad in (0.0, -1.0, np.nan, np.inf):
        d = c.copy()
        d[3, 4, 5] = bad
        with pytest.raises(Exception, match="speed: every interior value"):
            Solver(spec, backend="cpu", speed=d)
    d = c.copy()
    d[0], d[:, N], d[:, :, 0] = np.nan, -1.0, 0.0  # face values are ignored
    s = Solver(spec, backend="cpu", speed=d)
    t = Solver(spec, backend="cpu", speed=c)
    s.run(), t.run()
    assert same_bits(_fields(s)[0], _fields(t)[0])
    t.set_speed(None)  # cleared: the speedless solve again
    u = Solver(spec, backend="cpu")
    t.run(), u.run()
    assert same_bits(_fields(t)[0], _fields(u)[0])
    with pytest.raises(Exception, match="speed:"):
        Solver(spec, backend="cpu", speed=c[:-1])
