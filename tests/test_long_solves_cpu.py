"""CpuSolver over K = 203 steps at tau = 0.9 tau_max (N = 24 and 40, cube and box 1 x 1.3 x 0.7) against references that do
not compile stencil.hpp: the discrete dispersion relation, a numpy longdouble leapfrog, energy conservation and
source-receiver reciprocity (tests/long_reference.py). Every deviation is held to long_reference.bound = 16 K^2 eps umax
(derived there); each test prints the measured maximum next to it (profiles/longsolve/README.md records them)."""
import functools

import numpy as np
import pytest

from long_reference import (EPS, K_LONG, analytic_factor, bound, closed_form_factor, eigenmode, long_shot, long_spec,
                            longdouble_solve, max_dev, reciprocity_pair)
from sources_common import lcg_fields

from mpi_cuda_amd.solver import Solver

CASES = [pytest.param(N, box, id=f"N{N}-{'box' if box else 'cube'}") for N in (24, 40) for box in (False, True)]
K = K_LONG


def _held(what, dev, bnd):
    print(f"LONGSOLVE {what}: max deviation {dev:.3e} bound {bnd:.3e} ratio {dev / bnd:.2e}")
    assert dev <= bnd, (what, dev, bnd)


def _cpu(N, box, initial=None, shot=None, receivers=None, K_=K):
    s = Solver(long_spec(N, box, K_), backend="cpu")
    if initial is not None:
        s.set_initial(*initial)
    if shot is not None:
        s.set_sources(*shot)
    if receivers is not None:
        s.set_receivers(receivers)
    r = s.run()
    return s, r


def _fields(s):
    return s.global_field(0).numpy(), s.global_field(1).numpy()


def test_closed_form_factor_both_routes():
    """mpmath's cos(n acos(.)) and the 80-digit decimal recurrence are two evaluations of the same number: they agree to
    longdouble precision at every n, for the cube and the box. (A wrong Lambda for the box, or a recurrence that starts
    one step off, separates them or fails the eigenmode tests below.)"""
    for box in (False, True):
        spec = long_spec(40, box)
        for n in (0, 1, 2, 50, K - 1, K):
            a, b = closed_form_factor(spec, n), closed_form_factor(spec, n, use_mpmath=False)
            assert abs(a - b) <= 4 * np.finfo(np.longdouble).eps, (box, n, a, b)
        assert closed_form_factor(spec, 0) == 1 and abs(closed_form_factor(spec, K)) <= 1


@pytest.mark.parametrize("N,box", CASES)
def test_eigenmode_follows_the_dispersion_relation(N, box):
    """Default start (the eigenmode): u^K and u^{K-1} equal phi cos(n omega), and the printed Max Error of every step n
    equals max|phi| |cos(n omega) - cos(a_t n tau)| within bound(n, 1). Catches a wrong omega — a stencil or first-step
    coefficient off in its last digits grows to ~n^2 tau^2 Lambda delta over the solve, eight orders above the bound for
    delta = 1e-8 — a box axis with another axis's 1/h^2, and an error-log entry written at the wrong step index (the log
    of step n would hold another step's difference of cosines)."""
    spec = long_spec(N, box)
    s, r = _cpu(N, box)
    phi = eigenmode(spec)
    uK, uK1 = _fields(s)
    _held(f"eigenmode N={N} box={box} u^K", max_dev(uK, phi * closed_form_factor(spec, K)), bound(K, 1.0))
    _held(f"eigenmode N={N} box={box} u^K-1", max_dev(uK1, phi * closed_form_factor(spec, K - 1)), bound(K - 1, 1.0))
    assert r.steps == list(range(1, K + 1))
    pmax = float(np.abs(phi).max())
    worst = 0.0
    for n, m in zip(r.steps, r.max_err):
        want = pmax * abs(closed_form_factor(spec, n) - analytic_factor(spec, n))
        d = abs(float(np.longdouble(m) - want))
        worst = max(worst, d / bound(n, 1.0))
        assert d <= bound(n, 1.0), (n, m, float(want), d, bound(n, 1.0))
    print(f"LONGSOLVE eigenmode N={N} box={box} Max Error log: worst deviation / bound(n, 1) over {K} steps {worst:.2e}")


@functools.lru_cache(maxsize=None)
def _random_reference(N, box):
    phi, psi = lcg_fields(N)
    rec = long_shot(N, box).receivers
    return longdouble_solve(phi, psi, long_spec(N, box), K, receivers=rec)


@pytest.mark.parametrize("N,box", CASES)
def test_random_data_against_longdouble(N, box):
    """Seeded random phi and psi (every mode of the grid, no symmetry): u^K, u^{K-1} and the traces at nine receivers —
    walls, a face node, the centre — against the longdouble leapfrog. Catches a first step that drops or mis-scales psi,
    a wrong level (2 u^n - u^{n-1} with the levels swapped), a trace row written at the wrong step index."""
    ref = _random_reference(N, box)
    s, _ = _cpu(N, box, initial=lcg_fields(N), receivers=long_shot(N, box).receivers)
    uK, uK1 = _fields(s)
    b = bound(K, ref.umax)
    _held(f"random N={N} box={box} u^K", max_dev(uK, ref.uK), b)
    _held(f"random N={N} box={box} u^K-1", max_dev(uK1, ref.uK1), b)
    _held(f"random N={N} box={box} traces", max_dev(s.traces().numpy(), ref.traces), b)


@functools.lru_cache(maxsize=None)
def shot_reference(N, box):
    shot = long_shot(N, box)
    return longdouble_solve(None, None, long_spec(N, box), K, shot.sources, shot.w, shot.receivers)


@pytest.mark.parametrize("N,box", CASES)
def test_shot_against_longdouble(N, box):
    """Two Ricker sources fired into a field at rest, recorded until the wavefront has crossed the domain and come back
    from the walls. Fields and traces against the longdouble solve; the far receiver is exactly 0.0 before the
    disturbance can reach it and moves afterwards, so an empty signal cannot pass. Catches an addend scaled by the wrong
    cell volume (box), the start's a^0 / 2, a sample applied one step early or late (the far trace would move one row
    early, or every row would differ at the size of the signal)."""
    shot, ref = long_shot(N, box), shot_reference(N, box)
    s, _ = _cpu(N, box, initial=(np.zeros((N + 1,) * 3), None), shot=(shot.sources, shot.w), receivers=shot.receivers)
    uK, uK1 = _fields(s)
    tr = s.traces().numpy()
    b = bound(K, ref.umax)
    _held(f"shot N={N} box={box} u^K", max_dev(uK, ref.uK), b)
    _held(f"shot N={N} box={box} u^K-1", max_dev(uK1, ref.uK1), b)
    _held(f"shot N={N} box={box} traces", max_dev(tr, ref.traces), b)
    far = tr[:, shot.far]
    assert shot.arrival > 50
    assert not far[:shot.arrival].any() and not np.signbit(far[:shot.arrival]).any(), far[:shot.arrival]
    assert far[shot.arrival] != 0.0
    # the wave itself arrives, not just the stencil's exponentially small precursor
    assert np.abs(far).max() > 1e-3 * ref.umax and np.abs(ref.traces[:, shot.far]).max() > 1e-3 * ref.umax


@pytest.mark.parametrize("N,box", CASES)
def test_energy_is_conserved_over_the_long_solve(N, box):
    """E^{K-1/2} = E^{1/2} (cpu.hpp cpu_energy, the quantity tests/test_initial_cpu.py treats as conserved) to a relative
    K 64 eps on seeded random data. Derivation as for ``bound``: the energy is quadratic, so a rounding of relative size
    eps per node and step perturbs it by at most a few eps E per step (4 for the cross terms of the two levels it
    pairs, 16 roundings per node as in ``bound``), and errors of E add at most linearly in the steps since E itself is
    the conserved norm of the error equation. Catches an update that is not time-symmetric (a damping or growing
    scheme moves E by O(tau) per step, 1e10 bounds)."""
    s, _ = _cpu(N, box, initial=lcg_fields(N))
    e1, eK = s.energy(1), s.energy(0)
    drift, tol = abs(eK - e1) / e1, K * 64 * EPS
    print(f"LONGSOLVE energy N={N} box={box}: E(1/2) {e1!r} E(K-1/2) {eK!r} max deviation {drift:.3e} bound {tol:.3e} "
          f"ratio {drift / tol:.2e}")
    assert e1 > 0 and drift <= tol


@pytest.mark.parametrize("N", [24, 40])
def test_reciprocity(N):
    """The discrete operator is symmetric and every node has the same cell volume, so the trace at B of a source at A is
    the trace at A of the same wavelet at B; box geometry, A two nodes from three walls, B in the interior. Two solves of
    the code under test, no reference: catches a stencil whose axis weights depend on the side (lo / hi neighbour
    weights swapped between axes), a wall treated differently on the two sides, a source addend that depends on the
    node."""
    A, B = reciprocity_pair(N)
    w = long_shot(N, True).w[:, :1]
    zero = (np.zeros((N + 1,) * 3), None)
    # (the second receiver is the source's own node: its trace holds the solve's largest values, the bound's umax)
    ab, _ = _cpu(N, True, initial=zero, shot=(A, w), receivers=np.concatenate([B, A]))
    ba, _ = _cpu(N, True, initial=zero, shot=(B, w), receivers=np.concatenate([A, B]))
    tab, tba = ab.traces().numpy(), ba.traces().numpy()
    umax = max(float(np.abs(tab).max()), float(np.abs(tba).max()))
    assert np.abs(tab[:, 0]).max() > 1e-3 * umax and tab.shape == (K + 1, 2)
    _held(f"reciprocity N={N} box", float(np.abs(tab[:, 0] - tba[:, 0]).max()), bound(K, umax))
