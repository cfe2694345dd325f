"""CpuSolver with order = 4 — the definition the GPU path is tested against — checked against references that share none
of its code: a numpy longdouble leapfrog with the operator and the reflection written independently
(tests/order4_reference.py), the scheme's discrete dispersion relation, the convergence order, the CFL guard at its new
limit, the order = 2 identity, every refusal, and both CLIs.

Bounds. K = 203 at tau = 0.9 of the fourth-order limit: long_reference.bound = 16 K^2 eps umax holds as derived there — a
step of this scheme makes 16 roundings per node too (per axis two additions and two fused operations, two to combine the
axes, two in the update), each of size <= eps umax after the coefficient tau^2 / (12 h^2) (whose product with an axis sum
is below 1.1 umax at this tau), and 1 / sin(omega) < 1.3 at 0.9 of the limit as for the second-order scheme. The measured
distances are printed (ORDER4 lines) and recorded in profiles/order4/README.md."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from long_reference import EPS, bound, max_dev
from order4_reference import dispersion_factor, eigenmode4, order4_solve, order4_spec
from sources_common import lcg_fields, same_bits

from mpi_cuda_amd.models.wave3d import ProblemSpec
from mpi_cuda_amd.solver import Solver
from mpi_cuda_amd.utils import dump as dumpio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 203
GRIDS = [(24, False), (40, True)]


def _held(what, dev, bnd):
    print(f"ORDER4 {what}: max deviation {dev:.3e} bound {bnd:.3e} ratio {dev / bnd:.2e}")
    assert dev <= bnd, (what, dev, bnd)


@pytest.mark.parametrize("N,box", GRIDS)
def test_eigenmode_against_longdouble_and_dispersion(N, box):
    spec = order4_spec(N, box, K)
    s = Solver(spec, backend="cpu")
    r = s.run()
    phi = eigenmode4(spec)
    uK, uK1, umax = order4_solve(phi, None, spec, K)
    got = s.global_field(0).numpy()
    _held(f"eigenmode N={N} box={box} u^K vs longdouble", max_dev(got, uK), bound(K, umax))
    _held(f"eigenmode N={N} box={box} u^K-1 vs longdouble", max_dev(s.global_field(1).numpy(), uK1), bound(K - 1, umax))
    # the discrete dispersion relation at every checked level (check_every = 1: all of them)
    assert r.steps == list(range(1, K + 1))
    _held(f"eigenmode N={N} box={box} u^K vs dispersion", max_dev(got, phi * dispersion_factor(spec, K)), bound(K, 1.0))
    pmax = float(np.abs(phi).max())
    a_t = np.longdouble(spec.a_t)
    worst = 0.0
    for n, m in zip(r.steps, r.max_err):
        want = pmax * abs(dispersion_factor(spec, n) - np.cos(a_t * (n * np.longdouble(spec.tau))))
        d = abs(m - float(want))
        worst = max(worst, d / bound(n, 1.0))
        assert d <= bound(n, 1.0), (n, m, float(want), d)
    print(f"ORDER4 eigenmode N={N} box={box} Max Error log vs dispersion: worst deviation / bound(n, 1) {worst:.2e}")
    # a deliberately wrong operator in the reference lands orders of magnitude outside the bound
    for kw in (dict(coef=15), dict(wall=+1)):
        bad = order4_solve(phi, None, spec, K, **kw)[0]
        assert max_dev(got, bad) > 1e6 * bound(K, umax), kw


@pytest.mark.parametrize("N,box", GRIDS)
def test_initial_data_against_longdouble(N, box):
    spec = order4_spec(N, box, K)
    phi, psi = lcg_fields(N)
    s = Solver(spec, backend="cpu")
    s.set_initial(phi, psi)
    s.run()
    uK, uK1, umax = order4_solve(phi, psi, spec, K)
    b = bound(K, umax)
    got = s.global_field(0).numpy()
    _held(f"initial N={N} box={box} u^K vs longdouble", max_dev(got, uK), b)
    _held(f"initial N={N} box={box} u^K-1 vs longdouble", max_dev(s.global_field(1).numpy(), uK1), b)
    for kw in (dict(coef=15), dict(wall=+1)):
        assert max_dev(got, order4_solve(phi, psi, spec, K, **kw)[0]) > 1e6 * b, kw


def test_convergence_is_fourth_order():
    def err(N, order):
        return Solver(ProblemSpec(N=N, tau=1e-4, K=200, order=order), backend="cpu").run().max_err[-1]

    e4 = [err(N, 4) for N in (8, 16, 32)]
    e2 = [err(N, 2) for N in (8, 16, 32)]
    print(f"ORDER4 convergence: order 4 {e4} ratios {e4[0] / e4[1]:.2f} {e4[1] / e4[2]:.2f}; order 2 {e2}")
    assert 14.0 <= e4[0] / e4[1] <= 18.0 and 14.0 <= e4[1] / e4[2] <= 18.0
    assert 3.8 <= e2[0] / e2[1] <= 4.2
    assert e4[1] < e2[2]


def test_cfl_guard_at_the_new_limit():
    N = 16
    lim = ProblemSpec(N=N).tau_max * np.sqrt(3.0) / 2.0
    Solver(ProblemSpec(N=N, tau=0.999 * lim, K=5, order=4), backend="cpu")
    with pytest.raises(ValueError, match="CFL violated: courant = .* for order = 4"):
        Solver(ProblemSpec(N=N, tau=1.001 * lim, K=5, order=4), backend="cpu")
    Solver(ProblemSpec(N=N, tau=1.001 * lim, K=5, order=4), backend="cpu", force=True)
    Solver(ProblemSpec(N=N, tau=1.001 * lim, K=5), backend="cpu")  # (an order-2 solve at the same tau is untouched)
    # a forced solve at the classic Courant number 0.95 blows up and says so; order 2 at the same tau stays O(1)
    tau = 0.95 * ProblemSpec(N=N).tau_max
    phi, psi = lcg_fields(N)
    s = Solver(ProblemSpec(N=N, tau=tau, K=4000, check_every=500, order=4), backend="cpu", force=True)
    s.set_initial(phi, psi)
    assert not s.run().finite
    s2 = Solver(ProblemSpec(N=N, tau=tau, K=400, check_every=100), backend="cpu")
    s2.set_initial(phi, psi)
    assert s2.run().finite and float(np.abs(s2.global_field(0).numpy()).max()) < 1e3


def test_order2_given_explicitly_is_the_default():
    a = Solver(ProblemSpec(N=24, tau=1e-3, K=23), backend="cpu")
    b = Solver(ProblemSpec(N=24, tau=1e-3, K=23, order=2), backend="cpu")
    ra, rb = a.run(), b.run()
    assert ra.lines() == rb.lines() and ra.max_err == rb.max_err and ra.rms_err == rb.rms_err
    assert same_bits(a.global_field(0).numpy(), b.global_field(0).numpy())
    assert same_bits(a.global_field(1).numpy(), b.global_field(1).numpy())
    assert ProblemSpec(N=24, order=2).as_dict() == ProblemSpec(N=24).as_dict() and "order" not in ProblemSpec(N=24).as_dict()
    assert ProblemSpec(N=24, order=4).as_dict()["order"] == 4


def test_refusals():
    from mpi_cuda_amd._native import load

    C = load()
    N = 16
    with pytest.raises(ValueError, match="order: the spatial order must be 2 or 4"):
        ProblemSpec(N=N, order=3)
    with pytest.raises(ValueError, match="order: no sponge"):
        ProblemSpec(N=N, order=4, sponge=3)
    with pytest.raises(RuntimeError, match="order: no sponge"):
        C.Problem(N, 1e-3, 9, 1.0, sponge=C.Sponge(3, 0.0, 63), order=4)
    spec = ProblemSpec(N=N, tau=1e-3, K=9, order=4)
    one = np.ones((N + 1,) * 3)
    with pytest.raises(ValueError, match="order: no speed field"):
        Solver(spec, backend="cpu", speed=one)
    with pytest.raises(ValueError, match="order: order = 4 runs on one rank only"):
        Solver(spec, backend="cpu", rank=0, world=2)
    s = Solver(spec, backend="cpu")
    s.run()
    for call, msg in ((lambda: s.energy(0), "order: the second-order discrete energy"),
                      (lambda: s.set_speed(one), "order: no speed field"),
                      (lambda: s.set_state(one, one, 3), "order: order = 4 not together")):
        with pytest.raises(ValueError, match=msg):
            call()
    n = C.CpuSolver(spec.native(), 1, 0)
    for call in (lambda: n.set_speed(one.reshape(-1), False), lambda: n.set_state(one.reshape(-1), one.reshape(-1), 3),
                 lambda: n.energy(0)):
        with pytest.raises(RuntimeError, match="^wave3d: order:"):
            call()
    # the distributed CPU program
    p = subprocess.run([os.path.join(ROOT, "bin", "wave3d"), str(N), "1e-3", "9", "--cpu", "--np", "2", "--order", "4"],
                       cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "order:" in p.stderr


@pytest.mark.parametrize("cli", ["native", "python"])
def test_cli_roundtrip(tmp_path, cli):
    N, K_ = 16, 11
    spec = ProblemSpec(N=N, tau=1e-3, K=K_, order=4)
    s = Solver(spec, backend="cpu")
    s.run()
    out, js = str(tmp_path / "out"), str(tmp_path / "summary.json")
    common = [str(N), "1e-3", str(K_), "--order", "4", "--dump", out, "--json", js, "--quiet"]
    cmd = ([sys.executable, "-m", "mpi_cuda_amd", *common, "--backend", "cpu"] if cli == "python"
           else [os.path.join(ROOT, "bin", "wave3d"), *common, "--cpu"])
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    f, meta = dumpio.load(out)
    assert same_bits(f, s.global_field(0).numpy())
    assert meta["space_order"] == 4 and meta["order"] == "C" and json.load(open(js))["order"] == 4
    p = subprocess.run([c for c in cmd if c not in ("--order", "4")], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "space_order" not in dumpio.load(out)[1] and "order" not in json.load(open(js))
    p = subprocess.run(cmd + ["--energy", "--initial", "x"] if cli == "native" else cmd + ["--sponge", "3"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "order:" in p.stderr
