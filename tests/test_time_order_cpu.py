"""CpuSolver with time_order = 4 — the definition the GPU path is tested against — checked against references that share
none of its code: a numpy longdouble solve that applies the dense operator twice (tests/time_order_reference.py), the
scheme's closed forms for the eigenmode (first-step factor, dispersion relation, the joint-refinement error table), the CFL
guard at its new limit 3/2, every refusal, the time_order = 2 identity and both CLIs.

Bounds. Every comparison uses long_reference.bound = 16 K^2 eps umax at K = 203 and tau = 0.9 of the limit, as for the
other long solves. Re-derived for this operator: a step makes 32 roundings per node — 15 for v = lam s(u) (per axis two
additions and two fused operations, two to combine the axes, the product), 14 for s(v), 3 in the update ((2u - u_old) + v,
then the fused lam12 s(v) term). Their size is eps times the intermediate they round, and at 0.9 of the limit the
operator's largest symbol is z = 9.72 (3.24 per axis), so v reaches 9.72 umax for the stiffest mode where the (4, 2) scheme's
lam s(u) stayed below 3.3 umax: weighted by these sizes and by 1 + z / 12 <= 1.81 for what the second application does to
an error in v, the strict worst case is about 190 eps umax per step. The response to a kick is the leapfrog's,
sin((n - m) omega) / sin(omega) <= n - m (cos(omega) = 1 - z / 2 + z^2 / 24 lies in [-0.5, 1] for 0 <= z <= 9.72, so
1 / sin(omega) < 1.16 for the stiff modes), hence K^2 / 2 kicks: about 95 K^2 eps umax if every rounding of every node and
step had the worst size and sign. bound() is kept as it is, six times tighter than that worst case; it is no rigorous
bound here but the same yardstick the (2, 2) and (4, 2) solves are held to, and the measured distances (TIME_ORDER lines,
recorded in profiles/time_order/README.md) are four orders of magnitude inside it, as theirs are."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from long_reference import LD, bound, max_dev
from order4_reference import eigenmode4
from sources_common import lcg_fields, same_bits
from time_order_reference import (closed_form_error, dispersion_factor, first_step_factor, joint_refinement_spec,
                                  time_order_solve, time_order_spec)

from mpi_cuda_amd.models.wave3d import ProblemSpec
from mpi_cuda_amd.solver import Solver
from mpi_cuda_amd.utils import dump as dumpio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 203
GRIDS = [(24, False), (40, True)]
MUTATIONS = (dict(c4=24), dict(reflect_v=False))


def _held(what, dev, bnd):
    print(f"TIME_ORDER {what}: max deviation {dev:.3e} bound {bnd:.3e} ratio {dev / bnd:.2e}")
    assert dev <= bnd, (what, dev, bnd)


@pytest.mark.parametrize("N,box", GRIDS)
def test_eigenmode_against_longdouble_and_closed_form(N, box):
    spec = time_order_spec(N, box, K)
    assert spec.cfl_ok and spec.courant > 1.0  # (beyond what either second-order-in-time scheme allows)
    s = Solver(spec, backend="cpu")
    r = s.run()
    phi = eigenmode4(spec)
    uK, uK1, umax = time_order_solve(phi, None, spec, K)
    got = s.global_field(0).numpy()
    _held(f"eigenmode N={N} box={box} u^K vs longdouble", max_dev(got, uK), bound(K, umax))
    _held(f"eigenmode N={N} box={box} u^K-1 vs longdouble", max_dev(s.global_field(1).numpy(), uK1), bound(K - 1, umax))
    # u^n = cos(n omega_h tau) phi: the first step's factor is the recurrence's cosine
    assert abs(first_step_factor(spec) - dispersion_factor(spec, 1)) < 4 * np.finfo(LD).eps
    _held(f"eigenmode N={N} box={box} u^K vs dispersion", max_dev(got, phi * dispersion_factor(spec, K)), bound(K, 1.0))
    # the Max Error log against the closed form at every step (check_every = 1)
    assert r.steps == list(range(1, K + 1))
    pmax = float(np.abs(phi).max())
    worst = 0.0
    for n, m in zip(r.steps, r.max_err):
        want = pmax * closed_form_error(spec, n)
        d = abs(m - float(want))
        worst = max(worst, d / bound(n, 1.0))
        assert d <= bound(n, 1.0), (n, m, float(want), d)
    print(f"TIME_ORDER eigenmode N={N} box={box} Max Error log vs closed form: worst deviation / bound(n, 1) {worst:.2e}")
    # (for this smooth mode a missing reflection of v only changes the tau^4 term next to a wall, where v = O(z sin(pi / N))
    # is small: 1e5 bounds here, 1e6 for the random data below)
    for kw in MUTATIONS:
        bad = time_order_solve(phi, None, spec, K, **kw)[0]
        assert max_dev(got, bad) > 1e5 * bound(K, umax), kw


@pytest.mark.parametrize("N,box", GRIDS)
def test_initial_data_against_longdouble(N, box):
    spec = time_order_spec(N, box, K)
    phi, psi = lcg_fields(N)
    s = Solver(spec, backend="cpu")
    s.set_initial(phi, psi)
    r = s.run()
    assert r.finite
    uK, uK1, umax = time_order_solve(phi, psi, spec, K)
    b = bound(K, umax)
    got = s.global_field(0).numpy()
    _held(f"initial N={N} box={box} u^K vs longdouble", max_dev(got, uK), b)
    _held(f"initial N={N} box={box} u^K-1 vs longdouble", max_dev(s.global_field(1).numpy(), uK1), b)
    for kw in MUTATIONS + (dict(psi3=False),):
        assert max_dev(got, time_order_solve(phi, psi, spec, K, **kw)[0]) > 1e6 * b, kw
    # psi absent: the psi step is skipped, and equals a psi of zeros only up to the sign of zero
    s.set_initial(phi, None)
    s.run()
    _held(f"initial N={N} box={box} phi only, u^K vs longdouble", max_dev(s.global_field(0).numpy(),
                                                                           time_order_solve(phi, None, spec, K)[0]), b)


# eigenmode (1,1,1), unit cube, T = 0.5, the fewest steps K with tau = T / K <= 0.9 of each scheme's limit: (K, the
# largest Max Error of the steps 1..K in closed form, max_n |cos(n omega_h tau) - cos(a_t n tau)|)
TABLE = {4: {8: (6, 3.36e-4), 16: (11, 2.45e-5), 32: (21, 1.65e-6), 64: (42, 1.03e-7)},
         2: {8: (9, 6.71e-3), 16: (18, 1.72e-3), 32: (36, 4.32e-4), 64: (72, 1.08e-4)}}


def test_joint_refinement_converges_at_fourth_order():
    got = {}
    for to in (4, 2):
        for N, (K_, err) in TABLE[to].items():
            spec = joint_refinement_spec(N, to)
            assert spec.K == K_ and spec.cfl_ok
            cf = [float(closed_form_error(spec, n, to)) for n in range(1, K_ + 1)]
            assert abs(max(cf) - err) <= 0.006 * err, (to, N, max(cf), err)  # (the table's three digits)
            if N == 64:
                continue
            r = Solver(spec, backend="cpu").run()
            assert r.steps == list(range(1, K_ + 1))
            assert all(abs(m - c) <= bound(n, 1.0) for n, m, c in zip(r.steps, r.max_err, cf))
            got[to, N] = max(r.max_err)
            print(f"TIME_ORDER joint refinement time_order={to} N={N} K={K_}: largest Max Error {got[to, N]:.4e} closed form "
                  f"{max(cf):.4e}")
    r4 = (got[4, 8] / got[4, 16], got[4, 16] / got[4, 32])
    r2 = (got[2, 8] / got[2, 16], got[2, 16] / got[2, 32])
    print(f"TIME_ORDER joint refinement ratios: time order 4 {r4[0]:.2f} {r4[1]:.2f}; time order 2 {r2[0]:.2f} {r2[1]:.2f}")
    assert r4[0] > 13 and r4[1] > 13
    assert r2[0] < 4.1 and r2[1] < 4.1


def test_cfl_guard_at_the_new_limit():
    N = 16
    tau_max = ProblemSpec(N=N).tau_max
    lim = 1.5 * tau_max
    ok = ProblemSpec(N=N, tau=0.999 * lim, K=5, order=4, time_order=4)
    assert ok.cfl_ok and abs(ok.courant_eff - 0.999) < 1e-12 and ok.courant_limit == 1.5
    Solver(ok, backend="cpu").run()
    over = ProblemSpec(N=N, tau=1.001 * lim, K=5, order=4, time_order=4)
    with pytest.raises(ValueError, match="CFL violated: courant = .* for order = 4, time_order = 4"):
        Solver(over, backend="cpu")
    Solver(over, backend="cpu", force=True).run()
    # (4, 2) at its own limit is unchanged
    lim2 = tau_max * np.sqrt(3.0) / 2.0
    Solver(ProblemSpec(N=N, tau=0.999 * lim2, K=5, order=4), backend="cpu")
    with pytest.raises(ValueError, match="CFL violated: courant = .* > sqrt\\(3\\)/2 for order = 4 \\(effective"):
        Solver(ProblemSpec(N=N, tau=1.001 * lim2, K=5, order=4), backend="cpu")
    assert ProblemSpec(N=N, tau=lim2, order=4).courant_eff == ProblemSpec(N=N, tau=lim2, order=4, time_order=2).courant_eff
    # Just over the limit a forced solve grows. The stiffest mode of the N = 16 grid has 0.988 of the largest symbol, so
    # tau = 1.01 lim puts it at z = 12.09, where the step's symbol 2 - z + z^2 / 12 = 2.096 gives a growth of 1.36 per step:
    # e^92 over 300 steps, overflow after about 2300. Just under the limit the same data stay O(1).
    phi, psi = lcg_fields(N)

    def run(f, K_, ce):
        s = Solver(ProblemSpec(N=N, tau=f * lim, K=K_, check_every=ce, order=4, time_order=4), backend="cpu", force=True)
        s.set_initial(phi, psi)
        return s.run(), float(np.abs(s.global_field(0).numpy()).max())

    r, m = run(0.999, 300, 100)
    assert r.finite and m < 10.0
    r, m = run(1.01, 300, 100)
    assert m > 1e20
    r, m = run(1.01, 2600, 200)
    assert not r.finite


def test_time_order_2_given_explicitly_is_the_default():
    for order in (2, 4):
        a = Solver(ProblemSpec(N=24, tau=1e-3, K=23, order=order), backend="cpu")
        b = Solver(ProblemSpec(N=24, tau=1e-3, K=23, order=order, time_order=2), backend="cpu")
        ra, rb = a.run(), b.run()
        assert ra.lines() == rb.lines() and ra.max_err == rb.max_err and ra.rms_err == rb.rms_err
        assert same_bits(a.global_field(0).numpy(), b.global_field(0).numpy())
        assert same_bits(a.global_field(1).numpy(), b.global_field(1).numpy())
        assert ProblemSpec(N=24, order=order, time_order=2).as_dict() == ProblemSpec(N=24, order=order).as_dict()
    assert "time_order" not in ProblemSpec(N=24, order=4).as_dict()
    assert ProblemSpec(N=24, order=4, time_order=4).as_dict()["time_order"] == 4
    from mpi_cuda_amd._native import load

    C = load()
    c2, c4 = C.Coeffs.from_problem(C.Problem(24, 1e-3, 9, 1.0, order=4)), C.Coeffs.from_problem(
        C.Problem(24, 1e-3, 9, 1.0, order=4, time_order=4))
    assert c2.time_order == 2 and c4.time_order == 4 and c2.lam == c4.lam and c2.half_lam == c4.half_lam
    assert (c4.lam12, c4.lam24, c4.lam6) == (c4.lam / 12.0, c4.lam / 24.0, c4.lam / 6.0)


def test_refusals():
    from mpi_cuda_amd._native import load

    C = load()
    N = 16
    with pytest.raises(ValueError, match="time_order: the time order must be 2 or 4"):
        ProblemSpec(N=N, order=4, time_order=3)
    with pytest.raises(ValueError, match="time_order: 4 needs order = 4"):
        ProblemSpec(N=N, time_order=4)
    with pytest.raises(RuntimeError, match="^wave3d: time_order: the time order must be 2 or 4"):
        C.Problem(N, 1e-3, 9, 1.0, order=4, time_order=3)
    with pytest.raises(RuntimeError, match="^wave3d: time_order: 4 needs order = 4"):
        C.Problem(N, 1e-3, 9, 1.0, time_order=4)
    spec = ProblemSpec(N=N, tau=1e-3, K=9, order=4, time_order=4)
    one = np.ones((N + 1,) * 3)
    nodes, w = np.array([[3, 4, 5]], dtype=np.int64), np.ones((9, 1))
    # point sources: new with the time order
    s = Solver(spec, backend="cpu")
    with pytest.raises(ValueError, match="time_order: no point sources"):
        s.set_sources(nodes, w)
    n = C.CpuSolver(spec.native(), 1, 0)
    with pytest.raises(RuntimeError, match="^wave3d: time_order: no point sources"):
        n.set_sources(nodes, w)
    # what order = 4 refuses stays refused, with its messages
    with pytest.raises(ValueError, match="order: no sponge"):
        ProblemSpec(N=N, order=4, time_order=4, sponge=3)
    with pytest.raises(RuntimeError, match="order: no sponge"):
        C.Problem(N, 1e-3, 9, 1.0, sponge=C.Sponge(3, 0.0, 63), order=4, time_order=4)
    with pytest.raises(ValueError, match="order: no speed field"):
        Solver(spec, backend="cpu", speed=one)
    with pytest.raises(ValueError, match="order: order = 4 runs on one rank only"):
        Solver(spec, backend="cpu", rank=0, world=2)
    s.run()
    for call, msg in ((lambda: s.energy(0), "order: the second-order discrete energy"),
                      (lambda: s.set_speed(one), "order: no speed field"),
                      (lambda: s.set_state(one, one, 3), "order: order = 4 not together")):
        with pytest.raises(ValueError, match=msg):
            call()
    for call in (lambda: n.set_speed(one.reshape(-1), False), lambda: n.set_state(one.reshape(-1), one.reshape(-1), 3),
                 lambda: n.energy(0)):
        with pytest.raises(RuntimeError, match="^wave3d: order:"):
            call()
    # the distributed CPU program
    p = subprocess.run([os.path.join(ROOT, "bin", "wave3d"), str(N), "1e-3", "9", "--cpu", "--np", "2", "--order", "4",
                        "--time-order", "4"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "time_order:" in p.stderr
    p = subprocess.run([os.path.join(ROOT, "bin", "wave3d"), str(N), "1e-3", "9", "--cpu", "--time-order", "4"], cwd=ROOT,
                       capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "time_order: 4 needs order = 4" in p.stderr


@pytest.mark.parametrize("cli", ["native", "python"])
def test_cli_roundtrip(tmp_path, cli):
    N, K_ = 16, 11
    spec = ProblemSpec(N=N, tau=0.05, K=K_, order=4, time_order=4)  # (courant 1.39: refused without the time order)
    s = Solver(spec, backend="cpu")
    s.set_receivers(np.array([[3, 4, 5], [8, 8, 8]]))
    s.run()
    out, js, tr = str(tmp_path / "out"), str(tmp_path / "summary.json"), str(tmp_path / "tr")
    rc = tmp_path / "rec.txt"
    rc.write_text("3 4 5\n8 8 8\n")
    common = [str(N), "0.05", str(K_), "--order", "4", "--time-order", "4", "--dump", out, "--json", js, "--quiet",
              "--receivers", str(rc), "--traces", tr]
    cmd = ([sys.executable, "-m", "mpi_cuda_amd", *common, "--backend", "cpu"] if cli == "python"
           else [os.path.join(ROOT, "bin", "wave3d"), *common, "--cpu"])
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    f, meta = dumpio.load(out)
    assert same_bits(f, s.global_field(0).numpy())
    assert meta["time_order"] == 4 and meta["space_order"] == 4 and json.load(open(js))["time_order"] == 4
    tmeta = json.load(open(tr + ".json"))
    assert tmeta["time_order"] == 4
    got = np.fromfile(tr + ".bin", dtype="<f8").reshape(tmeta["shape"])
    assert same_bits(got, s.traces().numpy())
    # --order 4 alone: refused at this tau (CFL), and at a stable tau its sidecars do not name the time order
    i = cmd.index("--time-order")
    base = cmd[:i] + cmd[i + 2:]
    p = subprocess.run(base, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "CFL violated" in p.stderr
    base[base.index("0.05")] = "1e-3"
    p = subprocess.run(base, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "time_order" not in dumpio.load(out)[1] and "time_order" not in json.load(open(js))
    assert "time_order" not in json.load(open(tr + ".json"))
    # refusals at the command line
    p = subprocess.run(cmd + ["--sources", "x"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "time_order:" in p.stderr
