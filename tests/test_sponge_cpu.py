"""Sponge layers on the CPU (CpuSolver is the definition of the damped scheme): the switch-off cases reproduce the
undamped solve bit for bit, nodes outside the layers get the undamped bits, 203-step solves against the numpy longdouble
damped leapfrog (tests/sponge_reference.py) within long_reference.bound, the energy decays, a centred shot is absorbed,
the refusals, and both CLIs. Each comparison prints its measured margin (profiles/sponge/README.md records them)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from long_reference import EPS, K_LONG, long_spec, max_dev, ricker16
from sources_common import lcg_fields, same_bits
from sponge_reference import bound, damped_solve, energy, energy_tolerance, sponge_g

from mpi_cuda_amd import ProblemSpec
from mpi_cuda_amd._native import load
from mpi_cuda_amd.solver import Solver
from mpi_cuda_amd.utils import dump as dumpio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "wave3d")
K = K_LONG


def _held(what, dev, bnd):
    print(f"SPONGE {what}: max deviation {dev:.3e} bound {bnd:.3e} ratio {dev / bnd:.2e}")
    assert dev <= bnd, (what, dev, bnd)


def _with(spec, sponge):
    import dataclasses

    return dataclasses.replace(spec, sponge=sponge)


def _cpu(spec, initial=None, shot=None, receivers=None):
    s = Solver(spec, backend="cpu")
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


REC24 = np.array([[12, 12, 12], [1, 12, 23], [3, 4, 5], [24, 7, 7], [20, 21, 22]], dtype=np.int64)


@pytest.mark.parametrize("sponge", [(0, 0.0, 63), (6, 0.0, 0), (0, 5.0, 5)], ids=["width0", "faces0", "width0-sigma"])
def test_switched_off_reproduces_the_undamped_solve(sponge):
    """width = 0 and faces = 0 mean no sponge: fields, error log and traces of the undamped solve, bit for bit."""
    spec = long_spec(24, True, K=23, check_every=2)
    a, ra = _cpu(spec, initial=lcg_fields(24), receivers=REC24)
    b, rb = _cpu(_with(spec, sponge), initial=lcg_fields(24), receivers=REC24)
    assert _with(spec, sponge).sponge is None
    for fa, fb in zip(_fields(a), _fields(b)):
        assert same_bits(fa, fb)
    assert ra.steps == rb.steps and same_bits(ra.max_err, rb.max_err) and same_bits(ra.rms_err, rb.rms_err)
    assert same_bits(a.traces().numpy(), b.traces().numpy())


@pytest.mark.parametrize("box", [False, True], ids=["cube", "box"])
def test_one_step_outside_the_layers_is_the_undamped_step(box):
    """cpu_leapfrog from seeded random levels with and without the tables: every node with g = 0 holds the undamped
    step's bits, and the nodes of the layers differ (one-sided faces: x-, y+, z- and z+)."""
    C = load()
    N, sponge = 24, (5, 0.0, 0b111001)
    spec = _with(long_spec(N, box, K=4), sponge)
    prob = spec.native()
    lay = C.make_layout(prob, C.rank_box(prob, C.Dims(1, 1, 1), 0))
    co = C.Coeffs.from_problem(prob)
    s_ext = C.sin_table_ext(prob)
    phi, psi = lcg_fields(N)
    cur = C.initial_to_local(lay, phi.reshape(-1))
    old = C.initial_to_local(lay, psi.reshape(-1))
    plain, damped = old.copy(), old.copy()
    C.cpu_leapfrog(lay, co, cur, plain, C.compute_box(lay), s_ext)
    C.cpu_leapfrog(lay, co, cur, damped, C.compute_box(lay), s_ext, sponge=prob)
    g = sponge_g(spec, sponge)
    tab = C.sponge_tables(prob)
    assert tab.shape == (6, N + 3)
    gn = np.maximum(np.maximum(tab[0, 1:N + 2, None, None], tab[1, None, 1:N + 2, None]), tab[2, None, None, 1:N + 2])
    assert same_bits(gn, g)  # (the reference's g: the same float64 formula)
    from mpi_cuda_amd.ops.stencil import grid_view
    import torch

    pv = grid_view(lay, torch.from_numpy(plain)).numpy()[1:N + 2, 1:N + 2, 1:N + 2]
    dv = grid_view(lay, torch.from_numpy(damped)).numpy()[1:N + 2, 1:N + 2, 1:N + 2]
    same = pv.view(np.int64) == dv.view(np.int64)
    assert same[g == 0].all()
    assert (g > 0).sum() > 0 and (~same[g > 0]).sum() > 0.5 * (g > 0).sum()
    # x+ and y- are not damped: their neighbourhoods away from the other layers are untouched
    assert (g[N - 4:N, 6:12, 6:18] == 0).all() and (g[6:18, 1:5, 6:18] == 0).all() and (g[1:5, 6:12, 6:18] > 0).all()


CASES = [pytest.param(24, False, id="N24-cube"), pytest.param(40, True, id="N40-box")]


@functools.lru_cache(maxsize=None)
def _case(N, box):
    sponge = (6, 0.0, 63) if N == 24 else (8, 0.0, 0b110111)  # (N = 40: the y+ face keeps reflecting)
    rec = np.array([[N // 2] * 3, [2, N // 2, N - 2], [N - 1, N - 1, N - 1], [3, 5, 4], [N, 3, 3]], dtype=np.int64)
    return sponge, rec


@functools.lru_cache(maxsize=None)
def _random_reference(N, box):
    sponge, rec = _case(N, box)
    phi, psi = lcg_fields(N)
    return damped_solve(phi, psi, long_spec(N, box), K, sponge, receivers=rec)


@pytest.mark.parametrize("N,box", CASES)
def test_random_data_against_the_longdouble_damped_leapfrog(N, box):
    """K = 203 at tau = 0.9 tau_max from seeded random phi, psi: u^K, u^{K-1} and five traces (centre, inside a layer, a
    corner, a face) against the longdouble damped leapfrog, within 16 K^2 eps umax. Catches a profile with the wrong
    ramp, width or face, (1 - g) and (1 + g) swapped, g taken from the wrong axis, a damped node read from the wrong
    level."""
    sponge, rec = _case(N, box)
    ref = _random_reference(N, box)
    s, _ = _cpu(_with(long_spec(N, box), sponge), initial=lcg_fields(N), receivers=rec)
    uK, uK1 = _fields(s)
    b = bound(K, ref.umax)
    _held(f"random N={N} box={box} u^K", max_dev(uK, ref.uK), b)
    _held(f"random N={N} box={box} u^K-1", max_dev(uK1, ref.uK1), b)
    _held(f"random N={N} box={box} traces", max_dev(s.traces().numpy(), ref.traces), b)
    # the layers did something: the undamped solve from the same data is far outside the bound
    plain, _ = _cpu(long_spec(N, box), initial=lcg_fields(N))
    assert max_dev(plain.global_field(0).numpy(), ref.uK) > 1e6 * b


@pytest.mark.parametrize("N,box", CASES)
def test_energy_decays_and_tiny_sigma_conserves_it(N, box):
    """Random data: E(K-1/2) <= E(1/2) up to the summation-error scale (eps * depth * sum |terms|, energy_sums().abs), and
    with sigma so small that g = tau * sigma * q^2 underflows to 0 the energy is conserved exactly as without a sponge:
    the same bits as the undamped solve."""
    sponge, _ = _case(N, box)
    spec = long_spec(N, box)
    s, _ = _cpu(_with(spec, sponge), initial=lcg_fields(N))
    e1, eK = s.energy(1), s.energy(0)
    sums = [s._impl.energy_sums(w) for w in (1, 0)]
    half_v = 0.5 * np.prod([e / N for e in spec.edges])
    slack = sum(EPS * (4 + d["depth"]) * half_v * d["abs"] for d in sums)
    print(f"SPONGE energy N={N} box={box}: E(1/2) {e1!r} E(K-1/2) {eK!r} ratio {eK / e1:.3e} slack {slack:.3e}")
    assert e1 > 0 and eK <= e1 + slack
    assert eK < e1 - slack  # (... and it does decay)
    tiny, _ = _cpu(_with(spec, (sponge[0], 1e-323, sponge[2])), initial=lcg_fields(N))
    plain, _ = _cpu(spec, initial=lcg_fields(N))
    assert load().sponge_tables(_with(spec, (sponge[0], 1e-323, sponge[2])).native())[:3].max() == 0.0
    assert tiny.energy(0) == plain.energy(0) and tiny.energy(1) == plain.energy(1)
    assert same_bits(tiny.global_field(0).numpy(), plain.global_field(0).numpy())


# ---- absorption ----------------------------------------------------------------------------------------------------------
N_ABS, W_ABS, K_ABS = 40, 8, 170


def absorption_spec(sponge=None):
    return _with(long_spec(N_ABS, False, K=K_ABS), sponge)


@functools.lru_cache(maxsize=None)
def absorption_shot():
    """A Ricker wavelet at the centre of the N = 40 cube, f0 = N / 10 (a wavelength of 10 nodes), t0 = 1.5 / f0: it has
    died out after 3 / f0 = 0.75 = 58 steps at tau = 0.9 tau_max = 0.013. The front moves tau / h = 0.52 nodes per step:
    20 nodes to a wall and W back out of the layer take 54 steps on an axis and 20 sqrt(3) + W sqrt(3) = 48.5 nodes = 93
    steps along the diagonal, so by K = 170 > 58 + 93 every part of the wavefront has crossed a layer twice."""
    tau = absorption_spec().tau
    f0 = N_ABS / 10.0
    src = np.array([[N_ABS // 2] * 3], dtype=np.int64)
    w = ricker16(f0, 1.5 / f0, tau, K_ABS)[:, None]
    rec = np.array([[N_ABS // 2] * 3, [N_ABS // 2, N_ABS // 2, 28], [12, 12, 12]], dtype=np.int64)
    return src, np.ascontiguousarray(w), rec


@functools.lru_cache(maxsize=None)
def absorption_references():
    src, w, rec = absorption_shot()
    damped = damped_solve(None, None, absorption_spec(), K_ABS, (W_ABS, 0.0, 63), src, w, rec)
    walls = damped_solve(None, None, absorption_spec(), K_ABS, None, src, w, rec)
    return damped, walls


def test_absorption_of_a_centred_shot():
    """All six faces damped, W = 8: the longdouble reference ALONE leaves at most 1/10 of the energy the same shot has
    between Dirichlet walls at the same step (checked first, on the reference); then CpuSolver's two energies at that
    step — with the layers and between the walls — match the reference's within the rounding rule pushed through the
    energy's first-order sensitivity."""
    damped, walls = absorption_references()
    spec = absorption_spec()
    e_d, e_w = energy(damped.uK1, damped.uK, spec), energy(walls.uK1, walls.uK, spec)
    ratio = float(e_d.E / e_w.E)
    print(f"SPONGE absorption N={N_ABS} W={W_ABS} K={K_ABS}: reference residual energy / Dirichlet energy = {ratio:.3e}")
    assert e_w.E > 0 and ratio <= 0.1
    src, w, rec = absorption_shot()
    zero = (np.zeros((N_ABS + 1,) * 3), None)
    depth = 3 * (N_ABS + 1)
    for name, sponge, ref, want in (("sponge", (W_ABS, 0.0, 63), damped, e_d), ("walls", None, walls, e_w)):
        s, _ = _cpu(absorption_spec(sponge), initial=zero, shot=(src, w), receivers=rec)
        tol = energy_tolerance(want, K_ABS, ref.umax, depth)
        _held(f"absorption {name} E(K-1/2)", abs(float(np.longdouble(s.energy(0)) - want.E)), tol)
        b = bound(K_ABS, ref.umax)
        _held(f"absorption {name} u^K", max_dev(s.global_field(0).numpy(), ref.uK), b)
        _held(f"absorption {name} traces", max_dev(s.traces().numpy(), ref.traces), b)


# ---- refusals and the CLIs -------------------------------------------------------------------------------------------------
def test_refusals():
    C = load()
    for bad, msg in (((-1, 0.0, 63), "width"), ((12, 0.0, 63), "2 * width"), ((4, -1.0, 63), "sigma"),
                     ((4, float("inf"), 63), "sigma"), ((4, 0.0, 64), "faces"), ((4, 0.0, "xq"), "xXyYzZ")):
        with pytest.raises(ValueError, match="sponge"):
            ProblemSpec(N=24, tau=1e-3, K=4, sponge=bad)
    for width, sigma, msg in ((-1, 0.0, "width"), (12, 0.0, "2 \\* width"), (4, -1.0, "sigma"), (4, float("nan"), "sigma")):
        with pytest.raises(RuntimeError, match="sponge: .*" + msg):
            C.Problem(24, 1e-3, 4, 1.0, sponge=C.Sponge(width, sigma, 63))
    assert C.Problem(24, 1e-3, 4, 1.0, sponge=C.Sponge(11, 0.0, 63)).sponge.on  # 2 * 11 <= 23
    assert ProblemSpec(N=24, tau=1e-3, K=4, sponge=(4, None, "xXz")).sponge == (4, 0.0, 0b010011)
    assert ProblemSpec(N=24, tau=1e-3, K=4, sponge=3).sponge == (3, 0.0, 63)
    with pytest.raises(ValueError, match="sponge: faces is empty"):
        ProblemSpec(N=24, tau=1e-3, K=4, sponge=(4, 0.0, ""))
    spec = ProblemSpec(N=24, tau=1e-3, K=4, sponge=(4, 0.0, 63))
    with pytest.raises(ValueError, match="sponge: .*one rank"):
        Solver(spec, backend="cpu", transport="torch", rank=0, world=2)
    with pytest.raises(ValueError, match="sponge:"):
        Solver(spec, backend="torch")
    with pytest.raises(ValueError, match="sponge: .*process"):
        Solver(spec, backend="hip", runtime="process")
    assert Solver(ProblemSpec(N=24, tau=1e-3, K=4), backend="cpu", sponge=(4, 0.0, "x")).spec.sponge == (4, 0.0, 1)


def test_cli_round_trip(tmp_path):
    """--sponge 6,,xXyYz on both CLIs with the CPU backend: the top face (z+) keeps reflecting, the JSON and the dump
    sidecar name the sponge, stderr says once that the error columns have no meaning, and the dumped field is the
    Python Solver's bit for bit; the distributed CPU program and a bad FACES letter are refused."""
    N, K_, tau = 24, 12, 0.01
    phi, psi = lcg_fields(N)
    dumpio.save(str(tmp_path / "ini.phi"), phi, N=N, L=1.0, tau=tau, step=0)
    dumpio.save(str(tmp_path / "ini.psi"), psi, N=N, L=1.0, tau=tau, step=0)
    spec = ProblemSpec(N=N, tau=tau, K=K_, sponge=(6, 0.0, "xXyYz"))
    assert spec.sponge == (6, 0.0, 31)
    s, _ = _cpu(spec, initial=(phi, psi))
    want = s.global_field(0).numpy()
    g = sponge_g(spec, spec.sponge)
    assert (g[8:16, 8:16, N - 5:N] == 0).all() and (g[8:16, 8:16, 1:6] > 0).all()
    for name, cmd in (("py", [sys.executable, "-m", "mpi_cuda_amd", str(N), repr(tau), str(K_), "--backend", "cpu"]),
                      ("native", [CLI, str(N), repr(tau), str(K_), "--cpu", "--threads", "2"])):
        d, j = tmp_path / f"dump_{name}", tmp_path / f"{name}.json"
        r = subprocess.run(cmd + ["--sponge", "6,,xXyYz", "--initial", str(tmp_path / "ini"), "--dump", str(d), "--json",
                                  str(j), "--quiet"], capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stderr.count("error columns") == 1 and "no meaning" in r.stderr
        assert json.loads(j.read_text())["sponge"] == [6, 0.0, 31]
        f, meta = dumpio.load(str(d))
        assert meta["sponge"] == [6, 0.0, 31]
        assert same_bits(f, want), name
        # ... and without --sponge neither file has the key
        r = subprocess.run(cmd + ["--initial", str(tmp_path / "ini"), "--dump", str(d), "--json", str(j), "--quiet"],
                           capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert r.returncode == 0 and "error columns" not in r.stderr
        assert "sponge" not in json.loads(j.read_text()) and "sponge" not in dumpio.load(str(d))[1]
    r = subprocess.run([CLI, str(N), repr(tau), str(K_), "--cpu", "--np", "2", "--sponge", "4"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "sponge: one rank only" in r.stderr
    r = subprocess.run([CLI, str(N), repr(tau), str(K_), "--cpu", "--sponge", "4,,xq"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "xXyYzZ" in r.stderr
    # an empty FACES would switch the sponge off silently: refused on both CLIs
    for cmd in ([CLI, str(N), repr(tau), str(K_), "--cpu"], [sys.executable, "-m", "mpi_cuda_amd", str(N), repr(tau), str(K_),
                                                            "--backend", "cpu"]):
        r = subprocess.run(cmd + ["--sponge", "6,0.5,"], capture_output=True, text=True, timeout=120, cwd=ROOT)
        assert r.returncode != 0 and "FACES is empty" in r.stderr
    r = subprocess.run([CLI, str(N), repr(tau), str(K_), "--cpu", "--sponge", "12"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "sponge:" in r.stderr and "2 * width" in r.stderr
