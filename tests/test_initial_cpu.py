"""Solve from user-supplied initial data on the CPU path: the first step from stored fields (cpu_first_step_field), the
discrete energy (cpu_energy) against the closed form and as a conserved quantity, CpuSolver.set_initial, and the
--initial / --energy flags of both CLIs.

Tolerances (none fixed in advance):

* two evaluations of the same energy sum differ by at most (D + 8)·2⁻⁵³·Σ|terms|, D the summation depth of the evaluation
  (cpu_energy: its three nested accumulators, nz + ny + nx), Σ|terms| from cpu_energy itself (``abs_terms``);
* against the closed form the fields' own rounding comes on top. Measured here with the CPU solver (K = 20, τ at half
  of tau_max): |E_cpu − E_oracle| / E = 3.6e-16 (N = 16), 2.2e-16 (N = 16 box), 1.922e-15 (N = 33), 2.2e-16 (N = 33 box),
  so at most 1.922e-15·E; the tests allow 4× that on top of the summation bound.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mpi_cuda_amd import ProblemSpec
from mpi_cuda_amd._native import load
from mpi_cuda_amd.models.wave3d import oracle_energy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "wave3d")
BOX = (1.0, 1.3, 0.7)
U = 2.0 ** -53
FIELD_ROUNDING = 1.922e-15  # measured, see the module docstring


def make_spec(N, box=None, K=20):
    kw = dict(Ly=box[1], Lz=box[2]) if box else {}
    tau = 0.5 * ProblemSpec(N=N, L=1.0, **kw).tau_max
    return ProblemSpec(N=N, tau=tau, K=K, L=1.0, **kw)


def layouts(C, prob):
    lay = C.make_layout(prob, C.rank_box(prob, C.Dims(1, 1, 1), 0))
    return lay, C.initial_layout(prob, lay)


def eigenmode(C, prob):
    t = np.asarray(C.sin_table_ext(prob))[1:-1]
    return np.ascontiguousarray((t[:, None, None] * t[None, :, None]) * t[None, None, :])


def random_data(N, seed=20240):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N + 1,) * 3), rng.standard_normal((N + 1,) * 3)


def dense(lay, flat, g):
    """(n + 2g)³ view of a padded local array with g ghost layers (one rank: the whole grid plus ghosts)."""
    rows = np.asarray(flat).reshape(lay.nx + 2 * lay.xg, lay.ny + 2 * lay.yg, lay.pitch)
    z0 = lay.zs + lay.zg - g
    return rows[lay.xg - g: lay.xg + lay.nx + g, lay.yg - g: lay.yg + lay.ny + g, z0: z0 + lay.nz + 2 * g]


@pytest.mark.parametrize("box", [None, BOX], ids=["cube", "box"])
@pytest.mark.parametrize("N", [16, 33])
def test_first_step_field_reproduces_init_first(N, box):
    C = load()
    spec = make_spec(N, box)
    prob = spec.native()
    lay, src = layouts(C, prob)
    c = C.Coeffs.from_problem(prob)
    r0, r1 = np.zeros(lay.total), np.zeros(lay.total)
    C.cpu_init_first(lay, c, C.sin_table_ext(prob), r0, r1)
    u0, u1 = np.full(lay.total, np.nan), np.full(lay.total, np.nan)
    C.cpu_first_step_field(lay, src, c, spec.tau, C.initial_to_local(src, eigenmode(C, prob).reshape(-1)), None, u0, u1)
    assert np.array_equal(u0, r0) and np.array_equal(u1, r1)


@pytest.mark.parametrize("with_psi", [True, False], ids=["psi", "nopsi"])
@pytest.mark.parametrize("box", [None, BOX], ids=["cube", "box"])
@pytest.mark.parametrize("N", [16, 33])
def test_first_step_field_matches_numpy(N, box, with_psi):
    """u¹ = fma(τ, ψ, fma(half_lam, d2sum(φ), φ)) on interior nodes (the ψ fma skipped without ψ), 0 elsewhere; the face
    values of the given arrays are ignored."""
    C = load()
    spec = make_spec(N, box)
    prob = spec.native()
    lay, src = layouts(C, prob)
    c = C.Coeffs.from_problem(prob)
    phi, psi = random_data(N)
    u0, u1 = np.full(lay.total, np.nan), np.full(lay.total, np.nan)
    C.cpu_first_step_field(lay, src, c, spec.tau, C.initial_to_local(src, phi.reshape(-1)),
                           C.initial_to_local(src, psi.reshape(-1)) if with_psi else None, u0, u1)
    f = phi.copy()
    for ax in range(3):
        for side in (0, -1):
            f[(slice(None),) * ax + (side,)] = 0.0
    cc = f[1:-1, 1:-1, 1:-1]
    c2 = 2.0 * cc
    dx = f[2:, 1:-1, 1:-1] - c2 + f[:-2, 1:-1, 1:-1]
    dy = f[1:-1, 2:, 1:-1] - c2 + f[1:-1, :-2, 1:-1]
    dz = f[1:-1, 1:-1, 2:] - c2 + f[1:-1, 1:-1, :-2]
    fma = lambda a, b, d: np.asarray(C.fma_array(np.full(b.size, a), np.ascontiguousarray(b).ravel(),  # noqa: E731
                                                 np.ascontiguousarray(d).ravel())).reshape(b.shape)
    lap = fma(c.rz, dz, fma(c.ry, dy, dx)) if c.box else (dx + dy) + dz
    w = fma(c.half_lam, lap, cc)
    if with_psi:
        w = fma(spec.tau, psi[1:-1, 1:-1, 1:-1], w)
    want1 = np.zeros_like(f)
    want1[1:-1, 1:-1, 1:-1] = w
    assert np.array_equal(dense(lay, u0, 0), f)
    assert np.array_equal(dense(lay, u1, 0), want1)
    # everything else in the allocation (ghosts outside the grid, padding, the zero slot) is an exact 0
    for u, want in ((u0, f), (u1, want1)):
        assert np.count_nonzero(u) == np.count_nonzero(want)
    assert u0[lay.zero_off()] == 0.0 and u1[lay.zero_off()] == 0.0


def test_solver_set_initial_equals_set_state():
    C = load()
    spec = make_spec(33, BOX)
    prob = spec.native()
    lay, src = layouts(C, prob)
    phi, psi = random_data(33)
    u0, u1 = np.zeros(lay.total), np.zeros(lay.total)
    C.cpu_first_step_field(lay, src, C.Coeffs.from_problem(prob), spec.tau, C.initial_to_local(src, phi.reshape(-1)),
                           C.initial_to_local(src, psi.reshape(-1)), u0, u1)
    a = C.CpuSolver(prob, 2, 2)
    a.set_initial(phi.reshape(-1), psi.reshape(-1))
    ra = a.run()
    b = C.CpuSolver(prob, 2, 2)
    b.set_state(np.ascontiguousarray(dense(lay, u0, 0)).reshape(-1), np.ascontiguousarray(dense(lay, u1, 0)).reshape(-1), 1)
    rb = b.run()
    assert np.array_equal(a.field(0), b.field(0)) and np.array_equal(a.field(1), b.field(1))
    assert ra["steps"] == rb["steps"] and ra["max_err"] == rb["max_err"]
    # set_state replaces the initial data again, and the other way round
    a.set_state(np.ascontiguousarray(dense(lay, u0, 0)).reshape(-1), np.ascontiguousarray(dense(lay, u1, 0)).reshape(-1), 1)
    a.run()
    with pytest.raises(RuntimeError, match="set_initial"):
        a.energy(1)
    with pytest.raises(RuntimeError, match=r"resume step must be in \[1, K\)"):
        C.CpuSolver(make_spec(16, K=1).native(), 2, 1).set_initial(np.zeros(17 ** 3), None)


@pytest.mark.parametrize("box", [None, BOX], ids=["cube", "box"])
@pytest.mark.parametrize("N", [16, 33])
def test_energy_of_the_eigenmode_matches_the_closed_form(N, box):
    C = load()
    spec = make_spec(N, box)
    prob = spec.native()
    lay, _ = layouts(C, prob)
    s = C.CpuSolver(prob, 2, 2)
    s.run()
    e = C.cpu_energy(prob, lay, s.field(1), s.field(0))
    assert e["depth"] == 3 * (N + 1) and e["E"] == s.energy(0)
    want = oracle_energy(spec, spec.K - 1)
    assert oracle_energy(spec, 0) == pytest.approx(want, rel=1e-13)  # (the closed form does not depend on n)
    tol = (e["depth"] + 8) * U * e["abs_terms"] + 4 * FIELD_ROUNDING * want
    print(f"N={N} box={box}: E={e['E']!r} oracle={want!r} diff={e['E'] - want:.3e} tol={tol:.3e}")
    assert abs(e["E"] - want) <= tol
    # the same data handed in as initial data: the same energy at the start and at the end
    s.set_initial(eigenmode(C, prob).reshape(-1), None)
    s.run()
    assert s.energy(0) == e["E"]
    assert abs(s.energy(1) - want) <= tol


def test_energy_is_conserved_on_random_data():
    C = load()
    spec = make_spec(33)
    prob = spec.native()
    lay, _ = layouts(C, prob)
    phi, psi = random_data(33)
    s = C.CpuSolver(prob, 2, 2)
    s.set_initial(phi.reshape(-1), psi.reshape(-1))
    s.run()
    e = C.cpu_energy(prob, lay, s.field(1), s.field(0))
    e1, ek = s.energy(1), s.energy(0)
    tol = (e["depth"] + 8) * U * e["abs_terms"]
    print(f"E(1/2)={e1!r} E(K-1/2)={ek!r} diff={ek - e1:.3e} tol={tol:.3e}")
    assert ek == e["E"] and e1 > 0
    assert abs(ek - e1) <= tol


# ---------------------------------------------------------------------------------------------------------------
# CLIs
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_built():
    if not os.path.exists(CLI):
        load()
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build.py")], check=True)
    assert os.path.exists(CLI)


def native(*args):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, timeout=120)


def pycli(*args):
    return subprocess.run([sys.executable, "-m", "mpi_cuda_amd", *map(str, args)], cwd=ROOT, capture_output=True,
                          text=True, timeout=300)


def test_cli_round_trip_and_refusals(tmp_path, cli_built):
    from mpi_cuda_amd.solver import Solver
    from mpi_cuda_amd.utils import dump as dumpio

    spec = make_spec(33, BOX)
    box = ",".join(map(str, BOX))
    phi, psi = random_data(33)
    pre = str(tmp_path / "ini")
    for part, f in (("phi", phi), ("psi", psi)):
        dumpio.save(f"{pre}.{part}", f, N=33, L=1.0, tau=spec.tau, step=0, box=BOX)
    js = tmp_path / "o.json"
    rn = native(33, repr(spec.tau), 20, "--box", box, "--cpu", "--initial", pre, "--energy", "--json", js)
    assert rn.returncode == 0, rn.stderr
    rp = pycli(33, repr(spec.tau), 20, "--box", box, "--backend", "cpu", "--initial", pre, "--energy")
    assert rp.returncode == 0, rp.stderr
    line = [l for l in rn.stdout.splitlines() if l.startswith("Energy: ")]
    assert len(line) == 1 and line == [l for l in rp.stdout.splitlines() if l.startswith("Energy: ")]
    s = Solver(spec, backend="cpu")
    s.set_initial(phi, psi)
    s.run()
    e1, ek = s.energy(1), s.energy(0)
    assert line[0] == f"Energy: E(1/2) = {e1:.15e}, E(K-1/2) = {ek:.15e}, drift = {abs(ek - e1) / e1:.3e}"
    rec = json.loads(js.read_text())
    assert rec["energy_start"] == e1 and rec["energy_end"] == ek
    # without the flags neither the line nor the keys appear
    plain = native(33, repr(spec.tau), 20, "--box", box, "--cpu", "--json", js)
    assert "Energy:" not in plain.stdout and "energy_start" not in json.loads(js.read_text())
    # no PREFIX.psi: u_t(.,0) = 0
    psi_meta = open(pre + ".psi.json").read()
    os.remove(pre + ".psi.bin"), os.remove(pre + ".psi.json")
    r0 = native(33, repr(spec.tau), 20, "--box", box, "--cpu", "--initial", pre, "--energy")
    s.set_initial(phi)
    s.run()
    assert f"E(1/2) = {s.energy(1):.15e}" in r0.stdout
    # a PREFIX.psi sidecar without its data is an error, not "no psi"
    open(pre + ".psi.json", "w").write(psi_meta)
    assert pycli(33, repr(spec.tau), 20, "--box", box, "--backend", "cpu", "--initial", pre).returncode != 0
    assert native(33, repr(spec.tau), 20, "--box", box, "--cpu", "--initial", pre).returncode == 1
    os.remove(pre + ".psi.json")
    # refusals, modelled on --resume's: another N, another box
    r = native(32, repr(spec.tau), 20, "--box", box, "--cpu", "--initial", pre)
    assert r.returncode == 1 and "initial: dump N differs from the run's N" in r.stderr
    r = native(33, repr(spec.tau), 20, "--box", "1.0,0.7,1.3", "--cpu", "--initial", pre)
    assert r.returncode == 1 and "initial: dump box differs from the run's box" in r.stderr
    r = pycli(32, repr(spec.tau), 20, "--box", box, "--backend", "cpu", "--initial", pre)
    assert r.returncode == 2 and "initial: dump N = 33 differs from the run's 32" in r.stderr
    r = pycli(33, repr(spec.tau), 20, "--box", "1.0,0.7,1.3", "--backend", "cpu", "--initial", pre)
    assert r.returncode == 2 and "initial: dump box" in r.stderr
    assert native(33, repr(spec.tau), 20, "--cpu", "--initial", pre, "--resume", pre).returncode == 2


def test_python_solver_refusals():
    from mpi_cuda_amd.solver import Solver

    spec = make_spec(16)
    s = Solver.__new__(Solver)  # (a process-runtime solver without its rank process: the refusal comes first)
    s.spec, s.backend, s.transport, s.runtime, s.world = spec, "hip", "rccl", "process", 1
    with pytest.raises(ValueError, match="runtime='process' has no initial data from Python"):
        s.set_initial(np.zeros((17, 17, 17)))
    with pytest.raises(ValueError, match="runtime='process' has no energy from Python"):
        s.energy()
    c = Solver(spec, backend="cpu")
    with pytest.raises(ValueError, match="expected a global"):
        c.set_initial(np.zeros((16, 16, 16)))
    with pytest.raises(ValueError, match="needs the native hip or cpu backend"):
        Solver(spec, backend="torch").set_initial(np.zeros((17, 17, 17)))
