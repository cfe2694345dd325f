"""Rectangular-box domains (Lx × Ly × Lz, the same N per axis) on the CPU path: the native solver against the
closed-form oracle and the PyTorch reference, cube invariance of the new arithmetic, the box CFL guard, the
multi-process CPU program and the CLI (--box, JSON, dumps, --resume)."""
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from mpi_cuda_amd import ProblemSpec
from mpi_cuda_amd.models.wave3d import oracle_errors, torch_reference_solve
from mpi_cuda_amd.ops import stencil as ops
from mpi_cuda_amd.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "wave3d")
EDGES = (1.0, 1.3, 0.7)
PERMS = [EDGES, (1.3, 0.7, 1.0), (0.7, 1.0, 1.3)]  # the box and its two cyclic permutations


def box_spec(N, K, edges=EDGES, tau=1e-3, check_every=2):
    return ProblemSpec(N=N, tau=tau, K=K, L=edges[0], Ly=edges[1], Lz=edges[2], check_every=check_every)


@pytest.fixture(scope="module", autouse=True)
def cli_built():
    if not os.path.exists(CLI):
        from mpi_cuda_amd._native import load

        load()
        subprocess.run(["python", os.path.join(ROOT, "tools", "build.py")], check=True)
    assert os.path.exists(CLI)


def run(*args, check=True):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, text=True, check=check, timeout=120)


def step_lines(out):
    return [l for l in out.splitlines() if l.startswith("Step ")]


# one native CPU solve per permutation, shared by the oracle and the torch-reference tests
@pytest.fixture(scope="module")
def cpu_runs():
    out = {}
    for e in PERMS:
        s = Solver(box_spec(32, 11, e), backend="cpu")
        out[e] = (s.run(), s.owned_field(0).clone(), s.owned_field(1).clone())
    return out


@pytest.mark.parametrize("edges", PERMS)
def test_cpu_solver_matches_box_oracle(cpu_runs, edges):
    """Native CpuSolver against the closed form with λ_h = 4·sin²(π/(2N))·Σ 1/h_d², rel 1e-6 (the cube's tolerance in
    tests/test_gpu_solver.py). A swapped ry / rz changes λ_h by O(1)."""
    spec = box_spec(32, 11, edges)
    r = cpu_runs[edges][0]
    o = oracle_errors(spec)
    assert r.steps == [2, 4, 6, 8, 10, 11] and sorted(o) == r.steps
    for n, m, e in zip(r.steps, r.max_err, r.rms_err):
        print(n, m, o[n][0], e, o[n][1])
        assert math.isclose(m, o[n][0], rel_tol=1e-6) and math.isclose(e, o[n][1], rel_tol=1e-6)


@pytest.mark.parametrize("edges", PERMS)
def test_torch_reference_agrees_with_native_cpu(cpu_runs, edges):
    """torch_reference_solve (d2sum_torch with the ratios, same operation order) against the native CPU path: as for the
    cube in tests/test_cpu_solver.py, fields bit for bit and the L∞ log exactly."""
    spec = box_spec(32, 11, edges)
    r, uk, ukm1 = cpu_runs[edges]
    errs, tk, tkm1 = torch_reference_solve(spec, return_fields=True)
    assert torch.equal(uk, tk) and torch.equal(ukm1, tkm1)
    for n, m in zip(r.steps, r.max_err):
        assert m == errs[n][0]


def test_cube_invariance(C):
    """A cube spelled with three equal edges is the cube, and the box arithmetic fed ratios of 1 reproduces the cube's
    bits: logs and field(0) bytes."""
    a = Solver(ProblemSpec(N=24, tau=1e-3, K=7, L=2.0), backend="cpu")
    b = Solver(ProblemSpec(N=24, tau=1e-3, K=7, L=2.0, Ly=2.0, Lz=2.0), backend="cpu")
    ra, rb = a.run(), b.run()
    assert ra.steps == rb.steps and ra.max_err == rb.max_err and ra.rms_err == rb.rms_err
    assert a.owned_field(0).numpy().tobytes() == b.owned_field(0).numpy().tobytes()
    sa, sb = ProblemSpec(N=24, tau=1e-3, K=7, L=2.0), ProblemSpec(N=24, tau=1e-3, K=7, L=2.0, Ly=2.0, Lz=2.0)
    assert not sb.is_box and sa.a_t == sb.a_t and sa.courant == sb.courant and sa.tau_max == sb.tau_max
    assert sa.as_dict() == ProblemSpec(N=24, tau=1e-3, K=7, L=2.0).as_dict() and "Ly" not in sa.as_dict()
    assert oracle_errors(sa) == oracle_errors(sb)
    # native Coeffs with the box form forced on: K steps of the CPU kernels, every level and check
    prob = sa.native()
    cube, forced = C.Coeffs.from_problem(prob), C.Coeffs.from_problem(prob, force_box=True)
    assert not cube.box and forced.box and forced.ry == 1.0 and forced.rz == 1.0
    assert (forced.lam, forced.half_lam, forced.ihx2) == (cube.lam, cube.half_lam, cube.ihx2)
    lay = C.make_layout(prob, C.rank_box(prob, C.parse_dims("slab", 1, 24), 0))
    s = ops.sin_table_ext(prob)
    box = C.compute_box(lay)
    fields, logs = [], []
    for co in (cube, forced):
        u0, u1 = ops.alloc_field(lay), ops.alloc_field(lay)
        ops.init_first(lay, co, s, u0, u1)
        log = []
        for n in range(2, 8):
            log.append(ops.leapfrog(lay, co, u1, u0, [box], s, math.cos(prob.a_t * n * prob.tau), check=True))
            u0, u1 = u1, u0
        fields.append((u0, u1))
        logs.append(log)
    assert logs[0] == logs[1]
    assert fields[0][1].numpy().tobytes() == fields[1][1].numpy().tobytes()
    assert fields[0][0].numpy().tobytes() == fields[1][0].numpy().tobytes()
    # (the forced form's u^K is the solver's)
    assert torch.equal(ops.to_grid(lay, fields[1][1])[1:-1, 1:-1, 1:-1], a.owned_field(0))


def test_box_cfl():
    """τ between the box's tau_max and the unit cube's (hz < hx makes the box's smaller): refused for the box, accepted
    for the cube; force overrides; Python and native agree on the Courant number."""
    N = 32
    cube, box = ProblemSpec(N=N, tau=1e-3, K=4, L=1.0), box_spec(N, 4)
    assert box.tau_max < cube.tau_max
    assert math.isclose(box.tau_max, 1.0 / (N * math.sqrt(1 / 1.0 + 1 / 1.69 + 1 / 0.49)), rel_tol=1e-14)
    tau = 0.5 * (box.tau_max + cube.tau_max)
    bad = box_spec(N, 4, tau=tau)
    assert not bad.cfl_ok and ProblemSpec(N=N, tau=tau, K=4, L=1.0).cfl_ok
    with pytest.raises(ValueError, match="CFL"):
        Solver(bad, backend="cpu")
    Solver(ProblemSpec(N=N, tau=tau, K=4, L=1.0), backend="cpu")
    Solver(bad, backend="cpu", force=True)
    for spec in (box, bad, box_spec(130, 4), cube):
        p = spec.native()
        assert spec.courant == p.courant and spec.tau_max == p.tau_max and spec.a_t == p.a_t
        assert spec.is_box == p.is_box and tuple(p.edges) == spec.edges
    assert 3.9e-3 < box_spec(130, 4).tau_max < 4.1e-3
    # the CLI names the box tau_max
    r = run(N, tau, 4, "--cpu", "--box", "1.0,1.3,0.7", check=False)
    assert r.returncode == 2 and "CFL" in r.stderr and f"{bad.tau_max:.3e}" in r.stderr and "1,1.3,0.7" in r.stderr
    assert run(N, tau, 4, 1.0, "--cpu").returncode == 0
    assert run(N, tau, 4, "--cpu", "--box", "1.0,1.3,0.7", "--force", check=False).returncode in (0, 3)


def test_cpu_multiprocess_box_log():
    """--cpu --np 4 --decomp block on a box prints the one-rank log exactly."""
    one = run(48, 0.001, 10, "--cpu", "--box", "1.0,1.3,0.7")
    par = run(48, 0.001, 10, "--cpu", "--np", 4, "--decomp", "block", "--box", "1.0,1.3,0.7")
    assert step_lines(par.stdout) == step_lines(one.stdout) and len(step_lines(one.stdout)) == 5
    assert "max over 4 ranks" in par.stdout
    o = oracle_errors(box_spec(48, 10))
    last = step_lines(one.stdout)[-1]
    assert last == "Step 10, t = 0.010000, Max Error = %e, L2 Error = %e" % o[10]


def test_cli_box(tmp_path):
    """--box with a positional L is an error; the --json line carries the edges; a dump round-trips them; --resume
    with another box is refused; every personality takes --box; cube sidecars without the key still load."""
    r = run(24, 0.001, 4, 2.0, "--cpu", "--box", "1.0,1.3,0.7", check=False)
    assert r.returncode == 2 and "--box" in r.stderr
    for bad in ("1.0,1.3", "1,2,3,4", "1,x,2", "1,-2,3"):
        assert run(24, 0.001, 4, "--cpu", "--box", bad, check=False).returncode == 2
    j, ck = tmp_path / "o.json", tmp_path / "ck"
    run(24, 0.001, 4, "--cpu", "--box", "1.0,1.3,0.7", "--json", j, "--checkpoint", ck, "--check-every", 1)
    rec = json.loads(j.read_text())
    assert rec["box"] == [1.0, 1.3, 0.7] and rec["L"] == 1.0 and rec["N"] == 24
    meta = json.loads((tmp_path / "ck.cur.json").read_text())
    assert meta["box"] == [1.0, 1.3, 0.7] and meta["L"] == 1.0 and meta["step"] == 4
    from mpi_cuda_amd.utils import dump as dumpio

    u, m = dumpio.load(str(ck) + ".cur")
    assert dumpio.box_of(m) == (1.0, 1.3, 0.7)
    _, uk, _ = torch_reference_solve(box_spec(24, 4, check_every=1), return_fields=True)
    assert np.array_equal(u, uk.numpy())
    # the Python writer records the same key, and none for a cube
    dumpio.save(str(tmp_path / "py"), u, N=24, L=1.0, tau=1e-3, step=4, box=(1.0, 1.3, 0.7))
    assert dumpio.box_of(dumpio.load(str(tmp_path / "py"))[1]) == (1.0, 1.3, 0.7)
    dumpio.save(str(tmp_path / "pyc"), u, N=24, L=2.0, tau=1e-3, step=4, box=(2.0, 2.0, 2.0))
    assert "box" not in json.loads((tmp_path / "pyc.json").read_text())
    # resume: the same box continues to the straight run's log; another box, or the cube, is refused
    straight = run(24, 0.001, 8, "--cpu", "--box", "1.0,1.3,0.7", "--check-every", 1)
    cont = run(24, 0.001, 8, "--cpu", "--box", "1.0,1.3,0.7", "--check-every", 1, "--resume", ck)
    assert step_lines(cont.stdout) == step_lines(straight.stdout)[4:]
    for other in (["--box", "1.0,0.7,1.3"], ["--box", "1.0,1.3,0.8"], [1.0], []):
        r = run(24, 0.001, 8, *other, "--cpu", "--resume", ck, check=False)
        assert r.returncode == 1 and "box" in r.stderr, (other, r.stderr)
    # a cube's sidecar has no such key (so cube dumps from before the key existed load as they did), and resumes
    run(24, 0.001, 4, 2.0, "--cpu", "--checkpoint", tmp_path / "cube", "--json", tmp_path / "c.json")
    assert "box" not in json.loads((tmp_path / "cube.cur.json").read_text())
    assert "box" not in json.loads((tmp_path / "c.json").read_text())
    assert run(24, 0.001, 8, 2.0, "--cpu", "--resume", tmp_path / "cube").returncode == 0
    r = run(24, 0.001, 8, "--cpu", "--box", "2.0,2.0,2.5", "--resume", tmp_path / "cube", check=False)
    assert r.returncode == 1 and "box" in r.stderr
    # a personality whose 4th positional is the thread count
    omp = subprocess.run([os.path.join(ROOT, "bin", "wave3dOMP"), "24", "0.001", "4", "2", "--box", "1.0,1.3,0.7",
                          "--check-every", "1"], capture_output=True, text=True, timeout=120)
    if os.path.lexists(os.path.join(ROOT, "bin", "wave3dOMP")):
        assert omp.returncode == 0 and step_lines(omp.stdout) == step_lines(straight.stdout)[:4]


def test_python_cli_box(tmp_path, capsys):
    """python -m mpi_cuda_amd --box: the native CLI's log; --box with a positional L is an error."""
    from mpi_cuda_amd.cli import main

    assert main(["24", "0.001", "4", "--box", "1.0,1.3,0.7", "--backend", "cpu", "--json", str(tmp_path / "p.json"),
                 "--checkpoint", str(tmp_path / "pck")]) == 0
    out = capsys.readouterr().out
    nat = run(24, 0.001, 4, "--cpu", "--box", "1.0,1.3,0.7")
    assert step_lines(out) == step_lines(nat.stdout) and "box=1,1.3,0.7" in out
    assert json.loads((tmp_path / "p.json").read_text())["box"] == [1.0, 1.3, 0.7]
    assert json.loads((tmp_path / "pck.cur.json").read_text())["box"] == [1.0, 1.3, 0.7]
    # the native program resumes the Python checkpoint of the same box and refuses it for another
    assert run(24, 0.001, 6, "--cpu", "--box", "1.0,1.3,0.7", "--resume", tmp_path / "pck").returncode == 0
    assert run(24, 0.001, 6, "--cpu", "--box", "1.3,1.0,0.7", "--resume", tmp_path / "pck", check=False).returncode == 1
    assert main(["24", "0.001", "6", "--box", "1.3,1.0,0.7", "--backend", "cpu", "--resume", str(tmp_path / "pck")]) == 2
    with pytest.raises(SystemExit):
        main(["24", "0.001", "4", "2.0", "--box", "1.0,1.3,0.7", "--backend", "cpu"])


def test_torch_dist_solver_box():
    """parallel/dist_solver.py (through ops/) on a box: the native CPU log and field."""
    from mpi_cuda_amd.parallel.dist_solver import TorchDistSolver

    spec = box_spec(20, 6)
    ref = Solver(spec, backend="cpu")
    rr = ref.run()
    d = TorchDistSolver(spec)
    r = d.run()
    assert r["steps"] == list(rr.steps) and r["max_err"] == list(rr.max_err) and r["rms_err"] == list(rr.rms_err)
    assert torch.equal(d.owned_field(0), ref.owned_field(0))
