"""Solve from user-supplied initial data on the GPU: k_first_step_field against the CPU path bit for bit (one rank and
rank layouts with deep ghosts), solves started by set_initial against set_state and the CPU solver, in-process groups,
graph capture / run_batch pipelining, and k_energy.

Shapes: N = 40, 77 (odd: the pairs start misaligned), 130 (more than one tile per axis), as tests/test_gpu_kernels.py.

Energy tolerances (none fixed in advance):

* two evaluations of the same sum differ by at most (D + 8)·2⁻⁵³·Σ|terms|: D = gpu_energy_depth(layout), the documented
  depth of k_energy's reduction tree; Σ|terms| from cpu_energy on the same fields (``abs_terms``);
* against the closed form the fields' own rounding comes on top. Measured with the CPU solver (K = 20, τ at half of
  tau_max, cube / box 1,1.3,0.7): |E_cpu − E_oracle| / E = 2.3e-15 / 0 (N = 40), 2.3e-15 / 2.2e-16 (N = 77),
  2.520e-15 / 4.4e-16 (N = 130), so at most 2.520e-15·E; the test allows 4× that on top of the summation bound;
* drift |E(K−1/2) − E(1/2)| / E(1/2) of the seeded random solve at N = 77: the CPU solver's own drift at the same shape
  is measured in the test (profiles/initial/README.md records it: 1.246e-16, one ulp of E), and the GPU solve's drift
  must stay within 4× it (the fields are bit-identical: any excess is the energy kernel's). Only if the CPU's two
  energies came out equal to the bit, a drift of 0, would one ulp of E stand in for it: a difference of two fp64
  numbers of size E cannot be resolved below that.
"""
import functools

import numpy as np
import pytest
import torch

from mpi_cuda_amd import ProblemSpec
from mpi_cuda_amd.models.wave3d import oracle_energy
from mpi_cuda_amd.solver import Solver

pytestmark = pytest.mark.gpu
BOX = (1.0, 1.3, 0.7)
U = 2.0 ** -53
FIELD_ROUNDING = 2.520e-15  # measured, see the module docstring
K = 20


def _C():
    from mpi_cuda_amd._native import load

    return load()


def make_spec(N, box=None, K_=K):
    kw = dict(Ly=box[1], Lz=box[2]) if box else {}
    return ProblemSpec(N=N, tau=0.5 * ProblemSpec(N=N, L=1.0, **kw).tau_max, K=K_, L=1.0, **kw)


@functools.lru_cache(maxsize=None)
def random_data(N, seed=20240):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N + 1,) * 3), rng.standard_normal((N + 1,) * 3)


def eigenmode(prob):
    t = np.asarray(_C().sin_table_ext(prob))[1:-1]
    return np.ascontiguousarray((t[:, None, None] * t[None, :, None]) * t[None, None, :])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _kernel_case(prob, tau, lay, phi, psi):
    """k_first_step_field and cpu_first_step_field on `lay`: (gpu u0, gpu u1, cpu u0, cpu u1) as numpy arrays."""
    C = _C()
    src = C.initial_layout(prob, lay)
    co = C.Coeffs.from_problem(prob)
    f = C.initial_to_local(src, phi.reshape(-1))
    p = None if psi is None else C.initial_to_local(src, psi.reshape(-1))
    c0, c1 = np.full(lay.total, np.nan), np.full(lay.total, np.nan)
    C.cpu_first_step_field(lay, src, co, tau, f, p, c0, c1)
    dev = torch.device("cuda", 0)
    df = torch.from_numpy(np.asarray(f)).to(dev)
    dp = None if p is None else torch.from_numpy(np.asarray(p)).to(dev)
    g0 = torch.full((lay.total,), float("nan"), dtype=torch.float64, device=dev)
    g1 = torch.full((lay.total,), float("nan"), dtype=torch.float64, device=dev)
    C.gpu_first_step_field(lay, src, co, tau, df.data_ptr(), 0 if dp is None else dp.data_ptr(), g0.data_ptr(),
                           g1.data_ptr(), _stream())
    torch.cuda.synchronize()
    return g0.cpu().numpy(), g1.cpu().numpy(), c0, c1


@pytest.mark.parametrize("with_psi", [True, False], ids=["psi", "nopsi"])
@pytest.mark.parametrize("box", [None, BOX], ids=["cube", "box"])
@pytest.mark.parametrize("N", [40, 77, 130])
def test_first_step_kernel_one_rank(gpu, N, box, with_psi):
    C = _C()
    spec = make_spec(N, box)
    prob = spec.native()
    lay = C.make_layout(prob, C.rank_box(prob, C.Dims(1, 1, 1), 0))
    phi, psi = random_data(N)
    g0, g1, c0, c1 = _kernel_case(prob, spec.tau, lay, phi, psi if with_psi else None)
    assert np.array_equal(g0, c0) and np.array_equal(g1, c1)  # ghosts, boundary, padding and the zero slot included
    assert g0[lay.zero_off()] == 0.0 and g1[lay.zero_off()] == 0.0 and np.count_nonzero(c1) > (N - 1) ** 3 // 2
    if not with_psi:  # the eigenmode array: init_first's u¹ bit for bit
        e0, e1, _, _ = _kernel_case(prob, spec.tau, lay, eigenmode(prob), None)
        r0, r1 = np.zeros(lay.total), np.zeros(lay.total)
        C.cpu_init_first(lay, C.Coeffs.from_problem(prob), C.sin_table_ext(prob), r0, r1)
        assert np.array_equal(e0, r0) and np.array_equal(e1, r1)


@pytest.mark.parametrize("dims,rank,depth", [((2, 2, 2), 3, (5, 5, 5)), ((4, 1, 1), 1, (5, 1, 1))],
                         ids=["block-rank3-g5", "slab-middle-xg5"])
@pytest.mark.parametrize("box", [None, BOX], ids=["cube", "box"])
def test_first_step_kernel_rank_layouts(gpu, dims, rank, depth, box):
    C = _C()
    N = 77
    spec = make_spec(N, box)
    prob = spec.native()
    lay = C.make_layout(prob, C.rank_box(prob, C.Dims(*dims), rank), 16, *depth)
    phi, psi = random_data(N)
    g0, g1, c0, c1 = _kernel_case(prob, spec.tau, lay, phi, psi)
    assert np.array_equal(g0, c0) and np.array_equal(g1, c1)
    # u⁰ on every owned and ghost node is the global φ (faces zeroed): the neighbours' values in the ghosts, 0 outside
    f = np.zeros((N + 1 + 2 * 5,) * 3)
    f[6:-6, 6:-6, 6:-6] = phi[1:-1, 1:-1, 1:-1]
    xg, yg, zg = depth
    rows = g0.reshape(lay.nx + 2 * xg, lay.ny + 2 * yg, lay.pitch)[:, :, lay.zs: lay.zs + lay.nz + 2 * zg]
    want = f[5 + lay.gx0 - xg: 5 + lay.gx0 + lay.nx + xg, 5 + lay.gy0 - yg: 5 + lay.gy0 + lay.ny + yg,
             5 + lay.gz0 - zg: 5 + lay.gz0 + lay.nz + zg]
    assert np.array_equal(rows, want)
    assert np.count_nonzero(g0) == np.count_nonzero(want) and g1[lay.zero_off()] == 0.0


# ---------------------------------------------------------------------------------------------------------------
# solves
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cpu_solve(N=77):
    """The CPU solver's solve of the seeded random data: (u¹ as a global array, u^K, u^{K−1} owned fields, E(1/2),
    E(K−1/2))."""
    C = _C()
    spec = make_spec(N)
    prob = spec.native()
    phi, psi = random_data(N)
    lay = C.make_layout(prob, C.rank_box(prob, C.Dims(1, 1, 1), 0))
    src = C.initial_layout(prob, lay)
    u0, u1 = np.zeros(lay.total), np.zeros(lay.total)
    C.cpu_first_step_field(lay, src, C.Coeffs.from_problem(prob), spec.tau, C.initial_to_local(src, phi.reshape(-1)),
                           C.initial_to_local(src, psi.reshape(-1)), u0, u1)
    dense = lambda u: np.ascontiguousarray(  # noqa: E731
        u.reshape(lay.nx + 2, lay.ny + 2, lay.pitch)[1:-1, 1:-1, lay.zs + 1: lay.zs + 1 + lay.nz])
    c = Solver(spec, backend="cpu")
    c.set_initial(phi, psi)
    c.run()
    return dict(u0=dense(u0), u1=dense(u1), uK=c.owned_field(0), uK1=c.owned_field(1), e1=c.energy(1), eK=c.energy(0))


@pytest.mark.parametrize("temporal", [5, 4])
def test_solve_equals_set_state_and_cpu(gpu, temporal):
    N = 77
    spec = make_spec(N)
    phi, psi = random_data(N)
    ref = cpu_solve(N)
    a = Solver(spec, backend="hip", device=0, temporal=temporal)
    a.set_initial(phi, psi)
    a.run()
    b = Solver(spec, backend="hip", device=0, temporal=temporal)
    b.set_state(ref["u0"], ref["u1"], 1)
    b.run()
    assert a.native.mode == b.native.mode
    for which in (0, 1):
        assert a.field_hash(which) == b.field_hash(which)
    assert torch.equal(a.owned_field(0), ref["uK"]) and torch.equal(a.owned_field(1), ref["uK1"])
    # set_state replaces the initial data, set_initial replaces the loaded state
    a.set_state(ref["u0"], ref["u1"], 1)
    a.run()
    assert a.field_hash(0) == b.field_hash(0)
    with pytest.raises(RuntimeError, match="set_initial"):
        a.energy(1)
    b.set_initial(phi, psi)
    for which in (0, 1):  # (the retained fields and the E(1/2) slot are an older start's)
        with pytest.raises(RuntimeError, match="no solve has run yet"):
            b.energy(which)
    b.run()
    assert b.field_hash(0) == a.field_hash(0) and b.energy(1) > 0


@pytest.mark.parametrize("world,decomp", [(2, "slab"), (8, "2x2x2")])
@pytest.mark.parametrize("temporal", [5, 4])
def test_group_equals_one_rank(gpu, world, decomp, temporal):
    N = 77
    spec = make_spec(N)
    phi, psi = random_data(N)
    one = Solver(spec, backend="hip", device=0, temporal=temporal)
    one.set_initial(phi, psi)
    one.run()
    g = Solver(spec, backend="hip", transport="loopback", world=world, rank=0, decomp=decomp, device=0,
               temporal=temporal)
    g.set_initial(phi, psi)
    for _ in range(2):  # (the second group solve is the captured one where the runtime captures groups)
        g.run()
        for which in (0, 1):
            assert g.field_hash(which) == one.field_hash(which)
    assert torch.equal(g.global_field(0), cpu_solve(N)["uK"])
    # energy of a group: cpu_energy on the assembled global fields = the CPU solver's
    assert g.energy(0) == cpu_solve(N)["eK"] and g.energy(1) == cpu_solve(N)["e1"]
    g.set_state(cpu_solve(N)["u0"], cpu_solve(N)["u1"], 1)  # (the loaded state takes the initial data's place)
    with pytest.raises(ValueError, match="set_initial"):
        g.energy(1)


@pytest.mark.parametrize("box", [None, BOX], ids=["cube", "box"])
def test_eigenmode_through_set_initial_is_the_default_solve(gpu, box):
    N = 77
    spec = make_spec(N, box)
    d = Solver(spec, backend="hip", device=0)
    rd = d.run()
    s = Solver(spec, backend="hip", device=0)
    s.set_initial(eigenmode(spec.native()))
    rs = s.run()
    print("default", rd.max_err, rd.rms_err, "\ninitial", rs.max_err, rs.rms_err)
    assert rs.steps == rd.steps and rs.max_err == rd.max_err and rs.rms_err == rd.rms_err
    assert s.field_hash(0) == d.field_hash(0) and s.field_hash(1) == d.field_hash(1)


def test_graph_and_batch(gpu):
    N = 77
    spec = make_spec(N)
    phi, psi = random_data(N)
    d = Solver(spec, backend="hip", device=0)
    d.run()
    s = Solver(spec, backend="hip", device=0)
    s.set_initial(phi, psi)
    hashes, energies = [], []
    for _ in range(3):
        s.run()
        hashes.append((s.field_hash(0), s.field_hash(1)))
        energies.append((s.energy(1), s.energy(0)))
    assert len(set(hashes)) == 1 and len(set(energies)) == 1
    assert s.native.graph_enabled == d.native.graph_enabled
    bd, bs = d.run_batch(3), s.run_batch(3)
    assert [r.extra["batched"] for r in bs] == [r.extra["batched"] for r in bd]
    assert all(r.max_err == bs[0].max_err for r in bs)
    assert (s.field_hash(0), s.field_hash(1)) == hashes[0]
    assert s.native.device_bytes() > d.native.device_bytes()


# ---------------------------------------------------------------------------------------------------------------
# k_energy
# ---------------------------------------------------------------------------------------------------------------
def _cpu_energy_of(s):
    C = _C()
    return C.cpu_energy(s.spec.native(), s.native.layout, s.native.download(1), s.native.download(0))


@pytest.mark.parametrize("box", [None, BOX], ids=["cube", "box"])
@pytest.mark.parametrize("N", [40, 77, 130])
def test_energy_of_the_eigenmode(gpu, N, box):
    spec = make_spec(N, box)
    s = Solver(spec, backend="hip", device=0)
    s.run()
    e = s.energy(0)
    assert s.energy(0) == e  # two calls: identical bits
    c = _cpu_energy_of(s)
    D = _C().gpu_energy_depth(s.native.layout)
    tol = (D + 8) * U * c["abs_terms"]
    want = oracle_energy(spec, K - 1)
    print(f"N={N} box={box}: D={D} E_gpu={e!r} E_cpu={c['E']!r} oracle={want!r} gpu-cpu={e - c['E']:.3e} tol={tol:.3e} "
          f"gpu-oracle={e - want:.3e}")
    assert abs(e - c["E"]) <= tol
    assert abs(e - want) <= tol + 4 * FIELD_ROUNDING * want


def test_energy_of_random_data(gpu):
    N = 77
    spec = make_spec(N)
    phi, psi = random_data(N)
    ref = cpu_solve(N)
    s = Solver(spec, backend="hip", device=0)
    s.set_initial(phi, psi)
    s.run()
    e1, eK = s.energy(1), s.energy(0)
    assert (s.energy(1), s.energy(0)) == (e1, eK)
    c = _cpu_energy_of(s)
    D = _C().gpu_energy_depth(s.native.layout)
    tol = (D + 8) * U * c["abs_terms"]
    cpu_drift = abs(ref["eK"] - ref["e1"]) / ref["e1"]
    drift = abs(eK - e1) / e1
    print(f"D={D} E(1/2): gpu {e1!r} cpu {ref['e1']!r}; E(K-1/2): gpu {eK!r} cpu {ref['eK']!r}; tol={tol:.3e}; drift gpu "
          f"{drift:.3e} cpu {cpu_drift:.3e}")
    assert c["E"] == ref["eK"]  # (bit-identical fields)
    assert abs(eK - ref["eK"]) <= tol and abs(e1 - ref["e1"]) <= tol
    assert abs(eK - e1) <= tol
    assert drift <= 4 * (cpu_drift if cpu_drift > 0 else np.spacing(ref["e1"]) / ref["e1"])


def test_energy_refusals(gpu):
    C = _C()
    spec = make_spec(40)
    s = Solver(spec, backend="hip", device=0)
    with pytest.raises(RuntimeError, match="no solve has run yet"):
        s.energy(0)
    s.run()
    with pytest.raises(RuntimeError, match="set_initial"):
        s.energy(1)
    o = C.SolverOptions()
    o.fake_comm = True
    r = C.GpuSolver(spec.native(), o, 0, 2, None)  # (a rank of a two-rank job, no transport)
    with pytest.raises(RuntimeError, match=r"energy: one rank only \(multi-rank: Solver.energy assembles the global fields\)"):
        r.energy(0)
    with pytest.raises(RuntimeError, match=r"resume step must be in \[1, K\)"):
        Solver(make_spec(40, K_=1), backend="hip", device=0).set_initial(np.zeros((41,) * 3))


def test_native_cli_initial_and_energy(gpu, tmp_path):
    """bin/wave3d N tau K --initial PREFIX --energy on the GPU prints the in-process solver's energies; a group takes
    --initial too."""
    import json
    import os
    import subprocess

    from mpi_cuda_amd.utils import dump as dumpio

    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "wave3d")
    N = 40
    spec = make_spec(N)
    phi, psi = random_data(N)
    pre = str(tmp_path / "ini")
    for part, f in (("phi", phi), ("psi", psi)):
        dumpio.save(f"{pre}.{part}", f, N=N, L=1.0, tau=spec.tau, step=0)
    s = Solver(spec, backend="hip", device=0)
    s.set_initial(phi, psi)
    s.run()
    e1, ek = s.energy(1), s.energy(0)
    js = tmp_path / "o.json"
    r = subprocess.run([cli, str(N), repr(spec.tau), str(K), "--initial", pre, "--energy", "--json", str(js), "--repeat",
                        "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"Energy: E(1/2) = {e1:.15e}, E(K-1/2) = {ek:.15e}, drift = {abs(ek - e1) / e1:.3e}" in r.stdout.splitlines()
    rec = json.loads(js.read_text())
    assert rec["energy_start"] == e1 and rec["energy_end"] == ek and rec["graph"] is True
    g = subprocess.run([cli, str(N), repr(spec.tau), str(K), "--initial", pre, "--group", "2", "--group-transport",
                        "loopback", "--dump", str(tmp_path / "g")], capture_output=True, text=True, timeout=120)
    assert g.returncode == 0, g.stderr
    u, _ = dumpio.load(str(tmp_path / "g"))
    assert np.array_equal(u, s.global_field(0).numpy())
