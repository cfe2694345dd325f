"""Rectangular-box domains on the GPU: every update kernel's box form against the native CPU box steps (bit for bit,
the pattern of tests/test_gpu_kernels.py), the box kernels fed ratios of 1 against the cube kernels, the solver against
the CPU backend and the oracle, decomposition invariance, and the rank-process runtime.

Box throughout: edges (1.0, 1.3, 0.7), τ = 1e-3 — the ratios 1/1.69 and 1/0.49 are not representable, so a wrong
operation order shows in the bits."""
import functools
import math

import pytest
import torch

from mpi_cuda_amd import ProblemSpec
from mpi_cuda_amd.models.wave3d import oracle_errors
from mpi_cuda_amd.ops import stencil as ops
from mpi_cuda_amd.solver import Solver

pytestmark = pytest.mark.gpu

EDGES = (1.0, 1.3, 0.7)
SHAPES = [40, 77, 130]  # a remainder tile, an odd extent, more than four tiles


def _C():
    from mpi_cuda_amd._native import load

    return load()


def box_spec(N, K=11, check_every=2):
    return ProblemSpec(N=N, tau=1e-3, K=K, L=EDGES[0], Ly=EDGES[1], Lz=EDGES[2], check_every=check_every)


def _setup(N, world=1, rank=0, decomp="slab", forced_cube=False):
    """(problem, coeffs, layout): the box, or (forced_cube) the unit cube with the box form forced on."""
    C = _C()
    prob = C.Problem(N, 1e-3, 20, 1.0) if forced_cube else C.Problem(N, 1e-3, 20, EDGES[0], Ly=EDGES[1], Lz=EDGES[2])
    co = C.Coeffs.from_problem(prob, force_box=forced_cube)
    assert co.box and (forced_cube or (co.ry != 1.0 and co.rz != 1.0))
    lay = C.make_layout(prob, C.rank_box(prob, C.parse_dims(decomp, world, N), rank))
    return prob, co, lay


def _rand_interior(lay, seed):
    torch.manual_seed(seed)
    g = torch.zeros((int(lay.nx) + 2, int(lay.ny) + 2, int(lay.nz) + 2), dtype=torch.float64)
    g[2:-2, 2:-2, 2:-2] = torch.randn(int(lay.nx) - 2, int(lay.ny) - 2, int(lay.nz) - 2, dtype=torch.float64)
    return ops.from_grid(lay, g)


def _cts(prob, n0, stages):
    return [math.cos(prob.a_t * (n0 + k) * prob.tau) for k in range(1, stages + 1)]


# ---- CPU references, computed once per shape and shared (5 native box steps; prefixes serve the shorter passes)
@functools.lru_cache(maxsize=None)
def _cpu_pass_ref(N):
    """Random u^{n−1}, u^n and the levels u^{n+1..n+5} of the native CPU box steps with their checks."""
    C = _C()
    prob, co, lay = _setup(N)
    box = C.compute_box(lay)
    prev, cur = _rand_interior(lay, N * 13 + 1), _rand_interior(lay, N * 17 + 2)
    s = ops.sin_table_ext(prob)
    ct = _cts(prob, 5, 5)
    a, b = prev.clone(), cur.clone()
    levels, errs = [], []
    for k in range(1, 6):
        errs.append(ops.leapfrog(lay, co, b, a, [box], s, ct[k - 1], check=True))
        a, b = b, a
        levels.append(ops.to_grid(lay, b).clone())
    return prev, cur, levels, errs, ct


@functools.lru_cache(maxsize=None)
def _cpu_start_ref(N):
    """u⁰, u¹ of cpu_init_first and u^2..u^5 of the native CPU box steps (the analytic start's reference)."""
    C = _C()
    prob, co, lay = _setup(N)
    box = C.compute_box(lay)
    s = ops.sin_table_ext(prob)
    u0, u1 = ops.alloc_field(lay), ops.alloc_field(lay)
    ops.init_first(lay, co, s, u0, u1)
    ct = _cts(prob, 1, 4)
    a, b = u0.clone(), u1.clone()
    levels, errs = [], []
    for k in range(1, 5):
        errs.append(ops.leapfrog(lay, co, b, a, [box], s, ct[k - 1], check=True))
        a, b = b, a
        levels.append(ops.to_grid(lay, b).clone())
    return u0, u1, levels, errs, ct


def _run_pass(lay, co, prob, prev, cur, stages, ct, p2, chunked, analytic=False, threads=1024):
    C = _C()
    box = C.compute_box(lay)
    o1 = torch.zeros(int(lay.total), dtype=torch.float64, device="cuda")
    o2 = torch.zeros_like(o1)
    s = ops.sin_table_ext(prob).cuda()
    e = ops.leapfrog_tb(lay, co, None if analytic else prev.cuda(), None if analytic else cur.cuda(), o1, o2, box, s,
                        stages, ct[:stages], (1 << stages) - 1, threads, analytic_start=analytic, p2=p2,
                        target_blocks=256 if chunked else 1)
    torch.cuda.synchronize()
    return ops.to_grid(lay, o1.cpu()), ops.to_grid(lay, o2.cpu()), e


def _check_pass(out, levels, errs, stages, inner=False):
    g1, g2, e = out
    sl = (slice(1, -1),) * 3 if inner else (slice(None),) * 3
    assert torch.equal(g1[sl], levels[stages - 2][sl])
    assert torch.equal(g2[sl], levels[stages - 1][sl])
    assert sorted(e) == list(range(1, stages + 1))
    for k in e:
        assert e[k][0] == errs[k - 1][0]
        assert math.isclose(e[k][1], errs[k - 1][1], rel_tol=1e-12)


# ---- 8. kernel level, bit for bit
@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("N", SHAPES)
@pytest.mark.parametrize("stages", [2, 3, 4, 5])
def test_p2_box_pass_equals_cpu_box_steps(gpu, stages, N, chunked):
    prob, co, lay = _setup(N)
    assert gpu.gpu_leapfrog_p2_supported(lay, gpu.compute_box(lay), stages)
    prev, cur, levels, errs, ct = _cpu_pass_ref(N)
    _check_pass(_run_pass(lay, co, prob, prev, cur, stages, ct, True, chunked), levels, errs, stages)


@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("N", SHAPES)
@pytest.mark.parametrize("stages", [2, 3, 4])
def test_p2_box_analytic_start_equals_cpu_box_steps(gpu, stages, N, chunked):
    prob, co, lay = _setup(N)
    _, _, levels, errs, ct = _cpu_start_ref(N)
    out = _run_pass(lay, co, prob, None, None, stages, ct, True, chunked, analytic=True)
    # (u⁰ = φ also fills the ghosts of the CPU buffers; the pass writes the interior only)
    _check_pass(out, levels, errs, stages, inner=True)


@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("N", SHAPES)
@pytest.mark.parametrize("stages", [2, 3, 4])
def test_tb_box_pass_equals_cpu_box_steps(gpu, stages, N, chunked):
    prob, co, lay = _setup(N)
    prev, cur, levels, errs, ct = _cpu_pass_ref(N)
    _check_pass(_run_pass(lay, co, prob, prev, cur, stages, ct, False, chunked), levels, errs, stages)


@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("N", SHAPES)
@pytest.mark.parametrize("stages", [2, 3, 4])
def test_tb_box_analytic_start_equals_cpu_box_steps(gpu, stages, N, chunked):
    prob, co, lay = _setup(N)
    _, _, levels, errs, ct = _cpu_start_ref(N)
    out = _run_pass(lay, co, prob, None, None, stages, ct, False, chunked, analytic=True)
    _check_pass(out, levels, errs, stages, inner=True)


def test_tb_box_768_threads(gpu):
    """The 768-thread workgroups of k_leapfrog_tb (the analytic start's default size) at one shape."""
    prob, co, lay = _setup(77)
    prev, cur, levels, errs, ct = _cpu_pass_ref(77)
    _check_pass(_run_pass(lay, co, prob, prev, cur, 4, ct, False, False, threads=768), levels, errs, 4)


def test_leapfrog2_box(gpu):
    """k_leapfrog2_rq: the two-step register-queue pass == two CPU box steps."""
    prob, co, lay = _setup(77)
    prev, cur, levels, errs, ct = _cpu_pass_ref(77)
    o1 = torch.zeros(int(lay.total), dtype=torch.float64, device="cuda")
    o2 = torch.zeros_like(o1)
    e = ops.leapfrog2(lay, co, prev.cuda(), cur.cuda(), o1, o2, gpu.compute_box(lay), ops.sin_table_ext(prob).cuda(),
                      ct[1], check=True)
    torch.cuda.synchronize()
    assert torch.equal(ops.to_grid(lay, o1.cpu()), levels[0])
    assert torch.equal(ops.to_grid(lay, o2.cpu()), levels[1])
    assert e[0] == errs[1][0] and math.isclose(e[1], errs[1][1], rel_tol=1e-12)


@pytest.mark.parametrize("tiling", [dict(variant=1, rows=4), dict(variant=0, ty=8)])
def test_single_step_box(gpu, tiling):
    """The single-step kernels (both variants): one step on random fields, ghosts included, on a block rank."""
    C = gpu
    prob, co, lay = _setup(70, 8, 3, "block")
    torch.manual_seed(70)
    cur = torch.randn(int(lay.total), dtype=torch.float64)
    old = torch.randn(int(lay.total), dtype=torch.float64)
    box = C.compute_box(lay)
    s = ops.sin_table_ext(prob)
    ct = math.cos(prob.a_t * 5 * prob.tau)
    old_cpu = old.clone()
    e_cpu = ops.leapfrog(lay, co, cur, old_cpu, [box], s, ct, check=True)
    t = C.LeapfrogTiling()
    for k, v in tiling.items():
        setattr(t, k, v)
    old_g = old.cuda()
    e_gpu = ops.leapfrog(lay, co, cur.cuda(), old_g, [box], s.cuda(), ct, check=True, tiling=t)
    torch.cuda.synchronize()
    assert torch.equal(old_g.cpu(), old_cpu)
    assert e_gpu[0] == e_cpu[0] and math.isclose(e_gpu[1], e_cpu[1], rel_tol=1e-12)
    # ... and the cube's coefficients give another field (the ratios are used)
    cube = C.Coeffs.from_problem(C.Problem(70, 1e-3, 20, 1.0))
    old_c = old.cuda()
    ops.leapfrog(lay, cube, cur.cuda(), old_c, [box], s.cuda(), ct, tiling=t)
    assert not torch.equal(old_c.cpu(), old_cpu)


def test_init_first_box(gpu):
    prob, co, lay = _setup(47)
    s = ops.sin_table_ext(prob)
    a0, a1 = ops.alloc_field(lay), ops.alloc_field(lay)
    ops.init_first(lay, co, s, a0, a1)
    g0, g1 = ops.alloc_field(lay, "cuda"), ops.alloc_field(lay, "cuda")
    ops.init_first(lay, co, s.cuda(), g0, g1)
    torch.cuda.synchronize()
    assert torch.equal(ops.to_grid(lay, g0).cpu(), ops.to_grid(lay, a0))
    assert torch.equal(ops.to_grid(lay, g1).cpu(), ops.to_grid(lay, a1))


def test_init_two_box(gpu):
    """k_init_two (u¹, u² analytically) == cpu_init_first + one CPU box step, with the check of u²."""
    C = gpu
    N = 53
    prob, co, lay = _setup(N)
    u0, u1, levels, errs, ct = _cpu_start_ref(N)
    s = ops.sin_table_ext(prob)
    a, b = ops.alloc_field(lay, "cuda"), ops.alloc_field(lay, "cuda")
    nb = C.gpu_init_two_partials(lay)
    part = torch.zeros((nb, 2), dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    C.gpu_init_two(lay, co, s.cuda().data_ptr(), a.data_ptr(), b.data_ptr(), ct[0], part.data_ptr(), st)
    out = torch.empty(2, dtype=torch.float64, device="cuda")
    C.gpu_reduce(part.data_ptr(), nb, out.data_ptr(), st)
    torch.cuda.synchronize()
    own = (slice(1, -1),) * 3  # the global grid's nodes (the single rank's ghosts lie outside it)
    assert torch.equal(ops.to_grid(lay, a.cpu())[own], ops.to_grid(lay, u1)[own])
    assert torch.equal(ops.to_grid(lay, b.cpu())[own], levels[0][own])
    o = out.cpu()
    assert float(o[0]) == errs[0][0] and math.isclose(float(o[1]), errs[0][1], rel_tol=1e-12)


# ---- 9. the box kernels with ratios of 1 forced == the cube kernels, bit for bit (N = 40)
def _cube_and_forced(N=40):
    C = _C()
    prob, forced, lay = _setup(N, forced_cube=True)
    cube = C.Coeffs.from_problem(prob)
    assert not cube.box and forced.box and forced.ry == 1.0 and forced.rz == 1.0
    return prob, cube, forced, lay


# (5 steps exist for the pair-tiled load pass only)
UNIT_CASES = [(S, p2, an) for S in (2, 3, 4) for p2 in (True, False) for an in (False, True)] + [(5, True, False)]


@pytest.mark.parametrize("stages,p2,analytic", UNIT_CASES)
def test_box_kernels_with_unit_ratios_equal_cube_kernels(gpu, stages, p2, analytic):
    prob, cube, forced, lay = _cube_and_forced()
    prev, cur = _rand_interior(lay, 91 + stages), _rand_interior(lay, 92 + stages)
    ct = _cts(prob, 1 if analytic else 5, stages)
    a = _run_pass(lay, cube, prob, prev, cur, stages, ct, p2, False, analytic=analytic)
    b = _run_pass(lay, forced, prob, prev, cur, stages, ct, p2, False, analytic=analytic)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]
    assert a[1].abs().max() > 0


def test_simple_kernels_with_unit_ratios_equal_cube(gpu):
    """k_leapfrog2_rq, k_init_two, k_init_first and the single-step kernel take one path for cube and box."""
    C = gpu
    prob, cube, forced, lay = _cube_and_forced()
    box = C.compute_box(lay)
    s = ops.sin_table_ext(prob).cuda()
    st = torch.cuda.current_stream().cuda_stream
    prev, cur = _rand_interior(lay, 7), _rand_interior(lay, 8)
    res = []
    for co in (cube, forced):
        o1 = torch.zeros(int(lay.total), dtype=torch.float64, device="cuda")
        o2 = torch.zeros_like(o1)
        e2 = ops.leapfrog2(lay, co, prev.cuda(), cur.cuda(), o1, o2, box, s, 0.6, check=True)
        i0, i1 = ops.alloc_field(lay, "cuda"), ops.alloc_field(lay, "cuda")
        ops.init_first(lay, co, s, i0, i1)
        t1, t2 = ops.alloc_field(lay, "cuda"), ops.alloc_field(lay, "cuda")
        C.gpu_init_two(lay, co, s.data_ptr(), t1.data_ptr(), t2.data_ptr(), 0.9, 0, st)
        old = prev.cuda()
        e1 = ops.leapfrog(lay, co, cur.cuda(), old, [box], s, 0.6, check=True)
        torch.cuda.synchronize()
        res.append(([x.cpu() for x in (o1, o2, i0, i1, t1, t2, old)], e1, e2))
    for x, y in zip(res[0][0], res[1][0]):
        assert torch.equal(x, y)
    assert res[0][1:] == res[1][1:]


# ---- 10. the solver: GPU == CPU bit for bit, and the oracle
@pytest.mark.parametrize("N", [40, 130])
def test_solver_box_hip_equals_cpu_and_oracle(gpu, N):
    spec = box_spec(N)
    g = Solver(spec, backend="hip", device=0)
    c = Solver(spec, backend="cpu")
    rg, rc = g.run(), c.run()
    assert rg.finite and rg.steps == rc.steps == [2, 4, 6, 8, 10, 11]
    assert rg.max_err == rc.max_err
    for a, b in zip(rg.rms_err, rc.rms_err):
        assert math.isclose(a, b, rel_tol=1e-12)
    assert torch.equal(g.global_field(0), c.owned_field(0))
    o = oracle_errors(spec)
    for n, m, e in zip(rg.steps, rg.max_err, rg.rms_err):
        print(N, n, m, o[n][0], e, o[n][1])
        assert math.isclose(m, o[n][0], rel_tol=1e-6) and math.isclose(e, o[n][1], rel_tol=1e-6)
    # the schedule is the cube's
    assert g.native.mode == Solver(ProblemSpec(N=N, tau=1e-3, K=11), backend="hip", device=0).native.mode


# ---- 11. decomposition invariance
@pytest.fixture(scope="module")
def single64():
    spec = box_spec(64)
    s = Solver(spec, backend="hip", device=0)
    r = s.run()
    return spec, r, s.global_field(0), s.field_hash(0)


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("world,decomp", [(4, "slab"), (8, "2x2x2")])
def test_box_decomposition_invariance(gpu, single64, world, decomp, overlap):
    spec, r1, f0, h0 = single64
    g = Solver(spec, backend="hip", transport="loopback", world=world, rank=0, decomp=decomp, overlap=overlap,
               device=0, poison_ghosts=True)
    r = g.run()
    assert r.finite and r.steps == r1.steps and r.max_err == r1.max_err
    for a, b in zip(r.rms_err, r1.rms_err):
        assert math.isclose(a, b, rel_tol=1e-12)
    assert g.field_hash(0) == h0
    assert torch.equal(g.global_field(0), f0)


# ---- 12. the rank-process runtime forwards the box
def test_box_process_runtime(gpu):
    spec = box_spec(40)
    ref = Solver(spec, backend="hip", device=0)
    r1 = ref.run()
    s = Solver(spec, backend="hip", device=0, runtime="process")
    try:
        r = s.run()
        assert r.steps == r1.steps and r.max_err == r1.max_err and r.rms_err == r1.rms_err
        assert s.field_hash(0) == ref.field_hash(0)
    finally:
        s.close()
