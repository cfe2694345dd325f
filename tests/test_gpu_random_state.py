"""Every halo transport of the in-process groups, started from a RANDOM loaded state (Solver.set_state).

The other multi-rank tests start from the analytic state: a separable sine product, mirror-symmetric about the middle
of every axis and unchanged by swapping axes of equal edge, so a lo/hi or y/z mix-up in a message offset, a region map,
a staging parity or a ghost store can move bit-identical data there (tests/test_gpu_rank_pass.py closed that hole for
the kernels alone). Here u^1 and u^2 are random on the interior nodes and exactly 0 on the global boundary; every rank
of a group takes its box and ghosts from them, the solve continues to K = 14 with every step checked, and the error log
and both final fields are compared with native CPU single steps of the UNDECOMPOSED grid — bit for bit for the fields
and the maxima, 1e-12 relative for the fixed-order sums. What the solves run between the load and the comparison is the
wiring no kernel test reaches: plan_msgs offsets and ghost_bits, msg_buf and the four-buffer rotation, the staging
layouts, the loopback / RCCL send-receive order and tags, the copy-engine region maps and flag epochs, the push staging
parities, the shell-first overlap order and the rank-ordered combination of the error partials.

Every case runs twice: the state is uploaded again, the flag parities / epochs and the buffer contents are those the
first solve left. Ghosts are NaN-poisoned wherever the existing tests poison them (not: rccl-self on block ranks, except
with debug_sync as test_poisoned_ghosts_still_bitexact runs it); from the second pass on the outputs rotate into buffers
whose ghosts hold stale data of the loaded state's era, so a missed delivery shows either way. On slab ranks with
ghost_store the poison includes the u^{n+S-1} plane the passes store themselves (schedule.hpp plan_poison).

Two-step deep halos (tb=False) exist only without odd check steps (schedule.cpp pairable), so those cases check every
second step; every other case checks every step.
"""
import functools
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from mpi_cuda_amd import ProblemSpec
from mpi_cuda_amd.ops import stencil as ops
from mpi_cuda_amd.solver import Solver
from mpi_cuda_amd.utils import dump

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "wave3d")

TAU, K, N0 = 1e-3, 14, 2
BOX = dict(L=1.0, Ly=1.3, Lz=0.7)
# key: (decomp, world, N) — N the smallest that gives the layout: slabs of 33 / 22 planes; odd extents; ny != nz;
# x neighbours on both sides; all 26 neighbours (33-node extents); 8-9 planes per slab rank (needs tb_min_planes)
DECOMPS = {"s2": ("slab", 2, 66), "s3": ("slab", 3, 66), "s8": ("slab", 8, 66), "c8": ("2x2x2", 8, 67),
           "b6": ("1x2x3", 6, 70), "x12": ("3x2x2", 12, 70), "r27": ("3x3x3", 27, 100)}


def _C():
    from mpi_cuda_amd._native import load

    return load()


def _spec(N, K_=K, box=False, check_every=1):
    return ProblemSpec(N=N, tau=TAU, K=K_, check_every=check_every, **(BOX if box else {}))


# ---- the reference: random u^1, u^2 on the whole grid and 12 native CPU steps of the one-rank layout, once per grid
@functools.lru_cache(maxsize=None)
def _global(N, box=False):
    """prev / cur: the loaded state, (N+1)^3; level[n]: u^n for n = 12, 13, 14; err[n]: (max, rms) for n = 3..14;
    torch_dist: max |native - plain torch| at u^14 (cubes)."""
    C = _C()
    prob = _spec(N, box=box).native()
    co = C.Coeffs.from_problem(prob)
    gl = C.make_layout(prob, C.rank_box(prob, C.Dims(1, 1, 1), 0))
    full = C.compute_box(gl)
    s = ops.sin_table_ext(prob)
    torch.manual_seed(N * 131 + (17 if box else 0))

    def rand_field():
        g = torch.zeros((N + 3,) * 3, dtype=torch.float64)
        g[2:-2, 2:-2, 2:-2] = torch.randn((N - 1,) * 3, dtype=torch.float64)
        return ops.from_grid(gl, g)

    dense = lambda f: ops.to_grid(gl, f)[1:-1, 1:-1, 1:-1].contiguous()  # noqa: E731
    prev, cur = rand_field(), rand_field()
    for f in (prev, cur):  # exactly 0 on the global boundary
        d = dense(f)
        for a in range(3):
            assert not d.select(a, 0).any() and not d.select(a, N).any()
    a, b = prev.clone(), cur.clone()
    level, err = {}, {}
    denom = float(N - 1) ** 3
    for n in range(N0 + 1, K + 1):
        ops.leapfrog(gl, co, b, a, [full], s)  # in place over u^{n-2}
        a, b = b, a
        m, q = C.cpu_error(gl, b.numpy(), full, s.numpy(), C.time_factor(prob, n))
        err[n] = (m, math.sqrt(q / denom))
        if n >= K - 2:
            level[n] = dense(b)
    torch_dist = None
    if not box:
        # the plain fp64 torch loop of the same 12 steps (guards the reference's formula). Measured max |native - torch|
        # at u^14 (values up to ~50): 7.1e-14 (N = 66), 5.7e-14 (67), 6.4e-14 (70), 4.6e-14 (100) — below a tenth of
        # the project's atol = 1e-9, which therefore stays
        ta, tb = ops.to_grid(gl, prev), ops.to_grid(gl, cur)
        for n in range(N0 + 1, K + 1):
            ta, tb = tb, ops.ref_leapfrog_grid(tb, ta, co.ihx2, co.ihy2, co.ihz2, co.tau2, full)
        torch_dist = float((tb[1:-1, 1:-1, 1:-1] - level[K]).abs().max())
        print(f"N={N}: max |native - torch| after {K - N0} steps = {torch_dist:.3e}")
        assert torch_dist <= 1e-10
        torch.testing.assert_close(tb[1:-1, 1:-1, 1:-1], level[K], rtol=0, atol=1e-9)
    return dict(prob=prob, prev=dense(prev), cur=dense(cur), level=level, err=err, torch_dist=torch_dist)


def test_reference_equals_cpu_solver(gpu):
    """The ops.leapfrog loop of `_global` against Solver(backend="cpu").set_state on the same random state: the same
    error log and fields (two routes through the native CPU kernels: the reference is not a slip of the loop)."""
    G = _global(66)
    c = Solver(_spec(66), backend="cpu")
    c.set_state(G["prev"], G["cur"], N0)
    r = c.run()
    assert r.steps == list(range(N0 + 1, K + 1))
    assert r.max_err == [G["err"][n][0] for n in r.steps]
    for n, e in zip(r.steps, r.rms_err):
        assert math.isclose(e, G["err"][n][1], rel_tol=1e-12)
    assert torch.equal(c.owned_field(0), G["level"][K]) and torch.equal(c.owned_field(1), G["level"][K - 1])


# ---- one case
def _assert_field(got, want, what):
    if torch.equal(got, want):
        return
    bad = torch.nonzero(~(got == want))
    lo, hi = bad.min(0).values.tolist(), bad.max(0).values.tolist()
    raise AssertionError(f"{what}: {len(bad)} nodes differ ({int(torch.isnan(got).sum())} NaN), within x {lo[0]}..{hi[0]} "
                         f"y {lo[1]}..{hi[1]} z {lo[2]}..{hi[2]}; first {bad[:4].tolist()}")


def _group(key, transport, K_=K, box=False, check_every=1, **kw):
    decomp, world, N = DECOMPS[key]
    return Solver(_spec(N, K_, box, check_every), backend="hip", transport=transport, world=world, rank=0,
                  decomp=decomp, device=0, **kw)


def _run_case(key, transport, mode, K_=K, box=False, check_every=1, temporal=None, **kw):
    N = DECOMPS[key][2]
    G = _global(N, box)
    if temporal is not None:
        kw["temporal"] = temporal
    g = _group(key, transport, K_, box, check_every, **kw)
    # the case runs the schedule and transport it names
    assert g.native.mode() == mode and g.native.transport == transport
    if mode.startswith("deep-tb"):
        p2 = (kw.get("tiling_tb") or {}).get("p2", True)
        assert g.native.temporal() == (4 if temporal == 5 and (transport == "push" or not p2) else temporal)
    assert g.native.overlapped() == kw.get("overlap", True)
    g.set_state(G["prev"], G["cur"], N0)
    steps = [n for n in range(N0 + 1, K_ + 1) if n % check_every == 0 or n == K_]
    for run in range(2):
        r = g.run()
        assert r.steps == steps, run
        for n, m, e in zip(r.steps, r.max_err, r.rms_err):
            print(f"run {run} step {n}: max {m!r} / {G['err'][n][0]!r}  rms {e!r} / {G['err'][n][1]!r}")
        assert r.finite and r.max_err == [G["err"][n][0] for n in steps], run
        for n, e in zip(steps, r.rms_err):
            assert math.isclose(e, G["err"][n][1], rel_tol=1e-12), (run, n)
        _assert_field(g.global_field(0), G["level"][K_], f"run {run} u^{K_}")
        _assert_field(g.global_field(1), G["level"][K_ - 1], f"run {run} u^{K_ - 1}")


def _tags(kw):
    """the options of a case that are not its defaults, for its id"""
    t = []
    if "K_" in kw:
        t.append(f"K{kw['K_']}")
    if kw.get("box"):
        t.append("box")
    if kw.get("ghost_store") is False:
        t.append("nogs")
    if "tiling_tb" in kw:
        t.append("nop2")
    if "fused_pack" in kw:
        t.append(f"fused{int(kw['fused_pack'])}")
    if kw.get("debug_sync"):
        t.append("dbgsync")
    if not kw.get("poison_ghosts", True):
        t.append("nopoison")
    return t


def _tb(key, transport, temporal, overlap, **kw):
    """An LDS-pass case (deep-tb on slab keys, deep-tb-block otherwise)."""
    slab = key.startswith("s")
    if slab:
        kw.setdefault("tb_min_planes", 2 * temporal)
    kw.setdefault("poison_ghosts", slab or transport != "rccl-self")
    return pytest.param(key, transport, "deep-tb" if slab else "deep-tb-block",
                        dict(temporal=temporal, overlap=overlap, **kw),
                        id="-".join([key, transport, f"S{temporal}", "ov" if overlap else "seq"] + _tags(kw)))


def _one(key, transport, overlap, **kw):
    """Single steps (k_pack / k_unpack)."""
    kw.setdefault("poison_ghosts", True)
    return pytest.param(key, transport, "single-step", dict(temporal=1, overlap=overlap, **kw),
                        id="-".join([key, transport, "S1", "ov" if overlap else "seq"] + _tags(kw)))


def _two(key, transport, overlap):
    """Two-step deep halos on slab ranks (no odd check step: every second step is checked)."""
    return pytest.param(key, transport, "deep-halo", dict(tb=False, deep_min_planes=3, overlap=overlap, check_every=2,
                                                          poison_ghosts=True),
                        id="-".join([key, transport, "deep2", "ov" if overlap else "seq"]))


NOP2 = {"p2": False}
CASES = [
    # ---- loopback
    _tb("s2", "loopback", 5, True), _tb("s2", "loopback", 4, False), _tb("s2", "loopback", 3, True, ghost_store=False),
    _tb("s2", "loopback", 2, False, ghost_store=False), _tb("s2", "loopback", 5, True, K_=13),
    _tb("s3", "loopback", 5, False), _tb("s3", "loopback", 4, True, ghost_store=False), _tb("s3", "loopback", 3, False),
    _tb("s3", "loopback", 2, True), _tb("s3", "loopback", 4, True, tiling_tb=NOP2), _tb("s3", "loopback", 4, False, K_=13),
    _tb("s8", "loopback", 2, True), _tb("s8", "loopback", 3, False),
    _one("s2", "loopback", True), _one("s2", "loopback", False), _one("s3", "loopback", True, K_=13),
    _two("s2", "loopback", True), _two("s3", "loopback", False),
    _tb("c8", "loopback", 5, True), _tb("c8", "loopback", 4, False), _tb("c8", "loopback", 3, True),
    _tb("c8", "loopback", 2, False), _tb("c8", "loopback", 3, True, K_=13),
    _tb("c8", "loopback", 4, False, tiling_tb=NOP2, fused_pack=True),
    _tb("c8", "loopback", 4, True, tiling_tb=NOP2, fused_pack=False), _tb("c8", "loopback", 5, False, fused_pack=False),
    _tb("c8", "loopback", 4, True, box=True), _tb("c8", "loopback", 2, False, box=True),
    _one("c8", "loopback", True),
    _tb("b6", "loopback", 5, False), _tb("b6", "loopback", 4, True), _tb("b6", "loopback", 2, True),
    _tb("b6", "loopback", 3, False, tiling_tb=NOP2, fused_pack=True),
    _tb("b6", "loopback", 5, True, box=True), _tb("b6", "loopback", 3, False, box=True),
    _one("b6", "loopback", False),
    _tb("x12", "loopback", 5, True), _tb("x12", "loopback", 4, False), _tb("x12", "loopback", 2, False),
    _tb("x12", "loopback", 3, True, tiling_tb=NOP2, fused_pack=True), _one("x12", "loopback", True),
    _tb("r27", "loopback", 5, True),
    # ---- rccl-self
    _tb("s2", "rccl-self", 5, True), _tb("s2", "rccl-self", 3, False, ghost_store=False),
    _tb("s3", "rccl-self", 4, True), _tb("s3", "rccl-self", 2, False), _tb("s3", "rccl-self", 5, False, ghost_store=False),
    _tb("s3", "rccl-self", 5, True, K_=13),
    _one("s2", "rccl-self", False), _one("s3", "rccl-self", True, debug_sync=True),
    _two("s2", "rccl-self", True), _two("s3", "rccl-self", False),
    _tb("c8", "rccl-self", 5, True), _tb("c8", "rccl-self", 2, False),
    _tb("c8", "rccl-self", 4, False, tiling_tb=NOP2, fused_pack=True),
    _tb("c8", "rccl-self", 5, False, poison_ghosts=True, debug_sync=True),
    _one("c8", "rccl-self", True, debug_sync=True),
    _tb("b6", "rccl-self", 4, True), _tb("b6", "rccl-self", 3, False),
    _tb("x12", "rccl-self", 5, False), _tb("x12", "rccl-self", 3, True, tiling_tb=NOP2, fused_pack=False),
    _tb("r27", "rccl-self", 5, True),
    # ---- copy engines
    _tb("s2", "sdma", 5, True), _tb("s2", "sdma", 4, False, ghost_store=False), _tb("s2", "sdma", 3, True),
    _tb("s2", "sdma", 2, False),
    _tb("s3", "sdma", 5, False), _tb("s3", "sdma", 4, True), _tb("s3", "sdma", 3, False, ghost_store=False),
    _tb("s3", "sdma", 2, True, ghost_store=False), _tb("s3", "sdma", 5, True, K_=13), _tb("s8", "sdma", 2, True),
    _tb("c8", "sdma", 5, True), _tb("c8", "sdma", 4, False), _tb("c8", "sdma", 3, True), _tb("c8", "sdma", 2, False),
    _tb("c8", "sdma", 4, False, tiling_tb=NOP2, fused_pack=True),
    _tb("c8", "sdma", 3, True, tiling_tb=NOP2, fused_pack=False), _tb("c8", "sdma", 4, True, K_=13),
    _tb("c8", "sdma", 4, False, box=True), _tb("c8", "sdma", 5, True, box=True),
    _tb("b6", "sdma", 5, False), _tb("b6", "sdma", 4, True), _tb("b6", "sdma", 2, True),
    _tb("b6", "sdma", 5, True, box=True), _tb("b6", "sdma", 3, False, box=True),
    _tb("x12", "sdma", 5, True), _tb("x12", "sdma", 3, False),
    _tb("x12", "sdma", 4, True, tiling_tb=NOP2, fused_pack=True),
    _tb("r27", "sdma", 5, True),
    # ---- push (slab ranks of a cube; k_leapfrog_tb: 5 becomes 4)
    _tb("s2", "push", 5, True), _tb("s2", "push", 4, False), _tb("s2", "push", 3, True), _tb("s2", "push", 2, False),
    _tb("s3", "push", 4, True), _tb("s3", "push", 3, False), _tb("s3", "push", 2, True), _tb("s3", "push", 5, False),
    _tb("s3", "push", 4, True, K_=13), _tb("s2", "push", 3, False, K_=13),
]


@pytest.mark.parametrize("key,transport,mode,kw", CASES)
def test_random_state_group(gpu, key, transport, mode, kw):
    """A group of `key` over `transport` from the random loaded state, two solves: steps, error maxima (exact), rms
    (1e-12), u^K and u^{K-1} over the whole (N+1)^3 grid (exact) against the undecomposed CPU steps. Catches: a message
    at a mirrored or transposed offset, a send / receive pair matched to the wrong peer or tag, a ghost plane skipped by
    both the message and the pass (ghost_store), a staging parity or flag epoch that holds only for the first solve, a
    shell computed after its exchange, an error partial of the wrong rank or slot."""
    _run_case(key, transport, mode, **kw)


# ---- refusals: no transport returns a field for a combination it does not implement
def test_push_refuses_box(gpu):
    with pytest.raises(Exception, match="push transport has no rectangular-box kernels"):
        _group("s2", "push", box=True, temporal=4, tb_min_planes=8)


def test_push_refuses_block_ranks(gpu):
    with pytest.raises(Exception, match=r"push transport: slab LDS passes \(deep-tb\) only, not deep-tb-block"):
        _group("c8", "push", temporal=4)


def test_push_refuses_single_steps(gpu):
    with pytest.raises(Exception, match=r"push transport: slab LDS passes \(deep-tb\) only, not single-step"):
        _group("s2", "push", temporal=1)


def test_sdma_refuses_single_steps(gpu):
    for key in ("s2", "c8"):
        with pytest.raises(Exception, match=r"sdma transport: LDS multi-step passes \(deep-tb, slab or block\) only, "
                                            "not single-step"):
            _group(key, "sdma", temporal=1)


@pytest.mark.parametrize("transport", ["loopback", "rccl-self"])
def test_deep_halo_refuses_odd_remainder(gpu, transport):
    G = _global(66)
    g = _group("s2", transport, check_every=2, tb=False, deep_min_planes=3)
    assert g.native.mode() == "deep-halo"
    with pytest.raises(Exception, match="resume: two-step passes need an even step count left"):
        g.set_state(G["prev"], G["cur"], 3)


@pytest.mark.parametrize("transport,key", [("loopback", "s2"), ("sdma", "c8"), ("push", "s3")])
def test_deep_tb_refuses_one_step_left(gpu, transport, key):
    G = _global(DECOMPS[key][2])
    g = _group(key, transport, temporal=4, tb_min_planes=8)
    assert g.native.mode().startswith("deep-tb")
    with pytest.raises(Exception, match="resume: the multi-rank LDS passes need >= 2 steps left"):
        g.set_state(G["prev"], G["cur"], K - 1)
    with pytest.raises(Exception, match=r"resume step must be in \[1, K\)"):
        g.set_state(G["prev"], G["cur"], K)


# ---- rank processes and the CLI group: the random state through checkpoint files
def _read_dump(prefix, world, N):
    field = np.full((N + 1,) * 3, np.nan)
    for r in range(world):
        m = json.loads(open(f"{prefix}.rank{r}.json").read())
        nx, ny, nz = m["shape"]
        x0, y0, z0 = m["offset"]
        field[x0:x0 + nx, y0:y0 + ny, z0:z0 + nz] = np.fromfile(f"{prefix}.rank{r}.bin").reshape(nx, ny, nz)
    return field


def test_random_checkpoint_through_processes(gpu, tmp_path):
    """The random state written as a checkpoint (utils.dump.save), resumed by two copy-engine rank processes sharing
    the GPU (IPC-mapped peers, no RCCL) and by a 4-rank 2x2x1 group of the CLI: the dumped u^K is the CPU reference's,
    bit for bit, and the CLI's combined error log is the reference's."""
    N = 66
    G = _global(N)
    ck = str(tmp_path / "ck")
    for name, f, step in (("prev", G["prev"], N0 - 1), ("cur", G["cur"], N0)):
        dump.save(f"{ck}.{name}", f.numpy(), N=N, L=1.0, tau=TAU, step=step)
    want = G["level"][K].numpy()
    env = dict(os.environ, W3D_TIMEOUT_S="30", W3D_SHARE_GPUS="1")
    env.pop("W3D_RDZV_FILE", None)
    out, js = str(tmp_path / "p"), str(tmp_path / "p.json")
    p = subprocess.run([CLI, str(N), str(TAU), str(K), "1", "--np", "2", "--transport", "sdma", "--no-rccl", "--check-every",
                        "1", "--resume", ck, "--dump", out, "--json", js, "--quiet"], env=env, timeout=120,
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    meta = json.loads(open(js).read())
    assert meta["transport"] == "sdma"
    assert np.array_equal(_read_dump(out, 2, N), want)
    assert [s[0] for s in meta["steps"]] == list(range(N0 + 1, K + 1))
    for n, m, e in meta["steps"]:  # (the JSON log is printed with 9 significant digits)
        assert m == pytest.approx(G["err"][n][0], rel=1e-8) and e == pytest.approx(G["err"][n][1], rel=1e-8)
    out = str(tmp_path / "g")
    p = subprocess.run([CLI, str(N), str(TAU), str(K), "1", "--group", "4", "--decomp", "2x2x1", "--check-every", "1",
                        "--resume", ck, "--dump", out, "--quiet"], env=env, timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    assert np.array_equal(_read_dump(out, 4, N), want)
