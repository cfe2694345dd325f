"""Every reduction on the path from a node's error to the error log, fed non-finite values on purpose.

`finite` in the error log is the project's only blow-up detector, and every maximum in the code drops NaN: a non-finite
node is reported only if its fma(e, e, acc) term reaches the final sum of squares. Here one node of the input is NaN,
+Inf, -Inf, 1e200 (finite, its square overflows) or 3.0 (the control), at the corners, face middles, pair halves and
seeded interior nodes of the box (nonfinite_common.positions), and the reduced (max, sum) of every kernel that checks is
compared with the CPU op on the same buffers and with the numpy reference of nonfinite_common: the maximum bit-equal
and never NaN, the sum of the same class (NaN / Inf / finite) and within the derived bound where finite. Two errors
are looked for: a lost term (an owned node whose mask is off, a dropped pair half, a wave whose maximum a NaN lane
swallows) and a false alarm (non-finite garbage in a lane the rank does not own reaching a partial)."""
import functools
import math

import numpy as np
import pytest
import torch

from nonfinite_common import (LD, PLANTS, assert_pair_matches_ref, assert_pair_same_class, klass, positions,
                              ref_error_box, same_class_bits)

from mpi_cuda_amd.ops import stencil as ops
from test_gpu_kernels import P2_MASKS, TILINGS, _rand_interior, _setup

pytestmark = pytest.mark.gpu

NONFINITE = ("nan", "+inf", "-inf")


def _C():
    from mpi_cuda_amd._native import load

    return load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same_class_bits_gpu(a, b):
    na, nb = a.isnan(), b.isnan()
    z = torch.zeros((), dtype=torch.int64, device=a.device)
    return bool(torch.equal(na, nb)) and bool(torch.equal(torch.where(na, z, a.view(torch.int64)),
                                                          torch.where(nb, z, b.view(torch.int64))))


def _off(lay, p):
    return int(lay.off(*p))


# ---- k_error + k_reduce ------------------------------------------------------------------------------------------------
def _error_case(key):
    C = _C()
    if key == "slab":
        prob, co, lay, _ = _setup(C, 77, 2, 1, "slab")
        box = C.compute_box(lay)
    else:
        prob, co, lay, _ = _setup(C, 45, 8, 5, "2x2x2")
        f = C.compute_box(lay)
        box = C.LBox(f.x0 + 2, f.x1 - 3, f.y0 + 1, f.y1 - 2, f.z0 + 3, f.z1 - 1)
    torch.manual_seed(3)
    u = torch.randn(int(lay.total), dtype=torch.float64)
    return lay, box, u, ops.sin_table_ext(prob)


def _plane_nodes(box):
    """The nodes of the box's second plane with in-plane index q = 0, 63, 64, 255, 256 and the last one (k_error: lane
    0, the wave seam, the block seam)."""
    ny, nz = box.y1 - box.y0, box.z1 - box.z0
    assert ny * nz > 257
    return [(box.x0 + 1, box.y0 + q // nz, box.z0 + q % nz) for q in (0, 63, 64, 255, 256, ny * nz - 1)]


@pytest.mark.parametrize("key", ["slab", "subbox"])
def test_error_kernel_one_planted_node(gpu, key):
    """k_error + k_reduce with one planted node. Catches: a NaN or an overflowing square that does not reach the sum, a
    NaN that reaches the reduced maximum (k_error's first value of a lane is the node's own error), a node of the box
    that no thread reads."""
    lay, box, u, s = _error_case(key)
    s_g, u_g = s.cuda(), u.cuda()
    ct = 0.3
    nodes = positions(box.as_tuple(), seed=1) + _plane_nodes(box)
    for name, v in PLANTS.items():
        for p in nodes:
            o = _off(lay, p)
            keep = float(u[o])
            u[o] = v
            u_g[o] = v
            got = ops.error(lay, u_g, box, s_g, ct)
            cpu = ops.error(lay, u, box, s, ct)
            what = (key, name, p)
            assert_pair_matches_ref(got, ref_error_box(lay, u, box, s.numpy(), ct), what)
            assert_pair_same_class(got, cpu, what)
            assert (klass(got[1]) == "finite") == (name == "3.0"), what
            u[o] = keep
            u_g[o] = keep


@pytest.mark.parametrize("key", ["slab", "subbox"])
def test_error_kernel_nan_lane_keeps_its_waves_maximum(gpu, key):
    """A NaN node and, in the same wave, a node whose error is the largest of the box: the reduced maximum is that
    error. A NaN that enters the butterfly as a lane's maximum stays in its lane and swallows every value routed through
    it (lane j takes its partners' maxima with `other > mine`, false against NaN), so the partner's 1e3 would be lost."""
    lay, box, u, s = _error_case(key)
    s_g = s.cuda()
    ny, nz = box.y1 - box.y0, box.z1 - box.z0
    node = lambda q: (box.x0 + 1, box.y0 + q // nz, box.z0 + q % nz)  # noqa: E731
    for j, big in ((1, 3), (0, 1), (2, 34), (37, 5), (63, 31), (64 + 33, 64 + 1), (256 + 5, 256 + 7)):
        v = u.clone()
        v[_off(lay, node(j))] = float("nan")
        v[_off(lay, node(big))] = 1e3
        got = ops.error(lay, v.cuda(), box, s_g, 0.3)
        ref = ref_error_box(lay, v, box, s.numpy(), 0.3)
        assert 999.0 < ref[0] < 1001.0 and klass(ref[1]) == "nan"
        assert_pair_matches_ref(got, ref, (key, j, big))
        assert_pair_same_class(got, ops.error(lay, v, box, s, 0.3), (key, j, big))


@pytest.mark.parametrize("key", ["slab", "subbox"])
def test_error_kernel_ignores_nan_outside_the_box(gpu, key):
    """NaN at every allocated node outside the box (ghosts, the rest of the rank, the row padding): the result keeps the
    bits of the clean one. Catches a partial that takes in a node next to the box."""
    lay, box, u, s = _error_case(key)
    s_g = s.cuda()
    clean = ops.error(lay, u.cuda(), box, s_g, 0.3)
    v = torch.full_like(u, float("nan"))
    inside = (slice(box.x0 + 1, box.x1 + 1), slice(box.y0 + 1, box.y1 + 1), slice(box.z0 + 1, box.z1 + 1))
    ops.grid_view(lay, v)[inside] = ops.grid_view(lay, u)[inside]
    assert int(v.isnan().sum()) > 0
    got = ops.error(lay, v.cuda(), box, s_g, 0.3)
    assert got == clean
    assert_pair_same_class(got, ops.error(lay, v, box, s, 0.3), key)
    assert_pair_matches_ref(got, ref_error_box(lay, v, box, s.numpy(), 0.3), key)


# ---- single steps with the check epilogue ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_case(key):
    C = _C()
    N, world, rank = {"N40": (40, 1, 0), "N61": (61, 2, 0)}[key]
    prob, co, lay, _ = _setup(C, N, world, rank, "slab")
    torch.manual_seed(N + rank)
    cur = torch.randn(int(lay.total), dtype=torch.float64)
    old = torch.randn(int(lay.total), dtype=torch.float64)
    return dict(prob=prob, co=co, lay=lay, box=C.compute_box(lay), cur=cur, old=old, s=ops.sin_table_ext(prob),
                ct=math.cos(prob.a_t * 5 * prob.tau), sponge=None)


@functools.lru_cache(maxsize=None)
def _damp_case():
    from test_gpu_sponge_kernel import _case

    C = _C()
    c = _case("N24-cube")
    torch.manual_seed(24)
    cur = torch.randn(int(c.lay.total), dtype=torch.float64)
    old = torch.randn(int(c.lay.total), dtype=torch.float64)
    return dict(prob=c.prob, co=c.co, lay=c.lay, box=C.compute_box(c.lay), cur=cur, old=old,
                s=torch.from_numpy(np.asarray(c.s_ext)), ct=0.7, sponge=c.tables)


def _cpu_step(K, old):
    """One checked CPU step in place over `old` (damped where the case has a sponge)."""
    C = _C()
    r = C.cpu_leapfrog(K["lay"], K["co"], K["cur"].numpy(), old.numpy(), K["box"], K["s"].numpy(), K["ct"], True,
                       sponge=K["prob"] if K["sponge"] is not None else None)
    return float(r[0]), float(r[1])


_step_refs = {}


def _step_ref(ckey, K, name, p):
    """(CPU error pair, numpy reference triple, the CPU's value at the planted node), once per case, value and node.
    u^{n+1} reads u^{n-1} at its own node only, so the CPU output is the clean output except there (asserted)."""
    k = (ckey, name, p)
    if k not in _step_refs:
        if (ckey, "clean") not in _step_refs:
            out = K["old"].clone()
            _step_refs[(ckey, "clean")] = (out, _cpu_step(K, out))
        clean = _step_refs[(ckey, "clean")][0]
        o = _off(K["lay"], p)
        old = K["old"].clone()
        old[o] = PLANTS[name]
        e = _cpu_step(K, old)
        exp = clean.clone()
        exp[o] = old[o]
        assert same_class_bits(old.numpy(), exp.numpy())
        _step_refs[k] = (e, ref_error_box(K["lay"], old, K["box"], K["s"].numpy(), K["ct"]), float(old[o]))
    return _step_refs[k]


def _single_steps(ckey, K, tiling):
    C = _C()
    lay, box = K["lay"], K["box"]
    t = C.LeapfrogTiling()
    for k, v in tiling.items():
        setattr(t, k, v)
    nb = C.gpu_leapfrog_blocks(lay, [box], t)
    cur_g, s_g, old0 = K["cur"].cuda(), K["s"].cuda(), K["old"].cuda()
    _step_ref(ckey, K, "3.0", (box.x0, box.y0, box.z0))
    clean_g = _step_refs[(ckey, "clean")][0].cuda()
    part = torch.empty((max(nb, 1), 2), dtype=torch.float64, device="cuda")
    out = torch.empty(2, dtype=torch.float64, device="cuda")
    old_g, exp_g = torch.empty_like(old0), torch.empty_like(old0)
    for name, v in PLANTS.items():
        for p in positions(box.as_tuple(), seed=2):
            e_cpu, ref, at = _step_ref(ckey, K, name, p)
            o = _off(lay, p)
            old_g.copy_(old0)
            old_g[o] = v
            part.fill_(float("nan"))
            C.gpu_leapfrog(lay, K["co"], cur_g.data_ptr(), old_g.data_ptr(), [box], s_g.data_ptr(), K["ct"],
                           part.data_ptr(), t, _stream(), sponge=K["sponge"].data_ptr() if K["sponge"] is not None else 0)
            C.gpu_reduce(part.data_ptr(), nb, out.data_ptr(), _stream())
            got = tuple(float(x) for x in out.cpu())
            what = (ckey, tiling, name, p)
            exp_g.copy_(clean_g)
            exp_g[o] = at
            assert _same_class_bits_gpu(old_g, exp_g), what  # the whole padded array
            assert_pair_same_class(got, e_cpu, what)
            assert_pair_matches_ref(got, ref, what)
            assert (klass(got[1]) == "finite") == (name == "3.0"), what
            if K["sponge"] is None:  # (2c - old: the sign flips; a damped node mixes old in twice and gives NaN)
                assert klass(old_g[o].item()) == {"nan": "nan", "+inf": "-inf", "-inf": "+inf"}.get(name, "finite"), what


@pytest.mark.parametrize("tiling", TILINGS)
@pytest.mark.parametrize("ckey", ["N40", "N61"])
def test_single_step_check_sees_one_planted_node(gpu, ckey, tiling):
    """The CHECK instantiations of k_leapfrog_lds / k_leapfrog_rq: u^{n-1} planted at X makes u^{n+1} non-finite at X
    and nowhere else — a pin-point probe of which nodes the check epilogue covers. Catches a pair half, a tile edge or
    a last row whose error is not accumulated, and a partial that turns NaN."""
    _single_steps(ckey, _step_case(ckey), tiling)


@pytest.mark.parametrize("tiling", [dict(variant=0, ty=8), dict(variant=1, rows=1), dict(variant=1, rows=2),
                                    dict(variant=1, rows=4)])
def test_damped_single_step_check_sees_one_planted_node(gpu, tiling):
    """The same for the DAMP forms (all six faces damped, N = 24, W = 6): X lies inside and outside the layers."""
    _single_steps("damp", _damp_case(), tiling)


# ---- fused passes ------------------------------------------------------------------------------------------------------
def _ct(prob, S):
    return [math.cos(prob.a_t * (5 + k) * prob.tau) for k in range(1, S + 1)]


@functools.lru_cache(maxsize=None)
def _fused_case(N):
    C = _C()
    prob, co, lay, _ = _setup(C, N)
    return dict(prob=prob, co=co, lay=lay, box=C.compute_box(lay), prev=_rand_interior(C, lay, N * 13),
                cur=_rand_interior(C, lay, N * 17), s=ops.sin_table_ext(prob))


def _cpu_steps(K, prev, S):
    """S checked CPU steps from (prev, K.cur): ({level: (max, sum)}, u^{n+S-1}, u^{n+S})."""
    a, b = prev, K["cur"].clone()
    ct = _ct(K["prob"], S)
    e = {}
    for k in range(1, S + 1):
        e[k] = ops.leapfrog(K["lay"], K["co"], b, a, [K["box"]], K["s"], ct[k - 1], check=True)
        a, b = b, a
    return e, a, b


@functools.lru_cache(maxsize=None)
def _fused_clean(N, S):
    return _cpu_steps(_fused_case(N), _fused_case(N)["prev"].clone(), S)


@functools.lru_cache(maxsize=None)
def _fused_ref(N, S, name, p):
    """S CPU steps from u^{n-1} planted at p: the errors of every level and both outputs as (indices, values) of the
    nodes whose bits differ from the clean outputs (the clipped diamond around p)."""
    K = _fused_case(N)
    prev = K["prev"].clone()
    prev[_off(K["lay"], p)] = PLANTS[name]
    e, a, b = _cpu_steps(K, prev, S)
    _, ca, cb = _fused_clean(N, S)
    diff = []
    for got, clean in ((a, ca), (b, cb)):
        idx = torch.nonzero(got.view(torch.int64) != clean.view(torch.int64)).reshape(-1)
        assert 0 < len(idx) <= (2 * S + 1) ** 3
        diff.append((idx, got[idx].clone()))
    return e, diff


def _assert_fields_with_pinned_face(N, name, got, exp, what):
    """k_leapfrog_p2 enforces the Dirichlet value through the coefficient: a node outside the global interior is updated
    with tau^2 = 0, fma(0, Lap, +0), which is +0 for a finite Laplacian and NaN for a non-finite one, where the CPU never
    computes. The pass stores whole 16-byte pairs, so with an odd number of interior nodes per row the boundary node
    z = N shares the last stored pair with z = N - 1 and that value reaches memory (docs/ARCHITECTURE.md "Non-finite
    fields"). Pinned here: every other node equals the CPU's; a node of the face z = N holds +0 or NaN; NaN only at
    1 <= x, y <= N - 1 and only where the CPU's level has NaN at (x, y, N - 1); and for a NaN plant the last level's
    face is NaN exactly where level S - 1 is non-finite at (x, y, N - 1), at the face node itself or at one of its four
    face neighbours (the terms of that Laplacian)."""
    (g1, g2), (e1, e2) = got, exp
    f = N + 1  # index of node z = N in the ghost-padded grid
    for g, e in ((g1, e1), (g2, e2)):
        gc, ec = g.clone(), e.clone()
        gc[:, :, f] = 0.0
        ec[:, :, f] = 0.0
        assert _same_class_bits_gpu(gc, ec), what
        face = g[:, :, f]
        nan = face.isnan()
        assert bool(((face.contiguous().view(torch.int64) == 0) | nan).all()), what
        inner = torch.zeros_like(nan)
        inner[2:N + 1, 2:N + 1] = True
        assert not bool((nan & ~inner).any()), what
        assert not bool((nan & ~e[:, :, f - 1].isnan()).any()), what
    if name == "nan":
        n1 = g1[:, :, f].isnan()
        want = ~e1[:, :, f - 1].isfinite() | n1
        want[1:] |= n1[:-1]
        want[:-1] |= n1[1:]
        want[:, 1:] |= n1[:, :-1]
        want[:, :-1] |= n1[:, 1:]
        inner = torch.zeros_like(want)
        inner[2:N + 1, 2:N + 1] = True
        assert torch.equal(g2[:, :, f].isnan(), want & inner), what


def _fused(N, S, launch, checked, names=NONFINITE + ("1e200",), pinned_face=False):
    """launch(K, prev_g, o1, o2) -> {level: (max, sum)}; `checked`: the levels that must be present."""
    K = _fused_case(N)
    K = dict(K, cur_g=K["cur"].cuda(), s_g=K["s"].cuda())
    lay = K["lay"]
    _, ca, cb = _fused_clean(N, S)
    ca_g, cb_g, prev0 = ca.cuda(), cb.cuda(), K["prev"].cuda()
    prev_g = torch.empty_like(prev0)
    o1 = torch.empty_like(prev0)
    o2 = torch.empty_like(prev0)
    e1, e2 = torch.empty_like(prev0), torch.empty_like(prev0)
    for name in names:
        for p in positions(K["box"].as_tuple(), seed=N + S):
            e_cpu, diff = _fused_ref(N, S, name, p)
            prev_g.copy_(prev0)
            prev_g[_off(lay, p)] = PLANTS[name]
            o1.zero_()
            o2.zero_()
            e_gpu = launch(K, prev_g, o1, o2)
            what = (N, S, name, p)
            for exp, clean, (idx, vals) in ((e1, ca_g, diff[0]), (e2, cb_g, diff[1])):
                exp.copy_(clean)
                exp[idx.cuda()] = vals.cuda()
            # (the fused kernels write the interior only: boundary and ghost nodes of the outputs stay 0, as the CPU's)
            if pinned_face:
                _assert_fields_with_pinned_face(N, name, (ops.grid_view(lay, o1), ops.grid_view(lay, o2)),
                                                (ops.grid_view(lay, e1), ops.grid_view(lay, e2)), what)
            else:
                assert _same_class_bits_gpu(ops.grid_view(lay, o1), ops.grid_view(lay, e1)), what
                assert _same_class_bits_gpu(ops.grid_view(lay, o2), ops.grid_view(lay, e2)), what
            assert sorted(e_gpu) == sorted(checked), what  # unchecked levels stay absent
            for k in checked:
                assert_pair_same_class(e_gpu[k], e_cpu[k], what + (k,))
                if name in NONFINITE:
                    assert klass(e_gpu[k][1]) != "finite", what + (k,)
            if name == "1e200":  # level 1: one node whose square overflows
                assert klass(e_cpu[1][1]) == "+inf" and e_cpu[1][0] > 1e199


@pytest.mark.parametrize("rows", [1, 2, 4])
@pytest.mark.parametrize("N", [40, 77])
def test_leapfrog2_check_with_a_planted_node(gpu, rows, N):
    """k_leapfrog2_rq (the check of u^{n+2}): u^{n-1} planted at X makes level 2 non-finite on the radius-1 diamond."""
    C = _C()
    t = C.Leapfrog2Tiling()
    t.rows = rows

    def launch(K, prev_g, o1, o2):
        e = ops.leapfrog2(K["lay"], K["co"], prev_g, K["cur_g"], o1, o2, K["box"], K["s_g"],
                          _ct(K["prob"], 2)[1], check=True, tiling=t)
        return {2: e}

    _fused(N, 2, launch, [2])


@pytest.mark.parametrize("threads", [768, 1024])
@pytest.mark.parametrize("stages", [2, 3, 4])
@pytest.mark.parametrize("N", [40, 77])
def test_leapfrog_tb_check_with_a_planted_node(gpu, N, stages, threads):
    """k_leapfrog_tb, every level checked: level 1 is non-finite at X only (exactly one node carries it), level k on
    the clipped diamond of radius k - 1."""

    def launch(K, prev_g, o1, o2):
        return ops.leapfrog_tb(K["lay"], K["co"], prev_g, K["cur_g"], o1, o2, K["box"], K["s_g"], stages,
                               _ct(K["prob"], stages), (1 << stages) - 1, threads, p2=False)

    _fused(N, stages, launch, list(range(1, stages + 1)), names=NONFINITE)


@pytest.mark.parametrize("chunked", [False, True])
@pytest.mark.parametrize("mask", ["all", "odd", "even"])
@pytest.mark.parametrize("stages", [2, 3, 4, 5])
@pytest.mark.parametrize("N", [40, 77])
def test_leapfrog_p2_check_with_a_planted_node(gpu, N, stages, mask, chunked):
    """k_leapfrog_p2 with both accumulator schemes: split accumulators per pair half, masked once in the reduction
    (kSplitAcc: 5 stages with at most 3 checked levels, here the odd and even masks at 5 stages) and the per-plane masked
    scheme (every other case). Catches a pair half whose
    term is dropped, the two halves' ownership masks swapped, a masked lane's garbage added instead of selected."""
    C = _C()
    m = P2_MASKS[mask](stages)
    checked = [k for k in range(1, stages + 1) if m >> (k - 1) & 1]

    def launch(K, prev_g, o1, o2):
        assert C.gpu_leapfrog_p2_supported(K["lay"], K["box"], stages)
        return ops.leapfrog_tb(K["lay"], K["co"], prev_g, K["cur_g"], o1, o2, K["box"], K["s_g"], stages,
                               _ct(K["prob"], stages), m, p2=True, target_blocks=256 if chunked else 1)

    # (N = 40: 39 interior nodes per row, the boundary node z = N is the second half of the last stored pair)
    _fused(N, stages, launch, checked, names=NONFINITE if not (mask == "all" and not chunked) else NONFINITE + ("1e200",),
           pinned_face=(N - 1) % 2 == 1)


# ---- ownership masks with non-finite garbage -----------------------------------------------------------------------------
@pytest.mark.parametrize("p2,S,mask", [(True, 4, 0b1111), (False, 4, 0b1111), (True, 5, 0b10101), (True, 5, 0b01010)],
                         ids=["p2-S4-all", "tb-S4-all", "p2-S5-odd", "p2-S5-even"])
@pytest.mark.parametrize("key", ["c7", "s1"])
def test_rank_pass_partials_ignore_nan_in_unowned_lanes(gpu, key, p2, S, mask):
    """One rank of a decomposition (tests/test_gpu_rank_pass.py: the global random fields cut to the rank's S-deep
    ghosts). A NaN in the global u^{n-1} one layer inside a neighbour's territory — a depth-1 ghost of this rank — makes
    level 1 non-finite in a lane this rank computes but does not own: the rank's level-1 partials keep the bits of the
    clean run; from level 2 on the NaN has reached owned nodes and the partials have the class of the CPU check of the
    global field on the rank's box. The same plant at the owned node next to that ghost: level 1 is non-finite too.
    S = 4 with every level checked takes the per-plane masked accumulators; S = 5 with the odd / even mask takes the
    split accumulators, whose ownership masks are applied in the reduction."""
    from test_gpu_rank_pass import Rank, _tiling

    C = _C()
    R = Rank(key, S)
    G, lay, full = R.G, R.lay, R.full
    t = _tiling(S, p2, 256)
    slot = C.tb_slot_blocks(lay, full, t, True)
    checked = [k for k in range(1, S + 1) if mask >> (k - 1) & 1]

    def run(prev_glob):
        prev = torch.from_numpy(R.cut(prev_glob, keep=S - 1)).reshape(-1).cuda()
        cur = torch.from_numpy(R.cut(G["cur"], keep=S)).reshape(-1).cuda()
        o1 = torch.zeros(int(lay.total), dtype=torch.float64, device="cuda")
        o2 = torch.zeros_like(o1)
        part = torch.full((S * slot, 2), float("nan"), dtype=torch.float64, device="cuda")
        C.gpu_leapfrog_tb(lay, G["co"], prev.data_ptr(), cur.data_ptr(), o1.data_ptr(), o2.data_ptr(), full,
                          R.s_gpu.data_ptr(), G["ct"][:S], mask, part.data_ptr(), t, _stream(), real=R.real,
                          level_stride=slot, grid_blocks=slot)
        res = {}
        for k in checked:
            out = torch.empty(2, dtype=torch.float64, device="cuda")
            C.gpu_reduce(part[(k - 1) * slot:].data_ptr(), slot, out.data_ptr(), _stream())
            res[k] = tuple(float(v) for v in out.cpu())
        return res, part.cpu().numpy().reshape(S, slot, 2).copy()

    def cpu_levels(prev_glob):
        """The CPU check of S global steps from the planted u^{n-1} over the rank's box."""
        gl = G["gl"]
        gfull = C.compute_box(gl)
        a = ops.from_grid(gl, torch.from_numpy(np.pad(prev_glob, 1)))
        b = ops.from_grid(gl, torch.from_numpy(np.pad(G["cur"], 1)))
        gb = C.LBox(full.x0 + lay.gx0, full.x1 + lay.gx0, full.y0 + lay.gy0, full.y1 + lay.gy0, full.z0 + lay.gz0,
                    full.z1 + lay.gz0)
        e = {}
        for k in range(1, S + 1):
            ops.leapfrog(gl, G["co"], b, a, [gfull], G["s"])
            a, b = b, a
            e[k] = ops.error(gl, b, gb, G["s"], G["ct"][k - 1])
        return e

    clean, clean_part = run(G["prev"])
    for k in checked:
        assert klass(clean[k][1]) == "finite"
    # the faces of the rank's box that have a neighbour: the ghost node one layer outside, and the owned node next to it
    lo = [R.g0[a] for a in range(3)]
    hi = [R.g0[a] + R.n[a] for a in range(3)]
    mid = [(lo[a] + hi[a]) // 2 for a in range(3)]
    done = 0
    for a in range(3):
        for side in (0, 1):
            if not R.nb[a][side]:
                continue
            ghost, owned = list(mid), list(mid)
            ghost[a] = lo[a] - 1 if side == 0 else hi[a]
            owned[a] = lo[a] if side == 0 else hi[a] - 1
            for node, is_owned in ((ghost, False), (owned, True)):
                glob = G["prev"].copy()
                glob[tuple(node)] = np.nan
                got, got_part = run(glob)
                want = cpu_levels(glob)
                what = (key, p2, a, side, is_owned)
                if not is_owned:
                    assert klass(want[1][1]) == "finite"
                    if 1 in checked:
                        assert np.array_equal(got_part[0].view(np.int64), clean_part[0].view(np.int64)), what
                for k in checked:
                    assert_pair_same_class(got[k], want[k], what + (k,))
                    assert (klass(got[k][1]) == "nan") == (is_owned or k >= 2), what + (k,)
                done += 1
    assert done >= 4


# ---- k_reduce / k_reduce_batch / k_energy_reduce -------------------------------------------------------------------------
LENS = [1, 5, 256, 1023, 1024, 1025, 3000]
REDUCE_PLANTS = {"nan": float("nan"), "inf": float("inf"), "1e308": 1e308}


def _reduce_cases(n):
    """(values to plant, indices): each value into .x, into .y and into both, at 0, 63, 64, 1023, 1024, n - 1 where the
    index exists; 1e308 at two indices (two of them sum to Inf)."""
    idx = sorted({i for i in (0, 63, 64, 1023, 1024, n - 1) if i < n})
    for name, v in REDUCE_PLANTS.items():
        for cols in ((0,), (1,), (0, 1)):
            for i in idx:
                at = [i] if name != "1e308" or n == 1 else [i, (i + 1) % n]
                yield name, v, cols, at


def _expected_reduce(p):
    with np.errstate(all="ignore"):
        return float(np.fmax.reduce(p[:, 0], initial=0.0)), p[:, 1].astype(LD).sum(dtype=LD)


def test_reduce_with_nonfinite_partials(gpu):
    """k_reduce: x = the maximum of the partial maxima that are not NaN (0 if none), y has the class of the longdouble
    sum (NaN sticks, Inf + finite = Inf, 1e308 + 1e308 = Inf). k_energy_reduce sums both columns. Catches a partial that
    is skipped (the first, a wave seam, the stride seam, the last) and a NaN partial maximum that reaches the result."""
    C = _C()
    rng = np.random.default_rng(11)
    out = torch.empty(2, dtype=torch.float64, device="cuda")
    for n in LENS:
        base = rng.random((n, 2))
        for name, v, cols, at in _reduce_cases(n):
            p = base.copy()
            for c in cols:
                p[at, c] = v
            d = torch.from_numpy(p).cuda()
            C.gpu_reduce(d.data_ptr(), n, out.data_ptr(), _stream())
            got = tuple(float(x) for x in out.cpu())
            mx, sm = _expected_reduce(p)
            what = (n, name, cols, at)
            assert not math.isnan(got[0]) and got[0] == mx, (what, got, mx)
            assert klass(got[1]) == klass(sm), (what, got, sm)
            if klass(sm) == "finite":
                assert abs(LD(got[1]) - sm) <= 2 * n * 2.0 ** -53 * sm, what
            C.gpu_energy_reduce(d.data_ptr(), n, out.data_ptr(), _stream())
            ge = tuple(float(x) for x in out.cpu())
            with np.errstate(all="ignore"):
                kin = p[:, 0].astype(LD).sum(dtype=LD)
            assert klass(ge[0]) == klass(kin) and klass(ge[1]) == klass(sm), (what, ge)


@pytest.mark.parametrize("planted_job", [5, 69])
def test_reduce_batch_equals_reduce_with_nonfinite_partials(gpu, planted_job):
    """k_reduce_batch == k_reduce per job under same_class_bits, 70 jobs (two launches), the planted job (1025 and 3000
    partials: past the 1024-thread stride) on either side of the 64-job split."""
    C = _C()
    rng = np.random.default_rng(12)
    lens = LENS * 10
    n = lens[planted_job]
    base = [rng.random((m, 2)) for m in lens]
    parts = [torch.from_numpy(b).cuda() for b in base]
    for name, v, cols, at in _reduce_cases(n):
        p = base[planted_job].copy()
        for c in cols:
            p[at, c] = v
        parts[planted_job] = torch.from_numpy(p).cuda()
        a = torch.zeros((len(lens), 2), dtype=torch.float64, device="cuda")
        b = torch.zeros_like(a)
        for j, q in enumerate(parts):
            C.gpu_reduce(q.data_ptr(), q.shape[0], a[j].data_ptr(), _stream())
        C.gpu_reduce_batch([(q.data_ptr(), q.shape[0], b[j].data_ptr()) for j, q in enumerate(parts)], _stream())
        torch.cuda.synchronize()
        assert same_class_bits(a.cpu().numpy(), b.cpu().numpy()), (name, cols, at)
        mx, sm = _expected_reduce(p)
        row = b[planted_job].cpu().numpy()
        assert row[0] == mx and klass(row[1]) == klass(sm), (name, cols, at, row)
        others = np.delete(b.cpu().numpy(), planted_job, axis=0)
        assert np.isfinite(others).all()
