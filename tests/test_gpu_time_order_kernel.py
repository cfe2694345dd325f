"""k_lap4, k_leapfrog44 and the time_order = 4 first step against cpu_lap4 / cpu_leapfrog44 / cpu_first_step_t4, bit for bit.

The method of tests/test_gpu_order4_kernel.py: u, u^{n-1} and the v buffer hold LCG-random values on the global interior
(v: what the kernel under test must produce, or cpu_lap4's), exact zeros on the six faces and NaN in the stored ghost layer
and the row padding, so a kernel that uses node -1 or N + 1 of any of the three as data, instead of -centre, produces NaN.
Outputs are compared over the whole padded array: nothing outside the interior is written, and k_lap4 writes nothing but v.
Shapes, each the smallest at which one mechanism can fail: N = 6 (every interior node within 2 of a wall), N = 24 cube (one
partial tile, both walls in it), N = 40 box (N - 1 odd: the last pair of a row is half boundary), N = 136 cube (68 pairs: two
z tiles; 135 rows: several y tiles; checked variants only). x is chunked down to 3 planes and to 1."""
import functools
import math

import numpy as np
import pytest
import torch

from sources_common import BOX, same_bits

pytestmark = pytest.mark.gpu

CONFIGS = {"N6-cube": (6, False), "N24-cube": (24, False), "N40-box": (40, True), "N136-cube": (136, False)}


def _C():
    from mpi_cuda_amd._native import load

    return load()


def lcg(n, seed):
    """n doubles in (-1, 1): two steps of a 64-bit linear congruential generator (Knuth's MMIX constants) from the state
    seed + i, with a shift between them."""
    a, c = np.uint64(6364136223846793005), np.uint64(1442695040888963407)
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=np.uint64) + np.uint64(seed)) * a + c
        x ^= x >> np.uint64(33)
        x = x * a + c
    return (x >> np.uint64(11)).astype(np.float64) / float(1 << 52) - 1.0


class Case:
    def __init__(self, key):
        C = _C()
        self.N, box = CONFIGS[key]
        N = self.N
        # tau at 0.9 of the limit: courant 1.35, where lam s(u) is several times u
        tm = C.Problem(N, 1.0, 9, BOX[0], Ly=BOX[1], Lz=BOX[2]).tau_max if box else C.Problem(N, 1.0, 9, 1.0).tau_max
        kw = dict(order=4, time_order=4)
        self.prob = (C.Problem(N, 1.35 * tm, 9, BOX[0], Ly=BOX[1], Lz=BOX[2], **kw) if box
                     else C.Problem(N, 1.35 * tm, 9, 1.0, **kw))
        self.co = C.Coeffs.from_problem(self.prob)
        assert self.co.order == 4 and self.co.time_order == 4
        self.lay = l = C.make_layout(self.prob, C.rank_box(self.prob, C.Dims(1, 1, 1), 0))
        self.s_ext = C.sin_table_ext(self.prob)
        self.full = C.compute_box(l)
        i, a = np.arange(1, N), np.arange(0, N + 1)
        o = int(l.off(0, 0, 0))
        self.inner = o + i[:, None, None] * int(l.plane) + i[None, :, None] * int(l.pitch) + i[None, None, :]
        owned = o + a[:, None, None] * int(l.plane) + a[None, :, None] * int(l.pitch) + a[None, None, :]
        vals = lcg(2 * self.inner.size, 2000 + N).reshape(2, *self.inner.shape)

        def field(k):
            f = np.full(int(l.total), np.nan)  # ghost layer and row padding: NaN
            f[owned] = 0.0
            if k is not None:
                f[self.inner] = vals[k]
            return f

        self.prev, self.cur, self.v0 = field(0), field(1), field(None)
        # the CPU definition of v (it never reads the ghost layer: every interior value is finite)
        self.v = self.v0.copy()
        C.cpu_lap4(l, self.co, self.cur, self.v, self.full)
        assert np.isfinite(self.v[self.inner]).all() and same_bits(np.isnan(self.v), np.isnan(self.v0))

    def six_boxes(self):
        C, f = _C(), self.full
        m = (f.x0 + f.x1) // 2
        return [C.LBox(f.x0, f.x0 + 1, f.y0, f.y1, f.z0, f.z1), C.LBox(f.x1 - 2, f.x1, f.y0, f.y1, f.z0, f.z1),
                C.LBox(f.x0 + 1, m, f.y0, f.y0 + 3, f.z0, f.z1), C.LBox(f.x0 + 1, m, f.y1 - 1, f.y1, f.z0, f.z1),
                C.LBox(f.x0 + 1, m, f.y0 + 3, f.y1 - 1, f.z0, f.z0 + 1),
                C.LBox(f.x0 + 1, m, f.y0 + 3, f.y1 - 1, f.z1 - 3, f.z1)]


@functools.lru_cache(maxsize=None)
def _case(key):
    return Case(key)


def _reduced(part):
    p = part.cpu().numpy().reshape(-1, 2)
    return float(np.fmax.reduce(p[:, 0], initial=0.0)), float(p[:, 1].sum())


def _tiling(tiling):
    t = _C().LeapfrogTiling()
    t.variant = 0
    tiling = dict(tiling)
    min_chunk = tiling.pop("min_chunk", 16)
    for k, v in tiling.items():
        setattr(t, k, v)
    return t, min_chunk


# every built tile height; x chunks of 3 planes (fewer than the queue's 5) and of 1; the XCD remap and the non-temporal
# store on and off
TILINGS = [dict(ty=8), dict(ty=16), dict(ty=8, target_blocks=1 << 20, min_chunk=3),
           dict(ty=16, target_blocks=1 << 20, min_chunk=3, xcd_remap=False, nt_store=False),
           dict(ty=8, xcd_remap=False), dict(ty=8, nt_store=False, target_blocks=1 << 20, min_chunk=1)]


def _id(key, t, *rest):
    return "-".join([key, "-".join(f"{k}{int(v)}" for k, v in t.items()), *rest])


LAP = [pytest.param(key, t, boxes, id=_id(key, t, boxes))
       for key in CONFIGS for t in TILINGS for boxes in ("full", "six")
       if not (key == "N136-cube" and (boxes == "six" or "min_chunk" in t or "nt_store" in t))
       and not (key == "N6-cube" and boxes == "six")]


@pytest.mark.parametrize("key,tiling,boxes", LAP)
def test_lap4(key, tiling, boxes):
    C, c = _C(), _case(key)
    l = c.lay
    t, min_chunk = _tiling(tiling)
    bl = [c.full] if boxes == "full" else c.six_boxes()
    want = c.v0.copy()
    for b in bl:
        C.cpu_lap4(l, c.co, c.cur, want, b)
    cur, v = (torch.from_numpy(a).cuda() for a in (c.cur, c.v0))
    if "target_blocks" in tiling and boxes == "full":  # (the x march really is cut into chunks of min_chunk planes)
        assert C.gpu_leapfrog44_blocks(l, bl, t, min_chunk) >= math.ceil((c.N - 1) / min_chunk) > 1
    C.gpu_lap4(l, c.co, cur.data_ptr(), v.data_ptr(), bl, t, torch.cuda.current_stream().cuda_stream, min_chunk)
    torch.cuda.synchronize()
    assert same_bits(v.cpu().numpy(), want)
    assert same_bits(cur.cpu().numpy(), c.cur)
    if boxes == "full":
        assert same_bits(want, c.v)


STEP = [pytest.param(key, t, check, boxes, id=_id(key, t, "check" if check else "nocheck", boxes))
        for key in CONFIGS for t in TILINGS for check in (False, True) for boxes in ("full", "six")
        if not (key == "N136-cube" and (boxes == "six" or not check or t.get("min_chunk") == 1))
        and not (key == "N6-cube" and boxes == "six")]


@pytest.mark.parametrize("key,tiling,check,boxes", STEP)
def test_leapfrog44(key, tiling, check, boxes):
    C, c = _C(), _case(key)
    l = c.lay
    t, min_chunk = _tiling(tiling)
    assert C.gpu_leapfrog4_ty(t) == tiling["ty"]
    bl = [c.full] if boxes == "full" else c.six_boxes()
    want = c.prev.copy()
    acc = [0.0, 0.0]
    for b in bl:
        r = C.cpu_leapfrog44(l, c.co, c.cur, c.v, want, b, c.s_ext, 0.83, check)
        if check:
            acc = [max(acc[0], r[0]), acc[1] + r[1]]
    assert np.isfinite(want[c.inner]).all()
    cur, v, out = (torch.from_numpy(a).cuda() for a in (c.cur, c.v, c.prev))
    s = torch.from_numpy(np.array(c.s_ext)).cuda()
    nblk = C.gpu_leapfrog44_blocks(l, bl, t, min_chunk)
    part = torch.full((2 * max(nblk, 1),), float("nan"), dtype=torch.float64).cuda()
    C.gpu_leapfrog44(l, c.co, cur.data_ptr(), v.data_ptr(), out.data_ptr(), bl, s.data_ptr(), 0.83,
                     part.data_ptr() if check else 0, t, torch.cuda.current_stream().cuda_stream, min_chunk)
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), want)
    assert same_bits(cur.cpu().numpy(), c.cur) and same_bits(v.cpu().numpy(), c.v)
    if check:
        m, sm = _reduced(part)  # (every partial of the launch was written: none is NaN)
        assert m == acc[0] and math.isclose(sm, acc[1], rel_tol=1e-12)


def test_the_launchers_want_time_order_4_coefficients_and_a_whole_domain():
    C, c = _C(), _case("N24-cube")
    cur, v, out = (torch.from_numpy(a).cuda() for a in (c.cur, c.v, c.prev))
    s = torch.from_numpy(np.array(c.s_ext)).cuda()
    t = C.LeapfrogTiling()
    st = torch.cuda.current_stream().cuda_stream
    co42 = C.Coeffs.from_problem(C.Problem(c.N, 0.5 * c.prob.tau, 9, 1.0, order=4))
    with pytest.raises(Exception, match="time_order:"):
        C.gpu_lap4(c.lay, co42, cur.data_ptr(), v.data_ptr(), [c.full], t, st)
    with pytest.raises(Exception, match="time_order:"):
        C.gpu_leapfrog44(c.lay, co42, cur.data_ptr(), v.data_ptr(), out.data_ptr(), [c.full], s.data_ptr(), 0.0, 0, t, st)
    half = C.make_layout(c.prob, C.rank_box(c.prob, C.Dims(2, 1, 1), 0))
    with pytest.raises(Exception, match="time_order:"):
        C.gpu_leapfrog44_blocks(half, [C.compute_box(half)], t)
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), c.prev) and same_bits(v.cpu().numpy(), c.v)


@pytest.mark.parametrize("with_psi", [False, True], ids=["phi", "phi-psi"])
@pytest.mark.parametrize("key", list(CONFIGS))
def test_first_step_t4(key, with_psi):
    C, c = _C(), _case(key)
    l = c.lay
    src = C.initial_layout(c.prob, l)
    n1 = c.N + 1
    g = lcg(2 * n1 ** 3, 77 + c.N).reshape(2, -1)
    phi, psi = (C.initial_to_local(src, g[k]) for k in (0, 1))
    # outside the global grid the source arrays hold NaN, not zeros: the reflection must never read them
    a = np.arange(0, n1)
    inside = (int(src.off(0, 0, 0)) + a[:, None, None] * int(src.plane) + a[None, :, None] * int(src.pitch)
              + a[None, None, :])
    for f in (phi, psi):
        keep = f[inside].copy()
        f[:] = np.nan
        f[inside] = keep
    w0, w1, wv = np.full(int(l.total), 7.0), np.full(int(l.total), 7.0), c.v0.copy()
    C.cpu_first_step_t4(l, src, c.co, c.prob.tau, phi, psi if with_psi else None, wv, w0, w1)
    assert np.isfinite(w0).all() and np.isfinite(w1).all()
    d = [torch.from_numpy(x).cuda() for x in (phi, psi, c.v0)]
    g0, g1 = (torch.full((int(l.total),), 7.0, dtype=torch.float64).cuda() for _ in range(2))
    C.gpu_first_step_t4(l, src, c.co, c.prob.tau, d[0].data_ptr(), d[1].data_ptr() if with_psi else 0, d[2].data_ptr(),
                        g0.data_ptr(), g1.data_ptr(), C.LeapfrogTiling(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert same_bits(g0.cpu().numpy(), w0) and same_bits(g1.cpu().numpy(), w1) and same_bits(d[2].cpu().numpy(), wv)
    # ... and it is not the (4, 2) first step
    v0, v1 = np.zeros(int(l.total)), np.zeros(int(l.total))
    C.cpu_first_step_field(l, src, c.co, c.prob.tau, np.nan_to_num(phi), np.nan_to_num(psi) if with_psi else None, v0, v1)
    assert not same_bits(v1, w1)
