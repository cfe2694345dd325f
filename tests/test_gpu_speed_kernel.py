"""The VARC instantiations (a coefficient per node, lamf = lam c^2) of k_leapfrog_rq, k_leapfrog_lds, k_leapfrog2_rq and
k_first_step_field against the native CPU kernels, bit for bit.

lamf is random PER NODE on the global interior and NaN everywhere else (boundary nodes, ghost layers, row padding), so a
coefficient taken from a neighbouring node, row or plane shows in the bits and one taken from outside the interior shows as
NaN. The fields hold random values on the interior, exact zeros on the boundary and NaN in the ghost layers and the
padding. N = 24 (cube) and N = 40 (box 1 x 1.3 x 0.7): N - 1 is odd, so the last pair of a row is half boundary; N = 150:
a z row holds 75 pairs, more than one wave's 64, and 149 rows, more than one workgroup's. Outputs are compared over the
whole padded array: nothing outside the box is written."""
import functools
import math

import numpy as np
import pytest
import torch

from sources_common import BOX, same_bits

pytestmark = pytest.mark.gpu

CONFIGS = {"N24-cube": (24, False), "N40-box": (40, True), "N150-cube": (150, False)}


def _C():
    from mpi_cuda_amd._native import load

    return load()


class Case:
    def __init__(self, key):
        C = _C()
        self.N, box = CONFIGS[key]
        N = self.N
        self.prob = (C.Problem(N, 0.4 / (N * 3.2), 9, BOX[0], Ly=BOX[1], Lz=BOX[2]) if box
                     else C.Problem(N, 0.4 / (N * 1.8), 9, 1.0))
        self.co = C.Coeffs.from_problem(self.prob)
        self.lay = l = C.make_layout(self.prob, C.rank_box(self.prob, C.Dims(1, 1, 1), 0))
        self.s_ext = C.sin_table_ext(self.prob)
        self.full = C.compute_box(l)
        rng = np.random.default_rng(500 + N)
        i, a = np.arange(1, N), np.arange(0, N + 1)
        o = int(l.off(0, 0, 0))
        self.inner = o + i[:, None, None] * int(l.plane) + i[None, :, None] * int(l.pitch) + i[None, None, :]
        owned = o + a[:, None, None] * int(l.plane) + a[None, :, None] * int(l.pitch) + a[None, None, :]

        def field():
            f = np.full(int(l.total), np.nan)
            f[owned] = 0.0
            f[self.inner] = rng.standard_normal(self.inner.shape)
            return f

        self.prev, self.cur = field(), field()
        self.lamf = np.full(int(l.total), np.nan)
        self.lamf[self.inner] = self.co.lam * rng.uniform(0.25, 4.0, self.inner.shape)
        self.sponge = C.Problem(N, self.prob.tau, 9, self.prob.L, Ly=BOX[1] if box else 0.0, Lz=BOX[2] if box else 0.0,
                                sponge=C.Sponge(5, 0.0, 63))

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


TILINGS = [dict(variant=1, rows=1), dict(variant=1, rows=2), dict(variant=1, rows=4), dict(variant=0, ty=4),
           dict(variant=0, ty=8), dict(variant=0, ty=16), dict(variant=1, rows=2, nt_store=False, xcd_remap=False)]


# (the large case runs whole-interior launches only: its job is the second wave of a row and the second workgroup of a plane)
SINGLE = [pytest.param(key, t, check, damp, boxes,
                       id=f"{key}-{'-'.join(f'{k}{int(v)}' for k, v in t.items())}-{'check' if check else 'nocheck'}-"
                          f"{'damp' if damp else 'plain'}-{boxes}")
          for key in CONFIGS for t in TILINGS for check in (False, True) for damp in (False, True)
          for boxes in ("full", "six") if not (key == "N150-cube" and (boxes == "six" or not check))
          and not (damp and t == dict(variant=1, rows=4))]  # (VARC && DAMP is built at 1 and 2 rows and the LDS variant)


@pytest.mark.parametrize("key,tiling,check,damp,boxes", SINGLE)
def test_single_step(key, tiling, check, damp, boxes):
    C, c = _C(), _case(key)
    l = c.lay
    t = C.LeapfrogTiling()
    for k, v in tiling.items():
        setattr(t, k, v)
    assert C.gpu_leapfrog_speed_supported(t, damp)
    bl = [c.full] if boxes == "full" else c.six_boxes()
    want = c.prev.copy()
    acc = [0.0, 0.0]
    for b in bl:
        r = C.cpu_leapfrog(l, c.co, c.cur, want, b, c.s_ext, 0.83, check, c.sponge if damp else None, c.lamf)
        if check:
            acc = [max(acc[0], r[0]), acc[1] + r[1]]
    assert np.isfinite(want[c.inner]).all()
    cur, out, lamf = (torch.from_numpy(a).cuda() for a in (c.cur, c.prev, c.lamf))
    s = torch.from_numpy(np.array(c.s_ext)).cuda()
    tab = torch.from_numpy(C.sponge_tables(c.sponge).copy()).cuda()
    part = torch.zeros(2 * max(C.gpu_leapfrog_blocks(l, bl, t), 1), dtype=torch.float64).cuda()
    C.gpu_leapfrog(l, c.co, cur.data_ptr(), out.data_ptr(), bl, s.data_ptr(), 0.83, part.data_ptr() if check else 0, t,
                   torch.cuda.current_stream().cuda_stream, tab.data_ptr() if damp else 0, lamf.data_ptr())
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), want)
    assert same_bits(cur.cpu().numpy(), c.cur) and same_bits(lamf.cpu().numpy(), c.lamf)
    if check:
        m, sm = _reduced(part)
        assert m == acc[0] and math.isclose(sm, acc[1], rel_tol=1e-12)


def test_single_step_refuses_what_is_not_built():
    C, c = _C(), _case("N24-cube")
    cur, out, lamf = (torch.from_numpy(a).cuda() for a in (c.cur, c.prev, c.lamf))
    s = torch.from_numpy(np.array(c.s_ext)).cuda()
    t = C.LeapfrogTiling()
    tab = torch.from_numpy(C.sponge_tables(c.sponge).copy()).cuda()
    for rows, sponge in ((8, 0), (4, tab.data_ptr())):
        t.variant, t.rows = 1, rows
        assert not C.gpu_leapfrog_speed_supported(t, sponge != 0)
        with pytest.raises(Exception, match="speed:"):
            C.gpu_leapfrog(c.lay, c.co, cur.data_ptr(), out.data_ptr(), [c.full], s.data_ptr(), 0.0, 0, t,
                           torch.cuda.current_stream().cuda_stream, sponge, lamf.data_ptr())
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), c.prev)


@pytest.mark.parametrize("target_waves", [0, 50])
@pytest.mark.parametrize("check", [False, True], ids=["nocheck", "check"])
@pytest.mark.parametrize("rows", [1, 2, 4])
@pytest.mark.parametrize("key", list(CONFIGS))
def test_two_step_pass(key, rows, check, target_waves):
    """k_leapfrog2_rq<VARC>: both stages, the recomputed halo rows and the spare z lanes at their own node's lamf."""
    C, c = _C(), _case(key)
    l = c.lay
    a, b = c.prev.copy(), c.cur.copy()
    C.cpu_leapfrog(l, c.co, b, a, c.full, c.s_ext, lamf=c.lamf)  # a = u^{n+1}
    r = C.cpu_leapfrog(l, c.co, a, b, c.full, c.s_ext, 0.61, check, None, c.lamf)  # b = u^{n+2}
    t = C.Leapfrog2Tiling()
    t.rows, t.target_waves = rows, target_waves
    prev, cur, lamf = (torch.from_numpy(x).cuda() for x in (c.prev, c.cur, c.lamf))
    sent = np.full(int(l.total), -1234.5)
    o1, o2 = torch.from_numpy(sent).cuda(), torch.from_numpy(sent).cuda()
    s = torch.from_numpy(np.array(c.s_ext)).cuda()
    part = torch.zeros(2 * max(C.gpu_leapfrog2_partials(l, c.full, t), 1), dtype=torch.float64).cuda()
    C.gpu_leapfrog2(l, c.co, prev.data_ptr(), cur.data_ptr(), o1.data_ptr(), o2.data_ptr(), c.full, s.data_ptr(), 0.61,
                    part.data_ptr() if check else 0, t, torch.cuda.current_stream().cuda_stream, lamf=lamf.data_ptr())
    torch.cuda.synchronize()
    for got, want in ((o1, a), (o2, b)):
        exp = sent.copy()
        exp[c.inner] = want[c.inner]
        assert same_bits(got.cpu().numpy(), exp)
    if check:
        m, sm = _reduced(part)
        assert m == r[0] and math.isclose(sm, r[1], rel_tol=1e-12)


@pytest.mark.parametrize("with_psi", [False, True], ids=["nopsi", "psi"])
@pytest.mark.parametrize("key", list(CONFIGS))
def test_first_step_field(key, with_psi):
    C, c = _C(), _case(key)
    l, N = c.lay, c.N
    src = C.initial_layout(c.prob, l)
    rng = np.random.default_rng(77 + N)
    phi = C.initial_to_local(src, rng.standard_normal((N + 1) ** 3))
    psi = C.initial_to_local(src, rng.standard_normal((N + 1) ** 3)) if with_psi else None
    w0, w1 = np.full(int(l.total), 5.0), np.full(int(l.total), 5.0)
    C.cpu_first_step_field(l, src, c.co, c.prob.tau, phi, psi, w0, w1, c.lamf)
    assert np.isfinite(w1).all()
    d = [torch.from_numpy(a).cuda() if a is not None else None for a in (phi, psi, c.lamf)]
    g0 = torch.full((int(l.total),), 7.0, dtype=torch.float64).cuda()
    g1 = g0.clone()
    C.gpu_first_step_field(l, src, c.co, c.prob.tau, d[0].data_ptr(), d[1].data_ptr() if with_psi else 0, g0.data_ptr(),
                           g1.data_ptr(), torch.cuda.current_stream().cuda_stream, d[2].data_ptr())
    torch.cuda.synchronize()
    assert same_bits(g0.cpu().numpy(), w0) and same_bits(g1.cpu().numpy(), w1)
