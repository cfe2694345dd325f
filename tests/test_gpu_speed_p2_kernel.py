"""The VARC instantiations of the pair-tiled S-step pass (k_leapfrog_p2 with a coefficient per node, lamf = lam c^2)
against S applications of the native CPU step with the same lamf, bit for bit.

The inputs are those of test_gpu_speed_kernel.py (its Case): lamf random PER NODE on the global interior and NaN
everywhere else (boundary nodes, ghost layers, row padding), so a coefficient taken from a neighbouring node, row or plane
shows in the bits and one taken from outside the interior shows as NaN; fields random on the interior, exact zeros on the
boundary, NaN in ghosts and padding. N = 24 (cube), N = 40 (box; N - 1 odd: the last pair of a row is half boundary),
N = 150 (5 x 5 tiles: interior tiles, the second wave of a row). Outputs are compared over the whole padded array against
a sentinel: the pass writes its boxes and, where a box ends at the last interior node, the +0 of the boundary node that
shares the last pair (as the constant-speed pass does), nothing else."""
import functools
import math

import numpy as np
import pytest
import torch

from sources_common import same_bits
from test_gpu_speed_kernel import CONFIGS, _C, _case

pytestmark = pytest.mark.gpu

SENT = -1234.5
CT = [0.83, 0.61, 0.47, 0.29, 0.13]


def _built():
    return list(range(2, _C().p2_varc_max_stages + 1))


STAGES = [2, 3, 4]  # (== _built(): asserted in test_built_depths; a literal so that collection needs no extension)
MASKS = {"none": lambda S: 0, "even": lambda S: 0b01010 & ((1 << S) - 1), "odd": lambda S: 0b10101 & ((1 << S) - 1),
         "full": lambda S: (1 << S) - 1}


def test_built_depths():
    assert STAGES == _built()


@functools.lru_cache(maxsize=None)
def _levels(key, plane_lamf=False):
    """u^{n+k}, k = 1..max S, by the CPU step over the whole compute box (level[0] = cur, level[-1] = prev)."""
    C, c = _C(), _case(key)
    lamf = _plane_lamf(key) if plane_lamf else c.lamf
    lv = {-1: c.prev, 0: c.cur}
    for k in range(1, max(STAGES) + 1):
        out = lv[k - 2].copy()
        C.cpu_leapfrog(c.lay, c.co, lv[k - 1], out, c.full, c.s_ext, lamf=lamf)
        assert np.isfinite(out[c.inner]).all()
        lv[k] = out
    return lv


@functools.lru_cache(maxsize=None)
def _plane_lamf(key):
    """lamf depending on x only, one distinct value per plane (NaN outside the interior as ever): a coefficient queue that
    is off by one plane changes every node of every plane."""
    c = _case(key)
    N = c.N
    f = np.full_like(c.lamf, np.nan)
    per_plane = c.co.lam * (0.3 + 3.0 * (np.arange(1, N) * 0.6180339887 % 1.0))
    f[c.inner] = np.broadcast_to(per_plane[:, None, None], c.inner.shape)
    return f


def _errors(key, lv, k, boxes, lamf):
    """CPU error values of level k over the boxes: the step from the reference levels again, box by box."""
    C, c = _C(), _case(key)
    acc = [0.0, 0.0]
    for b in boxes:
        scratch = lv[k - 2].copy()
        r = C.cpu_leapfrog(c.lay, c.co, lv[k - 1], scratch, b, c.s_ext, CT[k - 1], True, None, lamf)
        acc = [max(acc[0], r[0]), acc[1] + r[1]]
    return acc


def _six_boxes(c):
    """Six disjoint boxes the pair-tiled pass takes (z cuts on whole pairs from the first interior node)."""
    C, f = _C(), c.full
    m = (f.x0 + f.x1) // 2
    zc = f.z1 - 3 - (f.z1 - 3 - f.z0) % 2  # (a pair start: same parity as f.z0)
    return [C.LBox(f.x0, f.x0 + 1, f.y0, f.y1, f.z0, f.z1), C.LBox(f.x1 - 2, f.x1, f.y0, f.y1, f.z0, f.z1),
            C.LBox(f.x0 + 1, m, f.y0, f.y0 + 3, f.z0, f.z1), C.LBox(f.x0 + 1, m, f.y1 - 1, f.y1, f.z0, f.z1),
            C.LBox(f.x0 + 1, m, f.y0 + 3, f.y1 - 1, f.z0, f.z0 + 2), C.LBox(f.x0 + 1, m, f.y0 + 3, f.y1 - 1, zc, f.z1)]


def _expected(c, level, boxes):
    """The sentinel, the level's values on the boxes, and +0 on the boundary node that shares a box's last pair."""
    l, f = c.lay, c.full
    exp = np.full(int(l.total), SENT)
    o, P, pitch = int(l.off(0, 0, 0)), int(l.plane), int(l.pitch)
    for b in boxes:
        x, y = np.arange(b.x0, b.x1), np.arange(b.y0, b.y1)
        z = np.arange(b.z0, b.z1)
        idx = o + x[:, None, None] * P + y[None, :, None] * pitch + z[None, None, :]
        exp[idx] = level[idx]
        if b.z1 == f.z1 and (b.z1 - b.z0) % 2 == 1:
            exp[o + x[:, None] * P + y[None, :] * pitch + b.z1] = 0.0
    return exp


def _run(c, S, mask, boxes, lamf, tiling=None, real=None, prev=None, cur=None, out1=True, analytic=False, via_tb=False):
    C = _C()
    l = c.lay
    t = C.LeapfrogTbTiling()
    t.stages = S
    t.target_blocks = 1
    for k, v in (tiling or {}).items():
        setattr(t, k, v)
    nb = max(C.p2_launch_blocks(boxes, t)[0], 1)
    dev = [torch.from_numpy(a).cuda() for a in (c.prev if prev is None else prev, c.cur if cur is None else cur)]
    lam = torch.from_numpy(lamf).cuda() if lamf is not None else None
    sent = np.full(int(l.total), SENT)
    o1, o2 = torch.from_numpy(sent).cuda(), torch.from_numpy(sent).cuda()
    s = torch.from_numpy(np.array(c.s_ext)).cuda()
    part = torch.zeros(2 * S * nb, dtype=torch.float64).cuda()
    kw = dict(lamf=lam.data_ptr() if lam is not None else 0, analytic_start=analytic)
    if real is not None:
        kw["real"] = real
    args = (l, c.co, dev[0].data_ptr(), dev[1].data_ptr(), o1.data_ptr() if out1 else 0, o2.data_ptr())
    tail = (s.data_ptr(), CT[:S], mask, part.data_ptr() if mask else 0, t, torch.cuda.current_stream().cuda_stream)
    if via_tb:
        C.gpu_leapfrog_tb(*args, boxes[0], *tail, **kw)
    else:
        C.gpu_leapfrog_p2_boxes(*args, boxes, *tail, **kw)
    torch.cuda.synchronize()
    assert same_bits(dev[0].cpu().numpy(), c.prev if prev is None else prev)
    assert same_bits(dev[1].cpu().numpy(), c.cur if cur is None else cur)
    if lam is not None:
        assert same_bits(lam.cpu().numpy(), lamf)
    p = part.cpu().numpy().reshape(S, nb, 2)
    red = {k: (float(np.fmax.reduce(p[k - 1, :, 0], initial=0.0)), float(p[k - 1, :, 1].sum())) for k in range(1, S + 1)}
    return o1.cpu().numpy(), o2.cpu().numpy(), red


def _compare(key, S, mask, boxes, got, lv, lamf):
    c = _case(key)
    o1, o2, red = got
    assert same_bits(o2, _expected(c, lv[S], boxes)), "u^{n+S} differs from S CPU steps"
    assert same_bits(o1, _expected(c, lv[S - 1], boxes)), "u^{n+S-1} differs from S - 1 CPU steps"
    for k in range(1, S + 1):
        if mask >> (k - 1) & 1:
            want = _errors(key, lv, k, boxes, lamf)
            print(f"level {k}: max {red[k][0]!r} / {want[0]!r}  sumsq {red[k][1]!r} / {want[1]!r}")
            assert red[k][0] == want[0] and math.isclose(red[k][1], want[1], rel_tol=1e-12)


PASS = [pytest.param(key, S, m, boxes, id=f"{key}-S{S}-{m}-{boxes}")
        for key in CONFIGS for S in STAGES for m in MASKS for boxes in ("full", "six")]


@pytest.mark.parametrize("key,S,mask,boxes", PASS)
def test_pass_equals_cpu_steps(key, S, mask, boxes):
    c = _case(key)
    bl = [c.full] if boxes == "full" else _six_boxes(c)
    m = MASKS[mask](S)
    _compare(key, S, m, bl, _run(c, S, m, bl, c.lamf), _levels(key), c.lamf)


@pytest.mark.parametrize("S", STAGES)
@pytest.mark.parametrize("key,target", [("N150-cube", 256), ("N40-box", 64)])
def test_chunked_x(key, target, S):
    """The CH instantiations: x split into chunks, each with its own prologue load of the coefficient plane."""
    C, c = _C(), _case(key)
    t = C.LeapfrogTbTiling()
    t.stages, t.target_blocks = S, target
    assert C.p2_launch_blocks([c.full], t)[1][0][3] > 1  # (x chunks)
    m = MASKS["full"](S)
    _compare(key, S, m, [c.full], _run(c, S, m, [c.full], c.lamf, tiling=dict(target_blocks=target)), _levels(key), c.lamf)


@pytest.mark.parametrize("S", STAGES)
@pytest.mark.parametrize("key", ["N24-cube", "N40-box"])
def test_real_range_narrower_than_the_compute_box(key, S):
    """A box inside the x range whose stage-real range is just its halo: the general head and tail iterations zero a
    stage (xreal) whose coefficient plane is still loaded, queued and consumed."""
    C, c = _C(), _case(key)
    f = c.full
    b = C.LBox(f.x0 + 6, f.x1 - 7, f.y0, f.y1, f.z0, f.z1)
    real = C.LBox(b.x0 - (S - 1), b.x1 + (S - 1), 1, 0, 1, 0)
    m = MASKS["full"](S)
    _compare(key, S, m, [b], _run(c, S, m, [b], c.lamf, real=real), _levels(key), c.lamf)


@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
@pytest.mark.parametrize("S", STAGES)
@pytest.mark.parametrize("key", ["N24-cube", "N40-box"])
def test_plane_shift_detector(key, S, chunked):
    """lamf constant in y and z with a distinct value per x plane: every output plane is the CPU's."""
    c = _case(key)
    lamf = _plane_lamf(key)
    got = _run(c, S, 0, [c.full], lamf, tiling=dict(target_blocks=64) if chunked else None)
    lv = _levels(key, True)
    _compare(key, S, 0, [c.full], got, lv, lamf)
    l, N = c.lay, c.N
    o, P = int(l.off(0, 0, 0)), int(l.plane)
    for x in range(1, N):  # (plane by plane, for the message)
        sl = slice(o + x * P, o + (x + 1) * P)
        assert same_bits(got[1][sl], _expected(c, lv[S], [c.full])[sl]), f"plane {x}"


@pytest.mark.parametrize("S", STAGES)
@pytest.mark.parametrize("key", ["N24-cube", "N40-box"])
def test_unit_speed_is_the_constant_pass(key, S):
    """c = 1 (lamf = lam on the interior, 0 outside): the bits of the constant-speed pass from the same inputs."""
    c = _case(key)
    one = np.zeros_like(c.lamf)
    one[c.inner] = c.co.lam
    m = MASKS["full"](S)
    a = _run(c, S, m, [c.full], one)
    b = _run(c, S, m, [c.full], None)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[2] == b[2]


def test_refusals():
    C, c = _C(), _case("N24-cube")
    with pytest.raises(Exception, match="speed:"):
        _run(c, 3, 0, [c.full], c.lamf, analytic=True)
    with pytest.raises(Exception, match="speed:"):
        _run(c, 3, 0, [c.full], c.lamf, out1=False)
    with pytest.raises(Exception, match="speed:"):
        _run(c, 3, 0, [c.full], c.lamf, tiling=dict(p2=False), via_tb=True)
    for S in range(max(STAGES) + 1, 6):  # (an unbuilt depth)
        with pytest.raises(Exception, match="speed:"):
            _run(c, S, 0, [c.full], c.lamf)
    f = c.full
    with pytest.raises(Exception, match="speed:"):  # (a box that starts in the middle of a pair)
        _run(c, 3, 0, [C.LBox(f.x0, f.x1, f.y0, f.y1, f.z0 + 1, f.z1)], c.lamf)
