"""The tile planner of the single-step kernels: gpu_leapfrog_blocks, gpu_leapfrog4_blocks and gpu_leapfrog44_blocks
against literal counts, on the shapes of the order-4 kernel tests. Host only: the bindings run no device code.

The literals below were printed by this file at the commit before the planners were merged:
    PYTHONPATH=. python tests/test_tile_planner.py
(it prints ORDER2 and ORDER4 as they stand here). Per (shape, boxes) the counts are in the order of `order2_args` /
`order4_args`."""
import itertools
from types import SimpleNamespace

import pytest

from sources_common import BOX
from test_gpu_order4_kernel import CONFIGS, Case


def _C():
    from mpi_cuda_amd._native import load

    return load()


def _layout(key):
    C = _C()
    N, box = CONFIGS[key]
    prob = (C.Problem(N, 0.4 / (N * 3.2), 9, BOX[0], Ly=BOX[1], Lz=BOX[2], order=4) if box
            else C.Problem(N, 0.4 / (N * 1.8), 9, 1.0, order=4))
    return prob, C.make_layout(prob, C.rank_box(prob, C.Dims(1, 1, 1), 0))


def _boxes(l, kind):
    C = _C()
    full = C.compute_box(l)
    if kind == "full":
        return [full]
    six = Case.six_boxes(SimpleNamespace(full=full))
    if kind == "six":
        return six
    return [six[0], C.LBox(full.x0, full.x0, full.y0, full.y1, full.z0, full.z1), six[1], six[5]]  # "empty": one inside


def _tiling(**kw):
    t = _C().LeapfrogTiling()
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def order2_args():
    """every tile height of the LDS step, every row count of the register-queue step; target default and 1 << 20; remap"""
    kinds = [dict(variant=0, ty=ty) for ty in (4, 8, 16)] + [dict(variant=1, rows=r) for r in (1, 2, 4, 8)]
    return [dict(k, target_blocks=tb, xcd_remap=x) for k, tb, x in itertools.product(kinds, (0, 1 << 20), (True, False))]


def order4_args():
    """(tiling, min_chunk): ty 4, 8, 16 (4 runs the 8-row tile); target default and 1 << 20; floor 1, 3, 16; remap"""
    return [(dict(variant=0, ty=ty, target_blocks=tb, xcd_remap=x), mc)
            for ty, tb, mc, x in itertools.product((4, 8, 16), (0, 1 << 20), (1, 3, 16), (True, False))]


def counts(key, kind):
    C = _C()
    _, l = _layout(key)
    bl = _boxes(l, kind)
    o2 = [C.gpu_leapfrog_blocks(l, bl, _tiling(**a)) for a in order2_args()]
    o4 = [C.gpu_leapfrog4_blocks(l, bl, _tiling(**a), mc) for a, mc in order4_args()]
    o44 = [C.gpu_leapfrog44_blocks(l, bl, _tiling(**a), mc) for a, mc in order4_args()]
    return o2, o4, o44


CASES = [(key, kind) for key in CONFIGS for kind in ("full", "six", "empty")]

ORDER2 = {
    ('N6-cube', 'full'): [8, 2, 8, 2, 8, 1, 8, 1, 8, 1, 8, 1, 32, 8, 32, 8, 32, 4, 32, 4, 32, 4, 32, 4, 32, 4, 32, 4],
    ('N6-cube', 'six'): [8, 8, 8, 8, 8, 6, 8, 6, 8, 6, 8, 6, 32, 16, 32, 16, 32, 12, 32, 12, 32, 8, 32, 8, 32, 8, 32, 8],
    ('N6-cube', 'empty'): [8, 5, 8, 5, 8, 3, 8, 3, 8, 3, 8, 3, 32, 12, 32, 12, 32, 8, 32, 8, 32, 8, 32, 8, 32, 4, 32, 4],
    ('N24-cube', 'full'): [16, 12, 16, 12, 8, 6, 8, 6, 8, 4, 8, 4, 64, 48, 64, 48, 32, 24, 32, 24, 32, 12, 32, 12, 32, 8, 32, 8],
    ('N24-cube', 'six'): [24, 24, 24, 24, 16, 14, 16, 14, 16, 10, 16, 10, 96, 88, 96, 88, 64, 48, 64, 48, 32, 24, 32, 24, 32, 16, 32, 16],
    ('N24-cube', 'empty'): [24, 17, 24, 17, 16, 9, 16, 9, 8, 6, 8, 6, 96, 68, 96, 68, 64, 36, 64, 36, 32, 20, 32, 20, 32, 12, 32, 12],
    ('N40-box', 'full'): [32, 30, 32, 30, 16, 15, 16, 15, 16, 9, 16, 9, 128, 120, 128, 120, 64, 60, 64, 60, 32, 32, 32, 32, 32, 16, 32, 16],
    ('N40-box', 'six'): [64, 60, 64, 60, 40, 34, 40, 34, 24, 22, 24, 22, 256, 228, 256, 228, 128, 120, 128, 120, 64, 60, 64, 60, 64, 36, 64, 36],
    ('N40-box', 'empty'): [40, 38, 40, 38, 24, 20, 24, 20, 16, 12, 16, 12, 160, 148, 160, 148, 96, 76, 96, 76, 64, 40, 64, 40, 32, 20, 32, 20],
    ('N136-cube', 'full'): [616, 612, 616, 612, 312, 306, 312, 306, 168, 162, 168, 162, 2432, 2432, 2432, 2432, 1248, 1224, 1248, 1224, 640, 612, 640, 612, 320, 308, 320, 308],
    ('N136-cube', 'six'): [488, 486, 488, 486, 264, 258, 264, 258, 152, 146, 152, 146, 1920, 1892, 1920, 1892, 992, 964, 992, 964, 512, 488, 512, 488, 288, 260, 288, 260],
    ('N136-cube', 'empty'): [304, 301, 304, 301, 160, 153, 160, 153, 88, 81, 88, 81, 1216, 1196, 1216, 1196, 608, 604, 608, 604, 320, 304, 320, 304, 160, 156, 160, 156],
}
ORDER4 = {
    ('N6-cube', 'full'): [8, 5, 8, 2, 8, 1, 8, 5, 8, 2, 8, 1, 8, 5, 8, 2, 8, 1, 8, 5, 8, 2, 8, 1, 8, 5, 8, 2, 8, 1, 8, 5, 8, 2, 8, 1],
    ('N6-cube', 'six'): [8, 7, 8, 6, 8, 6, 8, 7, 8, 6, 8, 6, 8, 7, 8, 6, 8, 6, 8, 7, 8, 6, 8, 6, 8, 7, 8, 6, 8, 6, 8, 7, 8, 6, 8, 6],
    ('N6-cube', 'empty'): [8, 4, 8, 3, 8, 3, 8, 4, 8, 3, 8, 3, 8, 4, 8, 3, 8, 3, 8, 4, 8, 3, 8, 3, 8, 4, 8, 3, 8, 3, 8, 4, 8, 3, 8, 3],
    ('N24-cube', 'full'): [72, 69, 24, 24, 8, 6, 72, 69, 24, 24, 8, 6, 72, 69, 24, 24, 8, 6, 72, 69, 24, 24, 8, 6, 48, 46, 16, 16, 8, 4, 48, 46, 16, 16, 8, 4],
    ('N24-cube', 'six'): [96, 89, 40, 38, 16, 14, 96, 89, 40, 38, 16, 14, 96, 89, 40, 38, 16, 14, 96, 89, 40, 38, 16, 14, 72, 66, 32, 28, 16, 10, 72, 66, 32, 28, 16, 10],
    ('N24-cube', 'empty'): [40, 39, 24, 18, 16, 9, 40, 39, 24, 18, 16, 9, 40, 39, 24, 18, 16, 9, 40, 39, 24, 18, 16, 9, 32, 26, 16, 12, 8, 6, 32, 26, 16, 12, 8, 6],
    ('N40-box', 'full'): [200, 195, 72, 65, 16, 15, 200, 195, 72, 65, 16, 15, 200, 195, 72, 65, 16, 15, 200, 195, 72, 65, 16, 15, 120, 117, 40, 39, 16, 9, 120, 117, 40, 39, 16, 9],
    ('N40-box', 'six'): [232, 231, 88, 82, 40, 34, 232, 231, 88, 82, 40, 34, 232, 231, 88, 82, 40, 34, 232, 231, 88, 82, 40, 34, 160, 153, 56, 54, 24, 22, 160, 153, 56, 54, 24, 22],
    ('N40-box', 'empty'): [112, 105, 40, 40, 24, 20, 112, 105, 40, 40, 24, 20, 112, 105, 40, 40, 24, 20, 112, 105, 40, 40, 24, 20, 64, 63, 24, 24, 16, 12, 64, 63, 24, 24, 16, 12],
    ('N136-cube', 'full'): [1536, 1530, 1536, 1530, 312, 306, 4592, 4590, 1536, 1530, 312, 306, 1536, 1530, 1536, 1530, 312, 306, 4592, 4590, 1536, 1530, 312, 306, 1224, 1224, 816, 810, 168, 162, 2432, 2430, 816, 810, 168, 162],
    ('N136-cube', 'six'): [752, 748, 720, 714, 264, 258, 2616, 2610, 904, 904, 264, 258, 752, 748, 720, 714, 264, 258, 2616, 2610, 904, 904, 264, 258, 784, 780, 520, 520, 152, 146, 1512, 1506, 520, 520, 152, 146],
    ('N136-cube', 'empty'): [480, 476, 448, 442, 160, 153, 1224, 1224, 448, 442, 160, 153, 480, 476, 448, 442, 160, 153, 1224, 1224, 448, 442, 160, 153, 352, 351, 240, 234, 88, 81, 648, 648, 240, 234, 88, 81],
}


@pytest.mark.parametrize("key,kind", CASES, ids=[f"{k}-{b}" for k, b in CASES])
def test_block_counts(key, kind):
    o2, o4, o44 = counts(key, kind)
    assert o4 == o44  # one planner: equal arguments, equal counts
    assert o2 == ORDER2[key, kind]
    assert o4 == ORDER4[key, kind]


def test_default_min_chunk_is_16():
    C = _C()
    _, l = _layout("N40-box")
    bl = _boxes(l, "six")
    for a, mc in order4_args():
        if mc == 16:
            assert C.gpu_leapfrog4_blocks(l, bl, _tiling(**a)) == C.gpu_leapfrog4_blocks(l, bl, _tiling(**a), 16)
            assert C.gpu_leapfrog44_blocks(l, bl, _tiling(**a)) == C.gpu_leapfrog44_blocks(l, bl, _tiling(**a), 16)


def _raises(text, f, *a):
    with pytest.raises(RuntimeError) as e:
        f(*a)
    assert str(e.value) == "wave3d: " + text


def test_refusals_keep_their_text():
    C = _C()
    prob, l = _layout("N24-cube")
    full, t = C.compute_box(l), _tiling(variant=0)
    half = C.make_layout(prob, C.rank_box(prob, C.Dims(2, 1, 1), 0))
    span = "the fourth-order step needs one rank's layout that spans the whole domain"
    _raises("order: " + span, C.gpu_leapfrog4_blocks, half, [C.compute_box(half)], t)
    _raises("time_order: " + span, C.gpu_leapfrog44_blocks, half, [C.compute_box(half)], t)
    for f in (C.gpu_leapfrog_blocks, C.gpu_leapfrog4_blocks, C.gpu_leapfrog44_blocks):
        _raises("too many boxes in one leapfrog launch", f, l, [full] * 7, t)
    _raises("order: the x chunk floor must be >= 1", C.gpu_leapfrog4_blocks, l, [full], t, 0)
    _raises("time_order: the x chunk floor must be >= 1", C.gpu_leapfrog44_blocks, l, [full], t, 0)


if __name__ == "__main__":
    o2, o4 = {}, {}
    for key, kind in CASES:
        o2[key, kind], o4[key, kind], o44 = counts(key, kind)
        assert o4[key, kind] == o44
    for name, d in (("ORDER2", o2), ("ORDER4", o4)):
        print(name + " = {")
        for k, v in d.items():
            print(f"    {k!r}: {v},")
        print("}")
