"""A speed field c(x) on the fused pair-tiled passes (k_leapfrog_p2<VARC>, SpeedPlan::kFused) against CpuSolver, the
definition: both stored levels and the error log bit for bit.

N = 40 (box 1 x 1.3 x 0.7: 2 x 2 tiles, the last pair of a row half boundary) and N = 72 (cube: 3 x 3 tiles, one of them
interior), K = 23 — K - 1 = 22 is no multiple of 2, 3 or 4, so every plan ends in a shorter tail pass — check cadence 1
(every level of every pass checked) and 4; the default schedule, also asked for as temporal = 5 (the plan then holds 3-
and 4-step passes; set_speed keeps refusing temporal = 3 and 4, tests/test_gpu_speed.py); the two-layer and the random
medium of tests/speed_reference.py, c in [0.5, 2] and [1, 2]; first run, graph replay; set_initial; set_speed(None)
afterwards. With receivers, a source or a sponge the solve still runs single steps and still matches."""
import dataclasses
import functools

import numpy as np
import pytest

from long_reference import long_shot
from sources_common import lcg_fields, same_bits
from speed_reference import random_medium, two_layer
from test_speed_cpu import speed_spec

from mpi_cuda_amd.solver import Solver

pytestmark = pytest.mark.gpu

K = 23
GRIDS = {"N40-box": (40, True), "N72-cube": (72, False)}
SCHEDULES = {"default": dict(), "t5": dict(temporal=5), "t5-nograph": dict(temporal=5, graph=False)}


def _random_wide(N):
    """c in [0.5, 2] per node (speed_reference.random_medium is [1, 2])."""
    return 0.5 + 1.5 * np.random.default_rng(9000 + N).random((N + 1,) * 3)


MEDIA = {"layers": two_layer, "random": _random_wide}


def _spec(grid, every, mode="eigen"):
    N, box = GRIDS[grid]
    spec = speed_spec(N, box, 2.0, K_=K, check_every=every)
    return dataclasses.replace(spec, sponge=(5, 0.0, 63)) if mode == "sponge" else spec


def _arm(s, grid, mode):
    N, box = GRIDS[grid]
    if mode in ("initial", "sponge"):
        s.set_initial(*lcg_fields(N))
    if mode in ("source", "receivers"):
        shot = long_shot(N, box)
        s.set_initial(np.zeros((N + 1,) * 3) if mode == "source" else lcg_fields(N)[0])
        if mode == "source":
            s.set_sources(shot.sources, np.ascontiguousarray(shot.w[:K]))
        else:
            s.set_receivers(shot.receivers)
    return s


@functools.lru_cache(maxsize=None)
def _cpu(grid, medium, every, mode="eigen"):
    N = GRIDS[grid][0]
    s = _arm(Solver(_spec(grid, every, mode), backend="cpu", speed=MEDIA[medium](N)), grid, mode)
    r = s.run()
    return (s.global_field(0).numpy().copy(), s.global_field(1).numpy().copy(), r,
            s.traces().numpy().copy() if mode == "receivers" else None)


def _check(s, r, ref, what):
    uK, uK1, rc, tr = ref
    assert same_bits(s.global_field(0).numpy(), uK), f"{what}: u^K differs from CpuSolver"
    assert s.native.stored_prev, f"{what}: u^K-1 was not stored"
    assert same_bits(s.global_field(1).numpy(), uK1), f"{what}: u^K-1 differs from CpuSolver"
    assert r.steps == rc.steps, what
    assert same_bits(np.asarray(r.max_err, dtype=np.float64), np.asarray(rc.max_err, dtype=np.float64)), f"{what}: error log"
    if tr is not None:
        assert same_bits(s.traces().numpy(), tr), f"{what}: traces differ from CpuSolver"


def _depth(sched):
    from mpi_cuda_amd._native import load

    return min(SCHEDULES[sched].get("temporal", 5), load().p2_varc_max_stages)


@pytest.mark.parametrize("every", [1, 4])
@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("medium", list(MEDIA))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_fused_solve_is_the_cpu_solvers(gpu, grid, medium, sched, every):
    """The eigenmode start; first run and graph replay; the units are fused passes of the asked depth."""
    N = GRIDS[grid][0]
    s = Solver(_spec(grid, every), backend="hip", device=0, speed=MEDIA[medium](N), **SCHEDULES[sched])
    assert s.native.speed
    ref = _cpu(grid, medium, every)
    for what in ("first run", "graph replay"):
        r = s.run()
        assert not s.native.analytic_start
        _check(s, r, ref, f"{sched} {what}")
        steps = list(s.native.unit_steps)
        assert sum(steps) == K - 1 and max(steps) == _depth(sched) > 2, steps
        assert len(steps) == -(-(K - 1) // _depth(sched)), steps  # (whole passes and one tail)


def test_default_plans_fused_passes(gpu):
    """The default schedule with a speed field planned two-step pairs: it now plans passes of more than two steps, of
    both built depths above two (K - 1 = 22 = 3 + 3 + 4 + 4 + 4 + 4 at the deepest built depth of 4)."""
    N = 40
    s = Solver(_spec("N40-box", 4), backend="hip", device=0, speed=two_layer(N))
    s.run()
    steps = list(s.native.unit_steps)
    assert max(steps) == _depth("default") > 2 and min(steps) > 2 and sum(steps) == K - 1, steps
    assert len(set(steps)) > 1, steps  # (a tail pass shorter than the deepest one ran too)


@pytest.mark.parametrize("grid", list(GRIDS))
def test_set_initial_then_clear(gpu, grid):
    """set_initial + speed on fused passes; set_speed(None) afterwards returns to the constant-speed bits."""
    N = GRIDS[grid][0]
    plain = Solver(_spec(grid, 4), backend="hip", device=0)
    plain.set_initial(*lcg_fields(N))
    plain.run()
    want = (plain.field_hash(0), plain.field_hash(1))
    s = _arm(Solver(_spec(grid, 4), backend="hip", device=0, speed=two_layer(N)), grid, "initial")
    ref = _cpu(grid, "layers", 4, "initial")
    for what in ("first run", "graph replay"):
        _check(s, s.run(), ref, f"set_initial {what}")
        assert max(s.native.unit_steps) > 2
    s.set_speed(None)
    s.run(), s.run()
    assert (s.field_hash(0), s.field_hash(1)) == want


@pytest.mark.parametrize("mode", ["receivers", "source", "sponge"])
def test_single_steps_where_no_coefficient_form_exists(gpu, mode):
    """Receivers, a source or a sponge: the cone and sponge-box kernels have no coefficient form, so these solves keep
    running single steps — and keep matching CpuSolver."""
    grid, N = "N40-box", 40
    s = _arm(Solver(_spec(grid, 4, mode), backend="hip", device=0, speed=two_layer(N)), grid, mode)
    ref = _cpu(grid, "layers", 4, mode)
    for what in ("first run", "graph replay"):
        _check(s, s.run(), ref, f"{mode} {what}")
        assert set(s.native.unit_steps) == {1}


def test_traffic_falls_by_the_planned_ratio(gpu):
    """field_bytes from the unit plan: a pass of S steps moves 2 reads + 2 writes + the lamf read = 5 node-fields, a pair
    the same 5 for 2 steps, a single step 3 + 1; the first-step kernel writes 2 and reads lamf."""
    grid, N = "N72-cube", 72
    nodes = 8.0 * (N - 1) ** 3
    got = {}
    for name, kw in (("fused", dict()), ("pairs", dict(temporal=2))):
        s = Solver(_spec(grid, 0), backend="hip", device=0, speed=two_layer(N), **kw)
        s.run()
        steps = list(s.native.unit_steps)
        want = nodes * (3.0 + sum(5.0 if st >= 2 else 4.0 for st in steps))
        got[name] = s.traffic()["field_bytes"]
        print(f"{name}: units {steps} field_bytes {got[name]:.6e} planned {want:.6e}")
        assert got[name] == want
    d = _depth("default")
    n_fused, n_pairs = -(-(K - 1) // d), (K - 1) // 2 + (K - 1) % 2
    # (K - 1 = 22 steps, check at the end only: 11 pairs against ceil(22 / depth) passes)
    assert got["fused"] / got["pairs"] == (3.0 + 5.0 * n_fused) / (3.0 + 5.0 * n_pairs)
