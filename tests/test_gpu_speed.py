"""A speed field c(x) on one GPU rank against CpuSolver, the definition: both stored levels bit for bit.

N = 24 (cube) and N = 40 (box 1 x 1.3 x 0.7), the two-layer and the random medium of tests/speed_reference.py, K = 21 and
one K = 203; temporal = 1 on both single-step kernels and the pair schedule (k_leapfrog2<VARC> pairs with single steps
where a check falls between, odd and even K, temporal = 2 and the default); first run, graph replay and run_batch; the
eigenmode start and set_initial; sources + receivers (traces bit-equal: single steps only) and a sponge; c = 1 gives the
speedless GPU solve's field_hash; set_speed after a captured solve re-captures; every refusal; both CLIs."""
import dataclasses
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from long_reference import long_shot
from sources_common import lcg_fields, same_bits
from speed_reference import random_medium, two_layer
from test_speed_cpu import speed_spec

from mpi_cuda_amd.solver import Solver
from mpi_cuda_amd.utils import dump as dumpio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEDIA = {"layers": two_layer, "random": random_medium}
GRIDS = {"N24-cube": (24, False), "N40-box": (40, True)}
SCHEDULES = {"t1-rq": dict(temporal=1), "t1-lds": dict(temporal=1, tiling={"variant": 0}), "pairs": dict(),
             "pairs-t2": dict(temporal=2), "pairs-rows4": dict(temporal=2, tiling={"rows": 4}, tiling2={"rows": 4}),
             "pairs-nograph": dict(temporal=2, graph=False)}


def _spec(grid, K, check_every=2):
    N, box = GRIDS[grid]
    return speed_spec(N, box, 2.0, K_=K, check_every=check_every)


def _arm(s, grid, K, mode):
    N = GRIDS[grid][0]
    if mode in ("initial", "sponge"):
        s.set_initial(*lcg_fields(N))
    if mode == "shot":
        shot = long_shot(N, GRIDS[grid][1])
        s.set_initial(np.zeros((N + 1,) * 3))
        s.set_sources(shot.sources, np.ascontiguousarray(shot.w[:K]))
        s.set_receivers(shot.receivers)
    return s


def _full_spec(grid, K, mode, check_every=2):
    spec = _spec(grid, K, check_every)
    return dataclasses.replace(spec, sponge=(5, 0.0, 63)) if mode == "sponge" else spec


@functools.lru_cache(maxsize=None)
def _cpu(grid, medium, K, mode, check_every=2):
    N = GRIDS[grid][0]
    s = _arm(Solver(_full_spec(grid, K, mode, check_every), backend="cpu", speed=MEDIA[medium](N)), grid, K, mode)
    r = s.run()
    return (s.global_field(0).numpy().copy(), s.global_field(1).numpy().copy(), r,
            s.traces().numpy().copy() if mode == "shot" else None, s.energy(0), s.energy(1))


def _check(s, r, ref, what, traces=False):
    uK, uK1, rc, tr, eK, e1 = ref
    assert same_bits(s.global_field(0).numpy(), uK), f"{what}: u^K differs from CpuSolver"
    assert same_bits(s.global_field(1).numpy(), uK1), f"{what}: u^K-1 differs from CpuSolver"
    assert r.steps == rc.steps and r.max_err == rc.max_err, what
    if traces:
        assert same_bits(s.traces().numpy(), tr), f"{what}: traces differ from CpuSolver"


@pytest.mark.parametrize("K", [21, 20])
@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("medium", list(MEDIA))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_fields_are_the_cpu_solvers(gpu, grid, medium, sched, K):
    """The eigenmode start (through the first-step-field path); first run, graph replay, run_batch(2)."""
    N = GRIDS[grid][0]
    s = Solver(_spec(grid, K), backend="hip", device=0, speed=MEDIA[medium](N), **SCHEDULES[sched])
    assert s.native.speed
    ref = _cpu(grid, medium, K, "eigen")
    for what in ("first run", "second run"):
        r = s.run()
        assert not s.native.analytic_start and s.native.stored_prev
        _check(s, r, ref, f"{sched} {what}")
    r = s.run_batch(2)[-1]
    _check(s, r, ref, f"{sched} run_batch")
    # the weighted energy through Solver.energy (download + cpu_energy): CpuSolver's own number
    assert s.energy(0) == ref[4] and s.energy(1) == ref[5]
    # traffic counts the lamf reads
    plain = Solver(_spec(grid, K), backend="hip", device=0, **{**SCHEDULES[sched], "tb": False})
    plain.run()
    if sched.startswith("t1"):
        assert s.traffic()["field_bytes"] > plain.traffic()["field_bytes"]


@pytest.mark.parametrize("mode", ["initial", "shot", "sponge"])
@pytest.mark.parametrize("sched", ["t1-rq", "t1-lds", "pairs"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_with_initial_shot_and_sponge(gpu, grid, sched, mode):
    N, K = GRIDS[grid][0], 21
    s = _arm(Solver(_full_spec(grid, K, mode), backend="hip", device=0, speed=two_layer(N), **SCHEDULES[sched]), grid, K, mode)
    ref = _cpu(grid, "layers", K, mode)
    for what in ("first run", "second run"):
        r = s.run()
        _check(s, r, ref, f"{sched} {mode} {what}", traces=mode == "shot")
    r = s.run_batch(2)[-1]
    _check(s, r, ref, f"{sched} {mode} run_batch", traces=mode == "shot")


def test_long_solve(gpu):
    grid, K = "N40-box", 203
    s = _arm(Solver(_spec(grid, K, 7), backend="hip", device=0, speed=random_medium(40)), grid, K, "initial")
    ref = _cpu(grid, "random", K, "initial", 7)
    for what in ("first run", "replay"):
        r = s.run()
        _check(s, r, ref, f"K=203 {what}")


@pytest.mark.parametrize("sched", ["t1-rq", "t1-lds", "pairs"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_unit_speed_is_the_speedless_gpu_solve(gpu, grid, sched):
    N, K = GRIDS[grid][0], 21
    kw = {**SCHEDULES[sched], "tb": False}  # (the speedless solve on the same unit list)
    a = Solver(_spec(grid, K), backend="hip", device=0, **kw)
    b = Solver(_spec(grid, K), backend="hip", device=0, speed=np.ones((N + 1,) * 3), **kw)
    ra, rb = a.run(), b.run()
    assert a.field_hash(0) == b.field_hash(0) and a.field_hash(1) == b.field_hash(1)
    assert ra.max_err == rb.max_err


def test_set_speed_recaptures_and_clears(gpu):
    grid, K = "N24-cube", 21
    N = 24
    s = Solver(_spec(grid, K), backend="hip", device=0, temporal=2)
    s.run(), s.run()  # captured, speedless
    plain = (s.field_hash(0), s.field_hash(1))
    s.set_speed(two_layer(N))
    for _ in range(2):
        _check(s, s.run(), _cpu(grid, "layers", K, "eigen"), "after set_speed")
    s.set_speed(random_medium(N))
    for _ in range(2):
        _check(s, s.run(), _cpu(grid, "random", K, "eigen"), "after a second set_speed")
    s.set_speed(None)
    s.run(), s.run()
    assert (s.field_hash(0), s.field_hash(1)) == plain


def test_refusals(gpu):
    from mpi_cuda_amd._native import load

    C = load()
    N = 24
    spec = _spec("N24-cube", 21)
    c = two_layer(N).reshape(-1)

    def native(world=1, **opts):
        o = C.SolverOptions()
        for k, v in opts.items():
            if k == "rows":
                o.tiling.rows = v
            else:
                setattr(o, k, v)
        return C.GpuSolver(spec.native(), o, 0, world, None)

    for kw, msg in ((dict(fake_comm=True, world=2), "speed: one GPU rank"), (dict(push=True), "speed: not on the push or copy"),
                    (dict(sdma=True), "speed: not on the push or copy"), (dict(rows=8), "speed: the register-queue single step with 8"),
                    (dict(temporal=3), "speed: temporal = 3"), (dict(temporal=4), "speed: temporal = 4")):
        with pytest.raises(RuntimeError, match="^wave3d: " + msg):
            native(**kw).set_speed(c)
    g = C.GpuGroup(spec.native(), C.SolverOptions(), 2, "loopback")
    assert not hasattr(g, "set_speed")
    s = native()
    s.set_speed(c)
    with pytest.raises(RuntimeError, match="^wave3d: speed: not together with set_state"):
        s.set_state(np.zeros((N + 1) ** 3), np.zeros((N + 1) ** 3), 3)
    s.run()
    with pytest.raises(RuntimeError, match="^wave3d: speed: k_energy has no mass weight"):
        s.energy(0)
    t = native()
    t.set_state(np.zeros((N + 1) ** 3), np.zeros((N + 1) ** 3), 3)
    with pytest.raises(RuntimeError, match="^wave3d: speed: not together with set_state"):
        t.set_speed(c)
    with pytest.raises(RuntimeError, match="^wave3d: speed: CFL"):
        native().set_speed(3.0 * c)
    with pytest.raises(RuntimeError, match="^wave3d: speed: every interior value"):
        native().set_speed(-c)
    for kw, msg in ((dict(transport="loopback", world=2, rank=0), "speed: one rank only"), (dict(runtime="process"), "speed: not with runtime"),
                    (dict(temporal=3), "speed: temporal=3"), (dict(copy_engines=True), "speed: one GPU rank")):
        with pytest.raises(ValueError, match=msg):
            Solver(spec, backend="hip", device=0, speed=c, **kw)


@pytest.mark.parametrize("cli", ["native", "python", "native-cpu"])
def test_cli_dump_equals_the_api(gpu, tmp_path, cli):
    N, K = 24, 21
    spec = _spec("N24-cube", K)
    c = two_layer(N)
    pre = str(tmp_path / "medium")
    dumpio.save(pre + ".c", c, N=N, L=1.0, tau=spec.tau, step=0)
    out, js = str(tmp_path / "out"), str(tmp_path / "summary.json")
    common = [str(N), repr(spec.tau), str(K), "--speed", pre, "--dump", out, "--json", js, "--quiet"]
    if cli == "python":
        cmd = [sys.executable, "-m", "mpi_cuda_amd", *common, "--backend", "hip"]
    else:
        cmd = [os.path.join(ROOT, "bin", "wave3d"), *common] + (["--cpu"] if cli == "native-cpu" else [])
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stderr.count("a speed field is set") == 1
    f, meta = dumpio.load(out)
    assert same_bits(f, _cpu("N24-cube", "layers", K, "eigen")[0])
    assert meta["speed"] == [1.0, 2.0] and json.load(open(js))["speed"] == [1.0, 2.0]
    # without --speed the sidecars do not name one
    p = subprocess.run([c_ for c_ in cmd if c_ not in ("--speed", pre)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "speed" not in dumpio.load(out)[1] and "speed" not in json.load(open(js))
