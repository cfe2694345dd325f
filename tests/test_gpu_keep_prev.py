"""u^{K-1} after a solve whose last pass left it out (UnitPlan::drop_prev, the default) against a keep_prev=True
solver, which stores both levels in every pass: error logs, u^K, and — through each of the three accessors that
rebuild the level, download(1), field_hash(1), energy(0) — u^{K-1}, bit for bit; after run_batch, after a second
run(), from set_initial data, from a set_state resume, and on every rank of in-process groups.

K picks the last unit (default options, from the schedule itself: tests/test_drop_prev_native.py): K = 5 the analytic
start alone, 6 a single step (nothing to drop), 7 / 8 / 9 a 2- / 3- / 4-step pass, 20 a 5-step split-store pass."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from mpi_cuda_amd import ProblemSpec
from mpi_cuda_amd.solver import Solver

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAST_UNIT = {5: "analytic start alone", 6: "single step", 7: "S = 2", 8: "S = 3", 9: "S = 4", 20: "S = 5"}
DROPS = {K: K != 6 for K in LAST_UNIT}


def _pair(spec, **kw):
    a = Solver(spec, backend="hip", device=0, **kw)
    b = Solver(spec, backend="hip", device=0, keep_prev=True, **kw)
    return a, b


def _log(r):
    return (list(r.steps), list(r.max_err), list(r.rms_err))


def _same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.shape == y.shape and bool((x.view(np.int64) == y.view(np.int64)).all())


@pytest.mark.parametrize("N", [63, 40])
@pytest.mark.parametrize("K", sorted(LAST_UNIT))
def test_prev_level_is_rebuilt_bit_for_bit(gpu, N, K):
    spec = ProblemSpec(N=N, tau=1e-3, K=K)
    a, b = _pair(spec)
    ra, rb = a.run(), b.run()
    assert a.native.mode == b.native.mode == "fused-single"
    assert a.native.stored_prev == (not DROPS[K]), LAST_UNIT[K]
    assert b.native.stored_prev is True
    assert _log(ra) == _log(rb)
    assert a.traffic() == b.traffic()
    # u^K first (it must not need u^{K-1}), then u^{K-1} through download(1)
    assert _same(a.native.download(0), b.native.download(0))
    assert _same(a.native.download(1), b.native.download(1))
    assert _same(a.native.download(0), b.native.download(0))  # (the rebuild wrote u^K over itself)
    assert a.native.field_hash(1) == b.native.field_hash(1)
    assert a.native.stored_prev == (not DROPS[K])  # (a fact of the schedule, not of the rebuild)
    # a fresh solve drops it again: field_hash(1) is then the accessor that rebuilds it
    assert _log(a.run()) == _log(rb)
    assert a.native.field_hash(1) == b.native.field_hash(1)
    assert a.native.field_hash(0) == b.native.field_hash(0)
    # run_batch: every solve of it in full, then u^{K-1}
    la, lb = a.run_batch(3), b.run_batch(3)
    assert [_log(r) for r in la] == [_log(r) for r in lb] == [_log(rb)] * 3
    assert _same(a.native.download(1), b.native.download(1))
    # the rebuild disturbed nothing the next solve needs: same log, same fields
    assert _log(a.run()) == _log(rb)
    assert _same(a.native.download(0), b.native.download(0))
    assert _same(a.native.download(1), b.native.download(1))


@pytest.mark.parametrize("N", [63, 40])
@pytest.mark.parametrize("K", [5, 9, 20])
def test_energy_after_set_initial(gpu, N, K):
    """energy(0) reads u^{K-1}: it is the first accessor after the solve here."""
    spec = ProblemSpec(N=N, tau=1e-3, K=K)
    rng = np.random.default_rng(N * 100 + K)
    phi, psi = rng.standard_normal((N + 1,) * 3), rng.standard_normal((N + 1,) * 3)
    a, b = _pair(spec)
    a.set_initial(phi, psi)
    b.set_initial(phi, psi)
    assert _log(a.run()) == _log(b.run())
    # (a start from u⁰, u¹ has no analytic pass: K − 1 steps of passes follow, and only a fused last one drops)
    assert b.native.stored_prev is True
    dropped = not a.native.stored_prev
    assert a.native.energy(0) == b.native.energy(0)
    assert a.native.energy_sums(0) == b.native.energy_sums(0)
    assert a.native.energy(1) == b.native.energy(1)
    assert _same(a.native.download(1), b.native.download(1))
    assert _log(a.run()) == _log(b.run())
    assert a.native.energy_sums(0) == b.native.energy_sums(0)
    assert dropped == (not a.native.stored_prev)


@pytest.mark.parametrize("N", [63, 40])
@pytest.mark.parametrize("n0", [3, 11])
def test_resume_at_an_odd_step(gpu, N, n0):
    spec = ProblemSpec(N=N, tau=1e-3, K=20)
    rng = np.random.default_rng(N + n0)
    prev, cur = rng.standard_normal((N + 1,) * 3), rng.standard_normal((N + 1,) * 3)
    for f in (prev, cur):  # (Dirichlet faces)
        f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = 0, 0, 0, 0, 0, 0
    a, b = _pair(spec)
    a.set_state(prev, cur, n0)
    b.set_state(prev, cur, n0)
    assert _log(a.run()) == _log(b.run())
    assert _same(a.native.download(1), b.native.download(1))
    assert _same(a.native.download(0), b.native.download(0))
    assert a.native.field_hash(1) == b.native.field_hash(1)


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("N,world,decomp", [(63, 2, "slab"), (40, 4, "2x1x2")])
def test_groups_every_rank(gpu, N, world, decomp, overlap):
    spec = ProblemSpec(N=N, tau=1e-3, K=20)
    a, b = _pair(spec, transport="loopback", world=world, rank=0, decomp=decomp, overlap=overlap)
    ra, rb = a.run(), b.run()
    assert a.native.mode() == b.native.mode() == ("deep-tb" if decomp == "slab" else "deep-tb-block")
    assert _log(ra) == _log(rb)
    drops = [not a.native.stored_prev(r) for r in range(world)]
    assert all(b.native.stored_prev(r) for r in range(world))
    assert len(set(drops)) == 1, "the ranks of a world decide alike"
    if decomp == "slab":
        assert drops[0], "slab ranks run their last unit on the pair-tiled pass"
    for r in range(world):
        assert _same(a.native.download(r, 0), b.native.download(r, 0))
        assert _same(a.native.download(r, 1), b.native.download(r, 1))
    # the second run is the captured group graph's first replay, the third a replay after a rebuild
    for _ in range(2):
        assert _log(a.run()) == _log(rb)
        assert a.field_hash(1) == b.field_hash(1)
        for r in range(world):
            assert _same(a.native.download(r, 1), b.native.download(r, 1))
            assert _same(a.native.download(r, 0), b.native.download(r, 0))


@pytest.mark.parametrize("K", sorted(LAST_UNIT))
def test_cli_json_reports_stored_prev(gpu, tmp_path, K):
    """The CLI's --json: stored_prev false exactly where the last unit drops the level, true with --keep-prev; the
    same error log either way; traffic counts the schedule's levels, a dropped one included."""
    out = {}
    for tag, extra in (("drop", []), ("keep", ["--keep-prev"])):
        js = tmp_path / f"{tag}.json"
        subprocess.run([os.path.join(ROOT, "bin", "wave3d"), "40", "0.001", str(K), "1", "--json", str(js), "--quiet",
                        *extra], check=True, timeout=120, capture_output=True)
        out[tag] = json.loads(js.read_text())
    assert out["drop"]["mode"] == out["keep"]["mode"] == "fused-single"
    assert out["drop"]["stored_prev"] is (not DROPS[K])
    assert out["keep"]["stored_prev"] is True
    assert out["drop"]["steps"] == out["keep"]["steps"]
    assert out["drop"]["field_bytes"] == out["keep"]["field_bytes"]
