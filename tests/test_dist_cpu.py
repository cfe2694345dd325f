"""Multi-process decomposition on the CPU over torch.distributed gloo (the reference's MPI / MPI+OpenMP programs,
report.pdf p.9-11): every decomposition and rank count reproduces the single-process field bit-for-bit."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["ROOT"])
from mpi_cuda_amd import ProblemSpec
from mpi_cuda_amd.solver import Solver
dist.init_process_group("gloo")
spec = ProblemSpec(N=int(os.environ["N"]), tau=1e-3, K=int(os.environ["K"]), check_every=1)
s = Solver(spec, backend="cpu", transport="torch", decomp=os.environ["DECOMP"], threads=1)
r = s.run()
torch.save({"max": r.max_err, "rms": r.rms_err, "f": s.owned_field(0), "f1": s.owned_field(1),
            "dims": tuple(s.dims)}, os.environ["OUT"] + f".{dist.get_rank()}.pt")
dist.destroy_process_group()
"""


def _run(tmp_path, world, decomp, N, K, port):
    script = tmp_path / "w.py"
    script.write_text(_WORKER)
    env = dict(os.environ, ROOT=ROOT, OUT=str(tmp_path / "res"), DECOMP=decomp, N=str(N), K=str(K),
               OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(world), "--master-addr",
           "127.0.0.1", "--master-port", str(port), str(script)]
    subprocess.run(cmd, env=env, check=True, timeout=300, capture_output=True)
    return [torch.load(str(tmp_path / f"res.{r}.pt"), weights_only=True) for r in range(world)]


@pytest.mark.parametrize("world,decomp", [(2, "slab"), (4, "block"), (3, "1x3x1"), (4, "1x1x4")])
def test_decomposed_cpu_bitexact(tmp_path, world, decomp):
    from mpi_cuda_amd import ProblemSpec
    from mpi_cuda_amd.parallel.decomp import plan
    from mpi_cuda_amd.solver import Solver

    N, K = 30, 6
    port = 29400 + world * 10 + len(decomp) + (os.getpid() % 50)
    res = _run(tmp_path, world, decomp, N, K, port)
    spec = ProblemSpec(N=N, tau=1e-3, K=K, check_every=1)
    ref = Solver(spec, backend="cpu")
    rr = ref.run()
    full0, full1 = ref.owned_field(0), ref.owned_field(1)
    for rank, d in enumerate(res):
        assert d["max"] == rr.max_err
        assert all(abs(a - b) <= 1e-12 * b for a, b in zip(d["rms"], rr.rms_err))
        x0, x1, y0, y1, z0, z1 = plan(N, world, rank, decomp).box
        assert torch.equal(d["f"], full0[x0:x1, y0:y1, z0:z1])
        assert torch.equal(d["f1"], full1[x0:x1, y0:y1, z0:z1])


def test_bench_contract_cpu_two_ranks(tmp_path):
    """bench.py under torch.distributed.run prints exactly one JSON line with the contract keys. --cpu drives the same
    orchestration as on GPUs (per-launch nonce, one native bin/wave3d child per rank, agreement on success) with the
    native CPU ranks as children."""
    import json

    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(29380 + os.getpid() % 50), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--cpu",
           "--N", "24", "--steps", "2", "--warmup", "1"]
    out = subprocess.run(cmd, check=True, timeout=300, capture_output=True, text=True).stdout
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "ms_per_solve", "degraded", "process_wall_s"):
        assert k in d
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["correct"]
    assert d["degraded"] is False and d["ms_per_step"] == d["ms_per_solve"] > 0
    for k in ("model", "global_batch", "seq_len", "parallelism"):
        assert k in d["config"]
    assert d["config"]["schedule"] == "cpu-openmp-ranks" and d["config"]["decomp"] == "2x1x1"
    assert d["config"]["runtime"].startswith("native")


def test_bench_python_path_cpu_labels_step_loop(tmp_path):
    """--python on CPU ranks runs the in-process torch transport: the Python single-step loop, labelled as such."""
    import json

    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(29430 + os.getpid() % 50), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--cpu",
           "--python", "--N", "24", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "dump")]
    out = subprocess.run(cmd, check=True, timeout=300, capture_output=True, text=True).stdout
    d = json.loads([l for l in out.splitlines() if l.startswith("{")][0])
    assert d["config"]["schedule"] == "python-step-loop-S1" and d["config"]["transport"] == "torch"
    assert not d["config"]["graph"] and not d["config"]["overlap"] and not d["config"]["temporal_blocking"]
    assert d["correct"] and d["degraded"] is False
    # --dump-outputs of the in-process path: each rank's own slab of u^K, together the reference field
    import numpy as np

    from mpi_cuda_amd import ProblemSpec
    from mpi_cuda_amd.models.wave3d import torch_reference_solve

    _, uk, _ = torch_reference_solve(ProblemSpec(N=24, tau=1e-3, K=20), return_fields=True)
    parts = [np.load(tmp_path / "dump" / f"u_final.rank{r}.npy") for r in range(2)]
    assert np.array_equal(np.concatenate(parts, axis=0), uk.numpy())
    assert np.load(tmp_path / "dump" / "error_log.npy")[-1, 1] == d["final_max_err"]


def test_bench_failure_retries_once_with_the_conservative_schedule(tmp_path):
    """A rank whose native runtime fails makes every rank start ONE fresh child with the conservative schedule; the
    line then says so (VERDICT r4 next #3b) instead of the job ending without a scaling point."""
    import json

    env = dict(os.environ, W3D_BENCH_FAIL_SETUP_RANK="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(29380 + os.getpid() % 50), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--cpu",
           "--N", "24", "--steps", "2", "--warmup", "1"]
    p = subprocess.run(cmd, env=env, timeout=120, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert d["fallback_schedule"].startswith("slab-S4-seq")
    assert "injected fault" in d["first_failure"]
    assert d["correct"] is True


def test_bench_setup_failure_on_one_rank_exits_instead_of_hanging(tmp_path):
    """When the conservative retry fails too, every rank stops with a non-zero exit and no JSON line."""
    env = dict(os.environ, W3D_BENCH_FAIL_SETUP_RANK="1", W3D_BENCH_FAIL_FALLBACK="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(29330 + os.getpid() % 50), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--cpu",
           "--N", "24", "--steps", "2", "--warmup", "1"]
    p = subprocess.run(cmd, env=env, timeout=120, capture_output=True, text=True)
    assert p.returncode != 0
    assert "injected fault" in p.stderr
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]


def _bench_args(**kw):
    import argparse

    d = dict(N=512, tau=1e-3, K=20, L=1.0)
    d.update(kw)
    return argparse.Namespace(**d)


def test_bench_correct_gate_uses_the_oracle_for_every_config():
    """bench.py's correctness gate: every config, the 2048³ scale point included, is checked step by
    step against the closed-form oracle of the discrete scheme; a log off by 0.1 % (or non-finite) fails."""
    sys.path.insert(0, ROOT)
    import bench
    from mpi_cuda_amd import ProblemSpec
    from mpi_cuda_amd.models.wave3d import oracle_errors

    for N, tau, K, L in [(512, 1e-3, 20, 1.0), (2048, 2.5e-4, 20, 1.0), (128, 1e-3, 20, 3.141592653589793),
                         (96, 1e-3, 11, 1.0)]:
        a = _bench_args(N=N, tau=tau, K=K, L=L)
        spec = ProblemSpec(N=N, tau=tau, K=K, L=L, check_every=2)
        ref = oracle_errors(spec)
        steps = [[n, float(f"{m:.10g}"), float(f"{e:.10g}")] for n, (m, e) in sorted(ref.items())]  # CLI JSON digits
        ok, why = bench._correct(a, True, steps)
        assert ok, why
        bad = [[n, m * 1.001, e] for n, m, e in steps]  # (2048³: caught at the later steps, where 0.1 % > rounding)
        assert not bench._correct(a, True, bad)[0]
        assert not bench._correct(a, False, steps)[0]
        assert not bench._correct(a, True, [])[0]
    # the reference config also pins the reference's printed digits (report.pdf p.16): the oracle alone would accept
    # a log within 1e-5 of it
    a = _bench_args()
    steps = [[n, m, e] for n, (m, e) in sorted(oracle_errors(ProblemSpec(N=512, tau=1e-3, K=20)).items())]
    ok, _ = bench._correct(a, True, steps)
    assert ok
    # the measured 2048³ log of profiles/r2_final/cli_2048.log (one MI355X) passes
    a = _bench_args(N=2048, tau=2.5e-4)
    logged = [[2, 1.553202e-13, 5.485516e-14], [10, 3.875233e-12, 1.370967e-12], [20, 1.549894e-11, 5.483359e-12]]
    assert bench._correct(a, True, logged)[0]


def test_bench_plain_run_dumps_the_last_timed_solve(tmp_path):
    """A plain run does not trace the phases (phases_ms is null: --full does) and --dump-outputs writes what the last
    timed solve computed: the error log and u^K, here whole and bit-equal to the PyTorch reference; the ranks' raw
    dump is gone."""
    import json

    import numpy as np

    from mpi_cuda_amd import ProblemSpec
    from mpi_cuda_amd.models.wave3d import torch_reference_solve

    d = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cpu", "--N", "24", "--K", "6", "--steps",
           "2", "--warmup", "1", "--dump-outputs", str(d)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run(cmd, check=True, timeout=120, capture_output=True, text=True, env=env).stdout
    line = json.loads([l for l in out.splitlines() if l.startswith("{")][0])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["correct"] is True and line["phases_ms"] is None
    assert sorted(p.name for p in d.iterdir()) == ["error_log.npy", "u_final.npy"]
    errs, uk, _ = torch_reference_solve(ProblemSpec(N=24, tau=1e-3, K=6, check_every=2), return_fields=True)
    u = np.load(d / "u_final.npy")
    assert u.dtype == np.float64 and u.shape == (25, 25, 25) and np.array_equal(u, uk.numpy())
    log = np.load(d / "error_log.npy")
    assert log.dtype == np.float64 and log.shape == (3, 3) and list(log[:, 0]) == [2, 4, 6]
    assert line["final_max_err"] == log[-1, 1]


def test_bench_dump_gathers_the_sample_from_the_rank_files(tmp_path, monkeypatch):
    """The sampled path of --dump-outputs on a decomposed run: two native CPU ranks dump their boxes, bench.py gathers
    the fixed sample from the rank files; every value is the PyTorch reference's at that node."""
    import numpy as np

    from mpi_cuda_amd import ProblemSpec
    from mpi_cuda_amd.models.wave3d import torch_reference_solve

    sys.path.insert(0, ROOT)
    import bench

    prefix = str(tmp_path / bench.DUMP_RAW)
    subprocess.run([os.path.join(ROOT, "bin", "wave3d"), "24", "0.001", "6", "--cpu", "--np", "2", "--dump", prefix,
                    "--quiet"], check=True, timeout=120, capture_output=True)
    assert os.path.exists(prefix + ".rank1.bin")
    monkeypatch.setattr(bench, "DUMP_WHOLE_BYTES", 4096)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 3000)
    what = bench._dump_native_field(str(tmp_path), prefix)
    idx, _ = bench._dump_index(25 ** 3)
    assert 2000 < idx.size <= 3000 and what.startswith(f"{idx.size} of {25 ** 3} nodes")
    _, uk, _ = torch_reference_solve(ProblemSpec(N=24, tau=1e-3, K=6), return_fields=True)
    u = np.load(tmp_path / "u_final.npy")
    assert u.dtype == np.float64 and u.shape == idx.shape and np.array_equal(u, uk.numpy().reshape(-1)[idx])
    assert (idx // 625).min() < 12 and (idx // 625).max() > 12  # (nodes of both ranks' slabs)


def test_bench_dump_sample_is_fixed_and_bounded():
    """A field above the size limit is written at a fixed sample of its nodes: the same sorted indices in every run."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    n = 513 ** 3
    idx, what = bench._dump_index(n)
    again, _ = bench._dump_index(n)
    assert np.array_equal(idx, again) and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < n
    assert 3 << 20 < idx.size <= bench.DUMP_SAMPLE and idx.size * 8 <= 32 << 20 and str(idx.size) in what
    whole, _ = bench._dump_index(65 ** 3)
    assert np.array_equal(whole, np.arange(65 ** 3))
