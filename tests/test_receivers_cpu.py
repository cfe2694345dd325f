"""Receivers on the CPU backend: the Python API (Solver.set_receivers / traces), cross-checked through shorter solves
without receivers, and the CLI --cpu --receivers / --traces round trip through utils.dump.load_traces."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from receivers_common import (at_nodes, cpu_fields, cpu_traces, initial_data, receiver_set, same_bits, spec_for)

from mpi_cuda_amd.solver import Solver
from mpi_cuda_amd.utils import dump as dumpio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "wave3d")
N, K = 24, 12


@pytest.fixture(scope="module", autouse=True)
def cli_built():
    if not os.path.exists(CLI):
        from mpi_cuda_amd._native import load

        load()
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build.py")], check=True)
    assert os.path.exists(CLI)


def test_cpu_traces_equal_shorter_solves():
    """Row n of the traces equals u^n of a K = n solve without receivers (rows K - 1 and K: the solve's own fields);
    receivers on a face hold +0.0; the node listed twice gives two equal columns."""
    nodes, tr = cpu_traces(N, K, (2, 2, 2))
    assert tr.shape == (K + 1, len(nodes)) and not np.isnan(tr).any()
    for n in (2, 3, 7, K):
        prev, cur = cpu_fields(N, n)
        assert same_bits(tr[n], at_nodes(cur, nodes)), n
        assert same_bits(tr[n - 1], at_nodes(prev, nodes)), n
    phi = initial_data(N)[0]
    inner = ((nodes > 0) & (nodes < N)).all(axis=1)
    assert same_bits(tr[0][inner], at_nodes(phi, nodes)[inner])  # u^0 = phi inside
    assert (~inner).sum() >= 12 and same_bits(tr[:, ~inner], np.zeros((K + 1, int((~inner).sum()))))
    twin = [(a, b) for a in range(len(nodes)) for b in range(a + 1, len(nodes)) if (nodes[a] == nodes[b]).all()]
    assert twin and all(same_bits(tr[:, a], tr[:, b]) for a, b in twin)


def test_cpu_default_start_and_state():
    """The eigenmode start records u^0 = phi_analytic too, and a set_state start at n0 = 4 leaves the rows below 3 NaN
    and reproduces the uninterrupted solve's rows from 3 on."""
    nodes, full = cpu_traces(N, K, (2, 2, 2))
    _, resumed = cpu_traces(N, K, (2, 2, 2), "state4")
    assert np.isnan(resumed[:3]).all() and same_bits(resumed[3:], full[3:])
    _, dflt = cpu_traces(N, K, (2, 2, 2), "default")
    s = Solver(spec_for(N, K), backend="cpu")
    s.run()
    assert same_bits(dflt[K], at_nodes(s.global_field(0).numpy(), nodes))
    assert same_bits(dflt[K - 1], at_nodes(s.global_field(1).numpy(), nodes))


def test_api_refusals():
    s = Solver(spec_for(N, K), backend="cpu")
    with pytest.raises(ValueError):
        s.traces()
    with pytest.raises(Exception, match="outside the grid"):
        s.set_receivers([[0, N + 1, 0]])
    with pytest.raises(ValueError):
        s.set_receivers(np.zeros((4, 2), dtype=np.int64))
    s.set_receivers(receiver_set(N))
    s.set_receivers(np.zeros((0, 3), dtype=np.int64))  # removes them
    with pytest.raises(ValueError):
        s.traces()


def _write_nodes(path, nodes):
    with open(path, "w") as f:
        f.write("# i j k\n\n")
        for i, j, k in nodes.tolist():
            f.write(f"{i} {j} {k}\n")


def test_cli_cpu_round_trip(tmp_path):
    """bin/wave3d --cpu --receivers FILE --traces OUT: the files load through utils.dump.load_traces and hold the API's
    values (default eigenmode start); python -m mpi_cuda_amd writes the same."""
    nodes = receiver_set(N, (2, 2, 2))
    spec = spec_for(N, K)
    rf, out = tmp_path / "nodes.txt", tmp_path / "tr"
    _write_nodes(rf, nodes)
    r = subprocess.run([CLI, str(N), repr(spec.tau), str(K), "--cpu", "--threads", "2", "--receivers", str(rf),
                        "--traces", str(out), "--quiet"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    tr, meta = dumpio.load_traces(str(out))
    assert meta["format"] == "wave3d-traces-v1" and meta["N"] == N and meta["K"] == K and meta["tau"] == spec.tau
    assert np.array_equal(np.array(meta["nodes"]), nodes) and tr.shape == (K + 1, len(nodes))
    _, want = cpu_traces(N, K, (2, 2, 2), "default")
    assert same_bits(tr, want)
    out2 = tmp_path / "tr_py"
    r = subprocess.run([sys.executable, "-m", "mpi_cuda_amd", str(N), repr(spec.tau), str(K), "--backend", "cpu",
                        "--receivers", str(rf), "--traces", str(out2), "--quiet"], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    tr2, meta2 = dumpio.load_traces(str(out2))
    assert same_bits(tr2, want) and meta2["nodes"] == meta["nodes"]
    assert json.loads((tmp_path / "tr.json").read_text())["shape"] == [K + 1, len(nodes)]


def test_cli_np_refused(tmp_path):
    rf = tmp_path / "nodes.txt"
    _write_nodes(rf, receiver_set(N))
    r = subprocess.run([CLI, str(N), "0.001", str(K), "--cpu", "--np", "2", "--receivers", str(rf), "--traces",
                        str(tmp_path / "tr")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "one rank only" in r.stderr
    assert not (tmp_path / "tr.bin").exists()
    r = subprocess.run([CLI, str(N), "0.001", str(K), "--cpu", "--receivers", str(rf)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "go together" in r.stderr
