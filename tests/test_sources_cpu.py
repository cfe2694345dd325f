"""Point sources on the CPU backend: the Python API (Solver.set_sources), its defining properties — a zero wavelet changes
no bit, linearity in the amplitude, causality at receivers — every refusal, the --sources file and the CLI round trip."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sources_common import lcg_fields, same_bits, wavelet

from mpi_cuda_amd import ProblemSpec
from mpi_cuda_amd.solver import Solver
from mpi_cuda_amd.utils import dump as dumpio
from mpi_cuda_amd.utils.wavelets import load_sources, ricker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "bin", "wave3d")
N, K, TAU = 24, 12, 0.008
NODES = np.array([[12, 11, 13], [1, 1, 1], [23, 8, 20], [12, 11, 13]], dtype=np.int64)


@pytest.fixture(scope="module", autouse=True)
def cli_built():
    if not os.path.exists(CLI):
        from mpi_cuda_amd._native import load

        load()
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build.py")], check=True)
    assert os.path.exists(CLI)


def _spec(K=K, box=False):
    return ProblemSpec(N=N, tau=TAU, K=K, L=1.0, check_every=2, Ly=1.3 if box else None, Lz=0.7 if box else None)


def _solve(w=None, nodes=NODES, initial=True, receivers=None, box=False, zero=False):
    s = Solver(_spec(box=box), backend="cpu")
    if zero:
        s.set_initial(np.zeros((N + 1,) * 3), np.zeros((N + 1,) * 3))
    elif initial:
        s.set_initial(*lcg_fields(N))
    if w is not None:
        s.set_sources(nodes, w)
        assert s.sources == len(nodes) and s.native.sources == len(nodes)
    if receivers is not None:
        s.set_receivers(receivers)
    s.run()
    return s


def test_definition_against_numpy():
    """K = 2 from a zero field: u^1 = a^0/2 at the node, u^2 = 2 u^1 + lam d2sum(u^1) + a^1 by hand."""
    from mpi_cuda_amd._native import load

    C = load()
    spec = ProblemSpec(N=N, tau=TAU, K=2, L=1.0)
    s = Solver(spec, backend="cpu")
    s.set_initial(np.zeros((N + 1,) * 3))
    node = np.array([[5, 6, 7]])
    w = np.array([[1.5], [-0.75]])
    s.set_sources(node, w)
    s.run()
    h = 1.0 / N
    a = [C.source_addend(spec.native(), float(v)) for v in w[:, 0]]
    assert a[0] == (TAU * TAU * 1.5) / ((h * h) * h)
    u1, u2 = s.global_field(1).numpy(), s.global_field(0).numpy()
    want1 = np.zeros_like(u1)
    want1[5, 6, 7] = 0.5 * a[0]
    assert same_bits(u1, want1)
    lam = (TAU * TAU) * (1.0 / (h * h))
    assert u2[5, 6, 7] == pytest.approx(2 * want1[5, 6, 7] - 6 * lam * want1[5, 6, 7] + a[1], rel=1e-14)
    assert u2[4, 6, 7] == pytest.approx(lam * want1[5, 6, 7], rel=1e-14) and u2[4, 5, 7] == 0.0


def test_zero_wavelet_changes_no_bit():
    plain = _solve()
    zero = _solve(np.zeros((K, len(NODES))))
    for which in (0, 1):
        assert same_bits(zero.global_field(which).numpy(), plain.global_field(which).numpy())
    # removing the sources restores the plain solve as well
    s = Solver(_spec(), backend="cpu")
    s.set_initial(*lcg_fields(N))
    s.set_sources(NODES, wavelet(K, len(NODES)))
    s.run()
    assert not same_bits(s.global_field(0).numpy(), plain.global_field(0).numpy())
    s.set_sources(np.zeros((0, 3), dtype=np.int64), np.zeros((K, 0)))
    assert s.sources == 0
    s.run()
    assert same_bits(s.global_field(0).numpy(), plain.global_field(0).numpy())


@pytest.mark.parametrize("box", [False, True])
def test_linear_in_amplitude(box):
    """Zero initial data: doubling w doubles every value exactly (a power-of-two scale commutes with every rounding)."""
    w = wavelet(K, len(NODES))
    one = _solve(w, zero=True, box=box)
    two = _solve(2.0 * w, zero=True, box=box)
    f1 = one.global_field(0).numpy()
    assert np.abs(f1).max() > 0
    assert same_bits(two.global_field(0).numpy(), 2.0 * f1)
    assert same_bits(two.global_field(1).numpy(), 2.0 * one.global_field(1).numpy())
    # a node listed twice (slots 0 and 3) is added twice: the same as one source with the summed samples
    merged = _solve((w[:, [0, 1, 2]] + np.c_[w[:, 3], 0 * w[:, 1], 0 * w[:, 2]]), nodes=NODES[:3], zero=True, box=box)
    assert np.allclose(merged.global_field(0).numpy(), f1, rtol=0, atol=1e-12 * np.abs(f1).max())


def test_causality_at_receivers():
    """A receiver at L1 distance d from the only source stays exactly 0.0 up to row d and moves at row d + 1."""
    src = np.array([[12, 11, 13]])
    w = np.ones((K, 1))
    offs = [(0, 0, 0), (1, 0, 0), (0, -1, 1), (1, 1, 1), (-2, 0, 2), (3, -1, 1), (0, 0, 6)]
    rec = src + np.array(offs)
    s = _solve(w, nodes=src, zero=True, receivers=rec)
    tr = s.traces().numpy()
    for r, o in enumerate(offs):
        d = sum(abs(v) for v in o)
        assert same_bits(tr[:d + 1, r], np.zeros(d + 1)), (o, tr[:, r])
        assert tr[d + 1, r] != 0.0, (o, tr[:, r])
    assert same_bits(tr[K], s.global_field(0).numpy()[rec[:, 0], rec[:, 1], rec[:, 2]])


def test_refusals():
    s = Solver(_spec(), backend="cpu")
    w = np.zeros((K, 1))
    for bad in ([[0, 5, 5]], [[5, N, 5]], [[5, 5, N + 3]], [[-1, 5, 5]]):
        with pytest.raises(ValueError, match="sources:.*not strictly inside the grid"):
            s.set_sources(bad, w)
        with pytest.raises(RuntimeError, match="sources:.*not strictly inside the grid"):
            s.native.set_sources(np.array(bad, dtype=np.int64), w)
    with pytest.raises(ValueError, match=r"sources: w must have shape \(K, Q\)"):
        s.set_sources([[5, 5, 5]], np.zeros((K - 1, 1)))
    with pytest.raises(ValueError, match=r"sources: w must have shape \(K, Q\)"):
        s.set_sources([[5, 5, 5]], np.zeros((K, 2)))
    with pytest.raises(RuntimeError, match=r"sources: w must have shape \(K, Q\)"):
        s.native.set_sources(np.array([[5, 5, 5]], dtype=np.int64), np.zeros((K + 1, 1)))
    with pytest.raises(ValueError, match="sources:.*Q, 3"):
        s.set_sources(np.zeros((4, 2), dtype=np.int64), np.zeros((K, 4)))
    for v in (np.nan, np.inf):
        wb = np.zeros((K, 1))
        wb[3, 0] = v
        with pytest.raises(ValueError, match="sources:.*non-finite"):
            s.set_sources([[5, 5, 5]], wb)
        with pytest.raises(RuntimeError, match="sources:.*not finite"):
            s.native.set_sources(np.array([[5, 5, 5]], dtype=np.int64), wb)
    assert s.sources == 0
    # not together with a resumed start, in either order
    s.set_sources([[5, 5, 5]], w)
    f = np.zeros((N + 1,) * 3)
    with pytest.raises(RuntimeError, match="sources: not together with set_state"):
        s.set_state(f, f, 4)
    t = Solver(_spec(), backend="cpu")
    t.set_state(f, f, 4)
    with pytest.raises(RuntimeError, match="sources: not together with set_state"):
        t.set_sources([[5, 5, 5]], w)


def test_ricker_and_sources_file(tmp_path):
    f0, t0 = 25.0, 0.04
    w = ricker(f0, t0, TAU, K, amp=3.0)
    t = np.arange(K) * TAU - t0
    assert w.shape == (K,) and np.allclose(w, 3.0 * (1 - 2 * (np.pi * f0 * t) ** 2) * np.exp(-(np.pi * f0 * t) ** 2), rtol=1e-15)
    assert ricker(f0, 5 * TAU, TAU, K)[5] == 1.0  # the peak
    p = tmp_path / "src.txt"
    p.write_text("# i j k f0 t0 amp\n\n12 11 13 25 0.04 3\n  1 1 1 10.5 0.0 -2e0\n")
    nodes, ws = load_sources(str(p), TAU, K)
    assert nodes.tolist() == [[12, 11, 13], [1, 1, 1]] and ws.shape == (K, 2)
    assert same_bits(ws[:, 0], w) and same_bits(ws[:, 1], ricker(10.5, 0.0, TAU, K, -2.0))
    for text in ("1 2 3 4 5\n", "1 2 3 4 5 6 7\n", "a b c 1 2 3\n", "# nothing\n"):
        p.write_text(text)
        with pytest.raises(ValueError, match="sources:"):
            load_sources(str(p), TAU, K)


def test_cli_round_trip(tmp_path):
    """--sources with --receivers / --traces, --initial and --json on both CLIs: python -m mpi_cuda_amd reproduces the API
    bit for bit; bin/wave3d --cpu samples the wavelet with its own exp, so its traces agree to rounding."""
    sf, rf = tmp_path / "src.txt", tmp_path / "rec.txt"
    sf.write_text("# shots\n12 11 13 25 0.04 3\n5 6 7 40 0.02 -1.5\n")
    rec = np.array([[12, 11, 13], [13, 11, 13], [5, 6, 9], [20, 20, 20]])
    rf.write_text("".join(f"{i} {j} {k}\n" for i, j, k in rec.tolist()))
    phi, psi = lcg_fields(N)
    dumpio.save(str(tmp_path / "ini.phi"), phi, N=N, L=1.0, tau=TAU, step=0)
    dumpio.save(str(tmp_path / "ini.psi"), psi, N=N, L=1.0, tau=TAU, step=0)
    nodes, w = load_sources(str(sf), TAU, K)
    api = _solve(w, nodes=nodes, receivers=rec)
    want = api.traces().numpy()
    plain = _solve(receivers=rec).traces().numpy()
    assert np.abs(want - plain).max() > 1e-3  # the shots are in the seismograms
    out = {}
    for name, cmd in (("py", [sys.executable, "-m", "mpi_cuda_amd", str(N), repr(TAU), str(K), "--backend", "cpu"]),
                      ("native", [CLI, str(N), repr(TAU), str(K), "--cpu", "--threads", "2"])):
        o, j = tmp_path / f"tr_{name}", tmp_path / f"{name}.json"
        r = subprocess.run(cmd + ["--sources", str(sf), "--receivers", str(rf), "--traces", str(o), "--initial",
                                  str(tmp_path / "ini"), "--json", str(j), "--quiet"], capture_output=True, text=True,
                           timeout=120, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = dumpio.load_traces(str(o))[0]
        assert json.loads(j.read_text())["sources"] == 2
    assert same_bits(out["py"], want)
    assert np.allclose(out["native"], want, rtol=0, atol=1e-12 * np.abs(want).max())
    r = subprocess.run([CLI, str(N), repr(TAU), str(K), "--cpu", "--sources", str(sf), "--resume", "x"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--sources and --resume exclude each other" in r.stderr
    sf.write_text("0 11 13 25 0.04 3\n")
    r = subprocess.run([CLI, str(N), repr(TAU), str(K), "--cpu", "--sources", str(sf)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "sources:" in r.stderr and "not strictly inside" in r.stderr
