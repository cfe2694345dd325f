"""Shared by the receiver tests: the common receiver set for a grid and a decomposition, random initial data, and the
CPU-solver reference traces (computed once per case and shared)."""
import functools

import numpy as np

from mpi_cuda_amd import ProblemSpec
from mpi_cuda_amd._native import load


def spec_for(N, K, check_every=2):
    s = ProblemSpec(N=N, tau=1.0, K=K, L=1.0, check_every=check_every)
    return ProblemSpec(N=N, tau=0.5 * s.tau_max, K=K, L=1.0, check_every=check_every)


def receiver_set(N, dims=(1, 1, 1)):
    """(R, 3) int64 global nodes: per axis the nodes 0, 1, N - 1, N with mid-range values on the other axes; the first
    and last owned node of every rank along every split axis (both sides of every rank face); the eight corners of
    every rank box of a block decomposition; one node listed twice; 48 seeded random nodes."""
    C = load()
    mid = [N // 2, N // 3, (2 * N) // 3]
    v = []
    for a in range(3):
        for e in (0, 1, N - 1, N):
            n = list(mid)
            n[a] = e
            v.append(n)
    for a in range(3):
        if dims[a] > 1:
            for c in range(dims[a]):
                b, e = C.split_axis(N, dims[a], c)
                for x in (b, e - 1):
                    n = list(mid)
                    n[a] = x
                    v.append(n)
    if dims[1] > 1 or dims[2] > 1:
        prob = C.Problem(N, 1e-4, 2, 1.0)
        D = C.Dims(*dims)
        for r in range(dims[0] * dims[1] * dims[2]):
            b = C.rank_box(prob, D, r)
            for x in (b.x0, b.x1 - 1):
                for y in (b.y0, b.y1 - 1):
                    for z in (b.z0, b.z1 - 1):
                        v.append([x, y, z])
    v.append(list(v[5]))
    rng = np.random.default_rng(1000 + N)
    v += rng.integers(0, N + 1, size=(48, 3)).tolist()
    return np.array(v, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def initial_data(N):
    """Random phi, psi on the global (N+1)^3 grid (face values included: they must be ignored)."""
    rng = np.random.default_rng(77 + N)
    return rng.standard_normal((N + 1,) * 3), rng.standard_normal((N + 1,) * 3)


def at_nodes(field, nodes):
    f = np.asarray(field)
    return f[nodes[:, 0], nodes[:, 1], nodes[:, 2]]


def same_bits(a, b):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@functools.lru_cache(maxsize=None)
def cpu_traces(N, K, dims=(1, 1, 1), start="initial"):
    """CpuSolver traces (the oracle) of the common set: start = "initial" (random phi, psi), "default" (eigenmode) or
    "state4" (set_state at n0 = 4 from the K = 4 fields of the random-data solve). Returns (nodes, traces (K+1, R))."""
    from mpi_cuda_amd.solver import Solver

    nodes = receiver_set(N, dims)
    s = Solver(spec_for(N, K), backend="cpu")
    if start == "initial":
        s.set_initial(*initial_data(N))
    elif start == "state4":
        s.set_state(*state_at(N, 4), 4)
    s.set_receivers(nodes)
    s.run()
    return nodes, s.traces().numpy().copy()


@functools.lru_cache(maxsize=None)
def cpu_fields(N, n):
    """(u^{n-1}, u^n) global fields of a K = n CPU solve from the random data WITHOUT receivers: the cross-check that is
    independent of the record code."""
    from mpi_cuda_amd.solver import Solver

    s = Solver(spec_for(N, n), backend="cpu")
    if n > 1:
        s.set_initial(*initial_data(N))
        s.run()
        return s.global_field(1).numpy().copy(), s.global_field(0).numpy().copy()
    raise ValueError("n >= 2")


def state_at(N, n0):
    prev, cur = cpu_fields(N, n0)
    return prev, cur
