"""Shared by the point-source tests: the N = 40, K = 12 configurations (cube and box) with their source list, seeded
initial data and wavelet — the same numbers csrc/tests/test_sources.cpp builds, so the d_split / umax it prints for
"cube" and "box" belong to exactly these solves — and the CPU-solver references (computed once and shared)."""
import functools

import numpy as np

from mpi_cuda_amd import ProblemSpec

N40, K40, TAU40 = 40, 12, 0.005
BOX = (1.0, 1.3, 0.7)
# centre; (1,1,1), clipped by three faces; next to the upper x face; balls straddling the 32 x 32 tile edge (y = 31/32,
# x / z = 31/32); L1 distance 2 from the centre (a second colour class); the centre again (a third); one node from the
# 4-slab rank faces (slabs start at x = 10, 20, 30) and on the 2x2x2 rank corner (blocks start at 20)
SOURCES_40 = np.array([[20, 20, 20], [1, 1, 1], [39, 17, 22], [31, 32, 9], [32, 10, 31], [20, 21, 21], [20, 20, 20],
                       [10, 20, 20], [11, 5, 5]], dtype=np.int64)
# printed by the native program (csrc/tests/test_sources.cpp check_split "cube" / "box"; tests/test_sources_native.py
# compares them with its output): the rounding of the split identity on the CPU, 5 + 5 + 1 steps, and max |u|
D_SPLIT = {False: 4.4408920985006262e-15, True: 1.7763568394002505e-15}
UMAX = {False: 8.0939824767347339, True: 7.3247939685867181}
EPS = 2.0 ** -52


def tolerance(box):
    """Fused GPU solve against CpuSolver: max(8 d_split, 16 eps umax) — a rounding difference between two evaluation
    orders; the factor 8 covers the GPU's pass boundaries against the CPU program's 5 + 5 + 1 split."""
    return max(8.0 * D_SPLIT[box], 16.0 * EPS * UMAX[box])


def spec40(box, K=K40, check_every=2):
    return ProblemSpec(N=N40, tau=TAU40, K=K, L=BOX[0], check_every=check_every, Ly=BOX[1] if box else None,
                       Lz=BOX[2] if box else None)


def wavelet(K, Q):
    """(K, Q) exact dyadic samples: w[m][q] = ((7 m + 3 q) mod 11 - 5) / 4."""
    m, q = np.meshgrid(np.arange(K), np.arange(Q), indexing="ij")
    return np.ascontiguousarray(((m * 7 + q * 3) % 11 - 5) / 4.0)


@functools.lru_cache(maxsize=None)
def lcg_fields(N):
    """phi, psi on the global (N+1)^3 grid, values in [-1, 1) from the 64-bit LCG of the native program (phi first)."""
    n3 = (N + 1) ** 3
    out = np.empty(2 * n3)
    s, mask = 0x9E3779B97F4A7C15, (1 << 64) - 1
    for i in range(2 * n3):
        s = (s * 6364136223846793005 + 1442695040888963407) & mask
        out[i] = (s >> 11) / 9007199254740992.0 * 2.0 - 1.0
    return out[:n3].reshape((N + 1,) * 3).copy(), out[n3:].reshape((N + 1,) * 3).copy()


def receivers_around(sources, N):
    """Up to 6 receivers around each source — the node itself, its x+ neighbour, and nodes at L1 distance 2, 3, 4 and 5 —
    clipped to the grid 0..N (a clipped one may land on a face)."""
    offs = [(0, 0, 0), (1, 0, 0), (-1, 1, 0), (1, -1, 1), (0, 2, -2), (-2, 1, 2)]
    v = [np.clip(np.asarray(s) + np.asarray(o), 0, N) for s in sources for o in offs]
    return np.array(v, dtype=np.int64)


def same_bits(a, b):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@functools.lru_cache(maxsize=None)
def cpu_reference(box):
    """CpuSolver with SOURCES_40, the seeded data and the receivers around the sources: (u^K, u^{K-1}, traces)."""
    from mpi_cuda_amd.solver import Solver

    s = Solver(spec40(box), backend="cpu")
    s.set_initial(*lcg_fields(N40))
    s.set_sources(SOURCES_40, wavelet(K40, len(SOURCES_40)))
    s.set_receivers(receivers_around(SOURCES_40, N40))
    s.run()
    return s.global_field(0).numpy().copy(), s.global_field(1).numpy().copy(), s.traces().numpy().copy()
