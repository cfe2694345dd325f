"""Source wavelets for ``Solver.set_sources`` and ``--sources``."""
from __future__ import annotations

import numpy as np


def ricker(f0: float, t0: float, tau: float, K: int, amp: float = 1.0) -> np.ndarray:
    """The K samples w(m·τ), m = 0..K−1, of a Ricker wavelet of peak frequency ``f0`` centred at ``t0``:
    w(t) = amp · (1 − 2π²f0²(t − t0)²) · exp(−π²f0²(t − t0)²). One column of ``set_sources``' (K, Q) array."""
    t = np.arange(int(K), dtype=np.float64) * float(tau) - float(t0)
    x = (np.pi * float(f0) * t) ** 2
    return (1.0 - 2.0 * x) * np.exp(-x) * float(amp)


def load_sources(path: str, tau: float, K: int) -> tuple[np.ndarray, np.ndarray]:
    """((Q, 3) int64 nodes, (K, Q) samples) of a ``--sources`` file: one ``i j k f0 t0 amp`` per line, a Ricker wavelet
    per source; blank and # lines are skipped."""
    nodes, cols = [], []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            if len(t) != 6:
                raise ValueError(f"sources: {path} line {no}: expected i j k f0 t0 amp")
            try:
                ijk = [int(v) for v in t[:3]]
                f0, t0, amp = (float(v) for v in t[3:])
            except ValueError:
                raise ValueError(f"sources: {path} line {no}: expected three integers and three numbers") from None
            nodes.append(ijk)
            cols.append(ricker(f0, t0, tau, K, amp))
    if not nodes:
        raise ValueError(f"sources: {path} lists no source")
    return np.array(nodes, dtype=np.int64), np.ascontiguousarray(np.stack(cols, axis=1))
