"""Field dump format (the reference defines none, so this is the framework's own, documented here).

A dump of u at step n is ``<prefix>.bin`` + ``<prefix>.json`` for one rank, or ``<prefix>.rank<r>.bin/.json`` per rank
of a decomposed run:

* ``.bin``  raw little-endian float64, C order [x][y][z], the rank's OWNED nodes only (shape = json "shape");
* ``.json`` {"format": "wave3d-dump-v1", "dtype": "float64", "order": "C", "N", "L", "tau", "step", "t", "shape",
  "offset" (global index of the first node), "global_shape" [(N+1)]*3, "rank", "world", "dims"}; a rectangular box
  adds "box": [Lx, Ly, Lz] ("L" is Lx). The key is absent for cubes, so dumps written before boxes existed still load.

A single-rank dump is the whole (N+1)³ field: ``numpy.fromfile(p + ".bin").reshape(N+1, N+1, N+1)``.
``load()`` assembles either kind; ``save()`` writes the same format from Python (used for checkpoints).
"""
from __future__ import annotations

import glob
import json
import os

import numpy as np

FORMAT = "wave3d-dump-v1"


def save(prefix: str, field: np.ndarray, *, N: int, L: float, tau: float, step: int, offset=(0, 0, 0), rank: int = 0,
         world: int = 1, dims=(1, 1, 1), extra: dict | None = None, box=None) -> None:
    field = np.ascontiguousarray(field, dtype="<f8")
    base = prefix if world == 1 else f"{prefix}.rank{rank}"
    field.tofile(base + ".bin")
    meta = {"format": FORMAT, "dtype": "float64", "order": "C", "N": int(N), "L": float(L), "tau": float(tau),
            "step": int(step), "t": float(step * tau), "shape": list(field.shape), "offset": [int(o) for o in offset],
            "global_shape": [N + 1] * 3, "rank": int(rank), "world": int(world), "dims": [int(d) for d in dims]}
    if box is not None and not (box[0] == box[1] == box[2]):  # (absent for cubes, as in every earlier dump)
        meta["box"] = [float(e) for e in box]
    if extra:
        meta.update(extra)
    with open(base + ".json", "w") as f:
        json.dump(meta, f)


def read_meta(prefix: str) -> list[dict]:
    if os.path.exists(prefix + ".json"):
        paths = [prefix + ".json"]
    else:
        paths = sorted(glob.glob(prefix + ".rank*.json"), key=lambda p: int(p.rsplit(".rank", 1)[1][:-5]))
    if not paths:
        raise FileNotFoundError(f"no dump at {prefix}(.rank*).json")
    metas = []
    for p in paths:
        with open(p) as f:
            m = json.load(f)
        if m.get("format") != FORMAT:
            raise ValueError(f"{p}: not a {FORMAT} dump")
        m["_bin"] = p[:-5] + ".bin"
        metas.append(m)
    return metas


def box_of(meta: dict) -> tuple[float, float, float]:
    """(Lx, Ly, Lz) of a dump's sidecar: its "box", or the cube of edge "L"."""
    b = meta.get("box")
    return tuple(float(e) for e in b) if b else (float(meta["L"]),) * 3


TRACES_FORMAT = "wave3d-traces-v1"


def save_traces(prefix: str, traces: np.ndarray, nodes, *, N: int, K: int, L: float, tau: float, box=None,
                extra: dict | None = None) -> None:
    """Receiver traces (``Solver.traces()``, ``--traces``): ``<prefix>.bin`` raw little-endian float64, C order
    [K+1][R], row n = u^n at the R nodes; ``<prefix>.json`` {"format": "wave3d-traces-v1", "dtype", "order", "N", "K",
    "L" [, "box"], "tau", "shape": [K+1, R], "nodes": [[i, j, k], ...]}. The native CLI writes the same files."""
    traces = np.ascontiguousarray(traces, dtype="<f8")
    nodes = [[int(v) for v in n] for n in nodes]
    if traces.shape != (K + 1, len(nodes)):
        raise ValueError(f"traces of shape {traces.shape} for K = {K} and {len(nodes)} nodes")
    traces.tofile(prefix + ".bin")
    meta = {"format": TRACES_FORMAT, "dtype": "float64", "order": "C", "N": int(N), "K": int(K), "L": float(L),
            "tau": float(tau), "shape": list(traces.shape), "nodes": nodes}
    if box is not None and not (box[0] == box[1] == box[2]):
        meta["box"] = [float(e) for e in box]
    if extra:  # (keys a solve adds only when set, e.g. "space_order": 4)
        meta.update(extra)
    with open(prefix + ".json", "w") as f:
        json.dump(meta, f)


def load_traces(prefix: str) -> tuple[np.ndarray, dict]:
    """(traces (K+1, R), sidecar) of a ``--traces`` / ``save_traces`` output; meta["nodes"] lists the R nodes."""
    with open(prefix + ".json") as f:
        m = json.load(f)
    if m.get("format") != TRACES_FORMAT:
        raise ValueError(f"{prefix}.json: not a {TRACES_FORMAT} file")
    shape = m["shape"]
    a = np.fromfile(prefix + ".bin", dtype="<f8")
    if len(shape) != 2 or a.size != shape[0] * shape[1] or shape[0] != m["K"] + 1 or shape[1] != len(m["nodes"]):
        raise ValueError(f"{prefix}.bin: size {a.size} does not match shape {shape}, K and the node list")
    return a.reshape(shape), m


def load_receivers(path: str) -> np.ndarray:
    """(R, 3) int64 node indices of a ``--receivers`` file: one ``i j k`` per line, blank and # lines skipped."""
    rows = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            if len(t) != 3:
                raise ValueError(f"receivers: {path} line {no}: expected three integers i j k")
            rows.append([int(v) for v in t])
    if not rows:
        raise ValueError(f"receivers: {path} lists no node")
    return np.array(rows, dtype=np.int64)


def load(prefix: str) -> tuple[np.ndarray, dict]:
    """Assemble the global field from a single- or multi-rank dump. Returns (array (N+1)³, metadata of rank 0)."""
    metas = read_meta(prefix)
    g = metas[0]["global_shape"]
    out = np.zeros(g, dtype=np.float64)
    covered = 0
    for m in metas:
        a = np.fromfile(m["_bin"], dtype="<f8")
        shape = m["shape"]
        if a.size != int(np.prod(shape)):
            raise ValueError(f"{m['_bin']}: size {a.size} does not match shape {shape}")
        a = a.reshape(shape)
        x, y, z = m["offset"]
        out[x:x + shape[0], y:y + shape[1], z:z + shape[2]] = a
        covered += a.size
    if covered != out.size:
        raise ValueError(f"dump covers {covered} of {out.size} nodes (missing ranks?)")
    return out, metas[0]
