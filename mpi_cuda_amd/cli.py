"""Python CLI: ``python -m mpi_cuda_amd N tau K [L] [options]`` — same positional interface and output lines as the
reference programs (`wave`, `wave3dOMP`, `onlyMPI`, `mpiomp`, `mpigpu-1`; report.pdf p.15 §4.2.4, p.20-24 §5.x) and
as the native ``bin/wave3d``.

Launch several ranks with torchrun (the `mpirun -np P` analogue):

    torchrun --nproc-per-node 4 --master-addr 127.0.0.1 -m mpi_cuda_amd 512 0.001 20 1              # 4 GPUs, RCCL
    torchrun --nproc-per-node 4 --master-addr 127.0.0.1 -m mpi_cuda_amd 128 0.001 20 --backend cpu  # MPI analogue

``--checkpoint PREFIX`` dumps u^{K−1} and u^K (utils/dump.py format) so that ``--resume PREFIX`` can continue a run
from step K to a larger K on any backend and decomposition; the native CLI has the same flags.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m mpi_cuda_amd", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("N", type=int, help="intervals per axis ((N+1)^3 nodes)")
    ap.add_argument("tau", type=float, help="time step")
    ap.add_argument("K", type=int, help="number of steps")
    ap.add_argument("L", type=float, nargs="?", default=None, help="cube edge (default 1)")
    ap.add_argument("--box", default="", metavar="LX,LY,LZ",
                    help="rectangular box [0,LX]x[0,LY]x[0,LZ], the same N per axis (excludes the positional L)")
    ap.add_argument("--backend", default="auto", choices=["auto", "hip", "cpu", "torch"])
    ap.add_argument("--transport", default="auto", choices=["auto", "rccl", "torch", "loopback", "rccl-self", "push",
                                                               "push-ipc", "sdma", "sdma-ipc", "native", "none"])
    ap.add_argument("--world", type=int, default=0,
                    help="ranks of an in-process group on one GPU (transport loopback, or rccl-self: RCCL send/recv)")
    ap.add_argument("--decomp", default="slab", help="slab | block | PxQxR")
    ap.add_argument("--check-every", type=int, default=2)
    ap.add_argument("--threads", type=int, default=0, help="OpenMP threads of the CPU backend")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=0)
    ap.add_argument("--no-overlap", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-temporal", action="store_true")
    ap.add_argument("--temporal", type=int, default=5, help="at most this many steps per HBM pass (2..5)")
    ap.add_argument("--no-tb", action="store_true", help="two-step register-queue passes instead of the LDS kernel")
    ap.add_argument("--timers", action="store_true")
    ap.add_argument("--json", default="")
    ap.add_argument("--dump", default="", help="write u^K to PREFIX[.rankR].bin/.json")
    ap.add_argument("--checkpoint", default="", help="write u^{K-1}, u^K to PREFIX.prev / PREFIX.cur dumps")
    ap.add_argument("--resume", default="", help="continue from a --checkpoint PREFIX (any backend/transport)")
    ap.add_argument("--initial", default="", metavar="PREFIX",
                    help="solve from your own initial data: u(.,0) from the dump PREFIX.phi and, if present, u_t(.,0) "
                         "from PREFIX.psi (backends hip and cpu)")
    ap.add_argument("--energy", action="store_true",
                    help="print the discrete energy E(1/2), E(K-1/2) and its drift (with --initial)")
    ap.add_argument("--receivers", default="", metavar="FILE",
                    help="record u at grid nodes for every step 0..K: FILE lists one node per line as i j k")
    ap.add_argument("--traces", default="", metavar="OUT",
                    help="write the recorded (K+1) x R values to OUT.bin / OUT.json (utils/dump.py load_traces)")
    ap.add_argument("--sources", default="", metavar="FILE",
                    help="point sources w(t) delta(x - x_s): FILE lists one source per line as i j k f0 t0 amp (a node "
                         "strictly inside the grid and a Ricker wavelet of peak frequency f0 centred at t0); the error "
                         "lines then have no meaning (backends hip and cpu; not with --resume)")
    ap.add_argument("--sponge", default="", metavar="W[,SIGMA[,FACES]]",
                    help="absorbing sponge layers of W nodes next to the faces FACES, a subset of the letters xXyYzZ (lower "
                         "case: the low face; default all six), peak damping rate SIGMA (default 3 ln(1000) / (2 W h)); "
                         "one rank, backends hip and cpu; the error lines then have no meaning")
    ap.add_argument("--speed", default="", metavar="PREFIX",
                    help="variable wave speed: solve u_tt = c(x)^2 Lap u with c from the dump PREFIX.c (the --initial "
                         "format; face values ignored, interior values finite and > 0; courant * max c <= 1 unless "
                         "--force); one rank, backends hip (temporal 1 or 2) and cpu; not with --resume; the error lines "
                         "then have no meaning")
    ap.add_argument("--order", type=int, default=2, choices=(2, 4),
                    help="spatial order of the Laplacian (default 2). 4: the 13-point stencil with the odd reflection at the "
                         "walls, stable for courant <= sqrt(3)/2; one native rank (hip or cpu); not with --sponge, --speed, "
                         "--resume or --energy")
    ap.add_argument("--time-order", type=int, default=2, choices=(2, 4), dest="time_order",
                    help="order of the time integrator (default 2). 4: u^{n+1} = 2u^n - u^{n-1} + tau^2 L u^n + tau^4/12 L^2 u^n, "
                         "needs --order 4, stable for courant <= 3/2; runs where --order 4 runs; not with --sources")
    ap.add_argument("--force", action="store_true", help="run even if the CFL condition is violated")
    ap.add_argument("--quiet", action="store_true")
    return ap


def main(argv=None) -> int:
    ap = build_parser()
    a = ap.parse_args(argv)
    box = None
    if a.box:
        if a.L is not None:
            ap.error("--box and the positional L exclude each other")
        try:
            box = tuple(float(v) for v in a.box.split(","))
        except ValueError:
            box = ()
        if len(box) != 3 or not all(e > 0 and math.isfinite(e) for e in box):
            ap.error("--box expects three positive edges LX,LY,LZ")
        a.L = box[0]
    elif a.L is None:
        a.L = 1.0
    if a.initial and a.resume:
        ap.error("--initial and --resume exclude each other")
    if a.energy and not a.initial:
        ap.error("--energy needs --initial (E(1/2) is kept by solves that start from it)")
    if a.sources and a.resume:
        ap.error("--sources and --resume exclude each other")
    if a.order == 4 and (a.resume or a.speed or a.sponge or a.energy):
        ap.error("order: --order 4 not together with --resume, --speed, --sponge or --energy")
    if a.time_order == 4 and a.order != 4:
        ap.error("time_order: 4 needs order = 4 (--order 4)")
    if a.time_order == 4 and a.sources:
        ap.error("time_order: --time-order 4 not together with --sources")
    if a.speed and a.resume:
        ap.error("speed: not together with --resume")
    if bool(a.receivers) != bool(a.traces):
        ap.error("--receivers FILE and --traces OUT go together")
    sponge = None
    if a.sponge:
        part = a.sponge.split(",")
        try:
            if not 1 <= len(part) <= 3:
                raise ValueError(a.sponge)
            if len(part) == 3 and not part[2]:
                ap.error("--sponge: FACES is empty (leave the last comma out for all six faces)")
            sponge = (int(part[0]), float(part[1]) if len(part) > 1 and part[1] else 0.0,
                      part[2] if len(part) > 2 else 63)
        except ValueError:
            ap.error("--sponge expects W[,SIGMA[,FACES]]: an integer width and an optional number")
        if isinstance(sponge[2], str) and any(ch not in "xXyYzZ" for ch in sponge[2]):
            ap.error("--sponge: FACES is a subset of the letters xXyYzZ")
    import torch
    import torch.distributed as dist

    from . import ProblemSpec
    from .parallel.rccl import init_process_group
    from .solver import Solver
    from .utils import dump as dumpio
    from .utils.report import gcell_per_s

    spec = ProblemSpec(N=a.N, tau=a.tau, K=a.K, L=a.L, check_every=a.check_every,
                       Ly=box[1] if box else None, Lz=box[2] if box else None, sponge=sponge, order=a.order,
                       time_order=a.time_order)
    if spec.sponge is not None:
        print("wave3d: sponge layers are set: the error columns compare with the undamped eigenmode and have no meaning",
              file=sys.stderr)
    box_note = " box=" + ",".join(f"{e:g}" for e in spec.edges) if spec.is_box else ""
    if spec.time_order == 4 and not spec.cfl_ok:
        print(f"wave3d: CFL violated: courant = {spec.courant:.4f} > 3/2 for --order 4 --time-order 4 (effective "
              f"{spec.courant_eff:.4f} > 1, tau_max = {spec.tau_max * 1.5:.3e})", file=sys.stderr)
        if not a.force:
            return 2
    elif spec.order == 4 and not spec.cfl_ok:
        print(f"wave3d: CFL violated: courant = {spec.courant:.4f} > sqrt(3)/2 for --order 4 (effective "
              f"{spec.courant_eff:.4f} > 1, tau_max = {spec.tau_max * math.sqrt(3.0) / 2.0:.3e})", file=sys.stderr)
        if not a.force:
            return 2
    elif not spec.cfl_ok:
        form = "tau*sqrt(1/hx^2+1/hy^2+1/hz^2)" if spec.is_box else "tau*sqrt(3)/h"
        print(f"wave3d: CFL violated: courant = {form} = {spec.courant:.4f} > 1 (tau_max = {spec.tau_max:.3e}"
              f"{' for' + box_note if box_note else ''})", file=sys.stderr)
        if not a.force:
            return 2
    backend = a.backend
    if backend == "auto":
        backend = "hip" if torch.cuda.is_available() else "cpu"
    rank, world, local = init_process_group("gloo" if backend != "hip" or a.transport != "torch" else "nccl")
    transport = a.transport
    kw = dict(backend=backend, transport=transport, decomp=a.decomp, overlap=not a.no_overlap,
              graph=not a.no_graph, threads=a.threads, force=a.force, temporal=1 if a.no_temporal else a.temporal, tb=not a.no_tb)
    if backend == "hip":
        kw["device"] = local if a.world == 0 else 0
        kw["timers"] = a.timers
    if a.world:
        kw.update(transport=transport if transport in ("rccl-self", "push", "sdma") else "loopback", rank=0,
                  world=a.world)
    s = Solver(spec, **kw)
    if a.resume:
        prev, meta = dumpio.load(a.resume + ".prev")
        cur, meta_c = dumpio.load(a.resume + ".cur")
        for m in (meta, meta_c):  # the checkpoint must be of THIS problem (tau and L were not compared)
            for key, want in (("N", a.N), ("tau", a.tau), ("L", a.L)):
                got = m.get(key)
                if got is None or not math.isclose(float(got), float(want), rel_tol=1e-15, abs_tol=0.0):
                    print(f"wave3d: resume: checkpoint {key} = {got} differs from the run's {want}", file=sys.stderr)
                    return 2
            if any(not math.isclose(g, w, rel_tol=1e-15, abs_tol=0.0) for g, w in zip(dumpio.box_of(m), spec.edges)):
                print(f"wave3d: resume: checkpoint box {list(dumpio.box_of(m))} differs from the run's "
                      f"{list(spec.edges)}", file=sys.stderr)
                return 2
        s.set_state(prev, cur, int(meta_c["step"]))
    speed_range = None
    if a.speed:
        c, m = dumpio.load(a.speed + ".c")
        for key, want in (("N", a.N), ("tau", a.tau), ("L", a.L)):  # (the checks --initial makes)
            got = m.get(key)
            if got is None or not math.isclose(float(got), float(want), rel_tol=1e-15, abs_tol=0.0):
                print(f"wave3d: speed: dump {key} = {got} differs from the run's {want}", file=sys.stderr)
                return 2
        s.set_speed(c, a.force)
        speed_range = [float(v) for v in s.native.speed_range]
        print("wave3d: a speed field is set: the error columns compare with the constant-speed eigenmode and have no "
              "meaning", file=sys.stderr)
    if a.initial:
        fields = []
        for part in ("phi", "psi"):
            base = f"{a.initial}.{part}"
            if part == "psi" and not (os.path.exists(base + ".json") or os.path.exists(base + ".rank0.json")):
                fields.append(None)  # (no PREFIX.psi sidecar: u_t(.,0) = 0; a partial dump fails in load)
                continue
            f, m = dumpio.load(base)
            for key, want in (("N", a.N), ("tau", a.tau), ("L", a.L)):  # (the checks --resume makes)
                got = m.get(key)
                if got is None or not math.isclose(float(got), float(want), rel_tol=1e-15, abs_tol=0.0):
                    print(f"wave3d: initial: dump {key} = {got} differs from the run's {want}", file=sys.stderr)
                    return 2
            if any(not math.isclose(g, w, rel_tol=1e-15, abs_tol=0.0) for g, w in zip(dumpio.box_of(m), spec.edges)):
                print(f"wave3d: initial: dump box {list(dumpio.box_of(m))} differs from the run's "
                      f"{list(spec.edges)}", file=sys.stderr)
                return 2
            fields.append(f)
        s.set_initial(*fields)
    nodes = None
    if a.receivers:
        if world > 1:
            print("wave3d: --receivers / --traces: one rank (or --world P in this process) only; gathering traces from "
                  "several processes is not implemented", file=sys.stderr)
            return 2
        nodes = dumpio.load_receivers(a.receivers)
        s.set_receivers(nodes)
    n_sources = 0
    if a.sources:
        if world > 1:
            print("wave3d: sources: one rank (or --world P in this process) only; ranks of a multi-process world are not "
                  "supported", file=sys.stderr)
            return 2
        from .utils.wavelets import load_sources

        src_nodes, src_w = load_sources(a.sources, a.tau, a.K)
        s.set_sources(src_nodes, src_w)
        n_sources = int(src_nodes.shape[0])
    r = None
    times = []
    for i in range(a.warmup + a.repeat):
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        r = s.run()
        if i >= a.warmup:
            times.append(time.perf_counter() - t0)
    t = torch.tensor([min(times)], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    best = float(t[0])
    if rank == 0:
        if not a.quiet:
            print(f"wave3d: N={a.N} tau={a.tau:g} K={a.K} L={a.L:g}{box_note} backend={s.backend} transport={s.transport} "
                  f"ranks={s.world} decomp={'x'.join(map(str, s.dims))}")
            for line in r.lines():
                print(line)
        if a.energy:
            e_start, e_end = s.energy(1), s.energy(0)
            print(f"Energy: E(1/2) = {e_start:.15e}, E(K-1/2) = {e_end:.15e}, drift = {abs(e_end - e_start) / e_start:.3e}")
        cells = spec.cell_updates if not a.resume else float(a.N) ** 3 * (a.K - int(meta_c["step"]))
        print(f"Total time: {best:.6f} s, {cells / best / 1e9:.2f} GCell/s")
        ph = r.extra.get("phases")
        if a.timers and ph:
            print("Phases (device ms): " + ", ".join(f"{k} {v:.3f}" for k, v in ph.items()))
        if a.json:
            with open(a.json, "w") as f:
                json.dump({"backend": s.backend, "transport": s.transport, "N": a.N, "tau": a.tau, "K": a.K, "L": a.L,
                           **({"box": list(spec.edges)} if spec.is_box else {}), "ranks": s.world, "dims": list(s.dims), "solve_s": best,
                           "finite": bool(r.finite),
                           "gcell_per_s": gcell_per_s(a.N, a.K, best),
                           **({"energy_start": e_start, "energy_end": e_end} if a.energy else {}),
                           **({"sources": n_sources} if a.sources else {}),
                           **({"sponge": list(spec.sponge)} if spec.sponge is not None else {}),
                           **({"speed": speed_range} if speed_range is not None else {}),
                           **({"order": spec.order} if spec.order != 2 else {}),
                           **({"time_order": spec.time_order} if spec.time_order != 2 else {}),
                           "steps": [[n, m, e] for n, m, e in zip(r.steps, r.max_err, r.rms_err)]}, f)
    if a.traces:
        dumpio.save_traces(a.traces, s.traces().numpy(), nodes, N=a.N, K=a.K, L=a.L, tau=a.tau, box=spec.edges,
                           extra={**({"space_order": spec.order} if spec.order != 2 else {}),
                                  **({"time_order": spec.time_order} if spec.time_order != 2 else {})} or None)
    if a.dump or a.checkpoint:
        sponge_meta = {"sponge": list(spec.sponge)} if spec.sponge is not None else None  # (absent without a sponge)
        if speed_range is not None:  # (... and a speed field only when set: the interior minimum and maximum of c)
            sponge_meta = {**(sponge_meta or {}), "speed": speed_range}
        if spec.order != 2:  # (... and the spatial order only when it is not 2; "order" is the memory order there)
            sponge_meta = {**(sponge_meta or {}), "space_order": spec.order}
        if spec.time_order != 2:
            sponge_meta = {**(sponge_meta or {}), "time_order": spec.time_order}

        def write(prefix, which):
            if s.transport in ("loopback", "rccl-self", "push", "sdma"):
                if rank == 0:
                    dumpio.save(prefix, s.global_field(which).numpy(), N=a.N, L=a.L, tau=a.tau,
                                step=a.K - which, box=spec.edges, extra=sponge_meta)
                return
            f = s.owned_field(which)
            off = s.native.plan.box[0::2] if s.transport == "torch" else (0, 0, 0)
            dumpio.save(prefix, f.numpy(), N=a.N, L=a.L, tau=a.tau, step=a.K - which, offset=off, rank=rank,
                        world=s.world, dims=s.dims, box=spec.edges, extra=sponge_meta)

        if a.dump:
            write(a.dump, 0)
        if a.checkpoint:
            write(a.checkpoint + ".cur", 0)
            write(a.checkpoint + ".prev", 1)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0 if r.finite else 3


if __name__ == "__main__":
    sys.exit(main())
