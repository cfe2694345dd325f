"""512^3: time_order=4, order=4 and order-2 temporal=1 solvers of one build, interleaved; then the equal-accuracy pair.
Usage: python profiles/time_order/measure_512.py [all|three|equal] [output directory]"""
import json, math, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from mpi_cuda_amd.models.wave3d import ProblemSpec
from mpi_cuda_amd.solver import Solver

OUT = sys.argv[2] if len(sys.argv) > 2 else os.getcwd()  # output directory
os.makedirs(OUT, exist_ok=True)
N, K, tau = 512, 20, 5e-4
hip = dict(backend="hip", device=0)

def timed(s, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = s.run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, r

mode = sys.argv[1] if len(sys.argv) > 1 else "all"
res = {}
if mode in ("all", "three"):
    solvers = {"t4": Solver(ProblemSpec(N=N, tau=tau, K=K, order=4, time_order=4), **hip),
               "o4": Solver(ProblemSpec(N=N, tau=tau, K=K, order=4), **hip),
               "o2": Solver(ProblemSpec(N=N, tau=tau, K=K), temporal=1, **hip)}
    last = {}
    for _ in range(3):
        for k, s in solvers.items():
            timed(s)
    times = {k: [] for k in solvers}
    for _ in range(7):
        for k, s in solvers.items():
            ms, r = timed(s, 3)
            times[k].append(ms)
            last[k] = r
    for k in solvers:
        res[k] = {"min_ms": min(times[k]), "median_ms": statistics.median(times[k]), "max_ms": max(times[k]),
                  "units": len(solvers[k].native.unit_steps), "max_err_K": last[k].max_err[-1]}
    nodes = (N - 1) ** 3
    res["bound_ms_per_step_48B_at_6.29TBps"] = 48.0 * N ** 3 / 6.29e12 * 1e3
    res["bound_ms_per_step_24B_at_6.29TBps"] = 24.0 * N ** 3 / 6.29e12 * 1e3
    del solvers
if mode in ("all", "equal"):
    # equal-accuracy comparison: T fixed, each scheme at 0.9 of its limit
    T = 0.05
    eq = {}
    for name, to, lim in (("t2", 2, math.sqrt(3.0) / 2.0), ("t4", 4, 1.5)):
        tm = ProblemSpec(N=N).tau_max
        Kq = math.ceil(T / (0.9 * lim * tm))
        s = Solver(ProblemSpec(N=N, tau=T / Kq, K=Kq, check_every=Kq, order=4, time_order=to), **hip)
        timed(s)
        ts = [timed(s)[0] for _ in range(3)]
        r = s.run()
        eq[name] = {"K": Kq, "tau": T / Kq, "min_ms": min(ts), "median_ms": statistics.median(ts), "max_err_K": r.max_err[-1],
                    "finite": bool(r.finite)}
        del s
    res["equal_accuracy_T"] = T
    res["equal_accuracy"] = eq
with open(os.path.join(OUT, f"measure_512_{mode}.json"), "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
