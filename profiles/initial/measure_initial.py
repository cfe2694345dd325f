"""512^3: k_first_step_field next to a device copy of the same bytes; a set_initial solve next to the default solve."""
import json
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from mpi_cuda_amd import ProblemSpec  # noqa: E402
from mpi_cuda_amd._native import load  # noqa: E402
from mpi_cuda_amd.solver import Solver  # noqa: E402

C = load()
N = 512
spec = ProblemSpec(N=N, tau=1e-3, K=20, L=1.0)
prob = spec.native()
lay = C.make_layout(prob, C.rank_box(prob, C.Dims(1, 1, 1), 0))
src = C.initial_layout(prob, lay)
co = C.Coeffs.from_problem(prob)
dev = torch.device("cuda", 0)
out = {}
rng = np.random.default_rng(1)
phi = rng.standard_normal((N + 1,) * 3)
psi = rng.standard_normal((N + 1,) * 3)
f = torch.from_numpy(np.asarray(C.initial_to_local(src, phi.reshape(-1)))).to(dev)
p = torch.from_numpy(np.asarray(C.initial_to_local(src, psi.reshape(-1)))).to(dev)
u0 = torch.zeros(lay.total, dtype=torch.float64, device=dev)
u1 = torch.zeros(lay.total, dtype=torch.float64, device=dev)
st = torch.cuda.current_stream().cuda_stream


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts))


for name, pp in (("phi_psi", p), ("phi_only", None)):
    t = timed(lambda: C.gpu_first_step_field(lay, src, co, spec.tau, f.data_ptr(), 0 if pp is None else pp.data_ptr(),
                                             u0.data_ptr(), u1.data_ptr(), st))
    nbytes = (src.total * (2 if pp is not None else 1) + 2 * lay.total) * 8
    half = nbytes // 16  # a copy that reads + writes the same total bytes
    a, b = torch.empty(half, dtype=torch.float64, device=dev), torch.empty(half, dtype=torch.float64, device=dev)
    tc = timed(lambda: b.copy_(a))
    out[name] = {"kernel_ms_median": t[0], "kernel_ms_min": t[1], "bytes": nbytes, "copy_ms_median": tc[0],
                 "copy_ms_min": tc[1], "kernel_GBs": nbytes / t[0] / 1e6, "copy_GBs": nbytes / tc[0] / 1e6}
    del a, b
del f, p, u0, u1
torch.cuda.empty_cache()

d = Solver(spec, backend="hip", device=0)
for _ in range(3):
    d.run()
out["default_solve_ms"] = sorted(r.solve_s * 1e3 for r in d.run_batch(20))[10]
out["default_batched"] = bool(d.run_batch(2)[0].extra["batched"])
del d
s = Solver(spec, backend="hip", device=0)
s.set_initial(phi, psi)
for _ in range(3):
    s.run()
out["initial_solve_ms"] = sorted(r.solve_s * 1e3 for r in s.run_batch(20))[10]
out["initial_batched"] = bool(s.run_batch(2)[0].extra["batched"])
out["initial_mode"] = s.native.mode
e1, ek = s.energy(1), s.energy(0)
out["energy"] = [e1, ek, abs(ek - e1) / e1]
s.set_initial(phi)
for _ in range(3):
    s.run()
out["initial_nopsi_solve_ms"] = sorted(r.solve_s * 1e3 for r in s.run_batch(20))[10]
print(json.dumps(out))
