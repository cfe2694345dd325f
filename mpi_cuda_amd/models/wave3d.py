"""The 3D wave-equation "model": problem definition, analytic solution, closed-form discrete oracle and an independent
PyTorch fp64 reference solver.

Reference behaviour (AICCer1/MPI-CUDA; the programs are not in the snapshot, the documents are — SURVEY.md §0.1):

* PDE u_tt = Δu on [0,L]³, homogeneous Dirichlet BCs, u(t=0) = φ, u_t(t=0) = 0              report.pdf p.4 §1
* analytic u_a = sin(πx/L)·sin(πy/L)·sin(πz/L)·cos(a_t t), a_t = π·√3/L                    report.pdf p.4 §1
* grid x_i = i·h, h = L/N, nodes 0..N; leapfrog with the 7-point Laplacian;
  u¹ = u⁰ + τ²/2·Δ_h u⁰                                                                        report.pdf p.5 §2-2.2
* "Max Error" = L∞ over the nodes, "L2 Error" = RMS over the (N−1)³ interior nodes           report.pdf p.6 §3.1.2,
                                                                                               SURVEY.md §1.3 VERIFIED
* rectangular box [0,Lx]×[0,Ly]×[0,Lz], same N per axis: u_a = Π_d sin(π x_d/L_d)·cos(a_t t),
  a_t = π·√(1/Lx²+1/Ly²+1/Lz²), h_d = L_d/N (``ProblemSpec(Ly=, Lz=)``; L is Lx)                   report.pdf p.4 §1
* golden log (512³, τ=1e-3, K=20, L=1)                                                        report.pdf p.15-16 §4.3

The closed-form oracle: φ is a discrete eigenfunction of Δ_h with eigenvalue −λ, so the discrete
solution is exactly cos(nθ)·φ with cos θ = 1 − τ²λ/2. The error at step n is d_n·|φ| with d_n = |cos nθ − cos(a_t nτ)|,
giving L∞ = d_n·max|φ| and RMS = d_n·(Σφ²/(N−1)³)^½ — evaluated here in 50-digit arithmetic (mpmath), because the
two cosines cancel in fp64.
"""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass, field

import numpy as np
import torch

# Golden per-step log of the reference's GPU program, 1 and 2 GPUs identical (report.pdf p.15-16 §4.3.1-4.3.2).
REFERENCE_LOG_512 = [
    (2, 3.967859e-11, 1.406978e-11),
    (4, 1.587058e-10, 5.627573e-11),
    (6, 3.570526e-10, 1.266079e-10),
    (8, 6.346724e-10, 2.250497e-10),
    (10, 9.915001e-10, 3.515776e-10),
    (12, 1.427449e-09, 5.061618e-10),
    (14, 1.942419e-09, 6.887656e-10),
    (16, 2.536286e-09, 8.993458e-10),
    (18, 3.208909e-09, 1.137852e-09),
    (20, 3.960129e-09, 1.404229e-09),
]


@dataclass
class ProblemSpec:
    """N intervals per axis ((N+1)³ nodes), time step tau, K steps, cube edge L (positional CLI ``N tau K [L]``).

    ``Ly`` / ``Lz`` make the domain a rectangular box Lx × Ly × Lz with Lx = L (CLI ``--box LX,LY,LZ``); None means
    "= L". A spec whose three edges are equal is a cube and evaluates exactly the cube's expressions.

    ``sponge = (width, sigma, faces)`` (or just ``width``, or ``(width, sigma)``) puts an absorbing layer of ``width``
    nodes next to the faces of the mask ``faces`` (bits 0..5: x-, x+, y-, y+, z-, z+, or a string of the letters
    ``xXyYzZ``, lower case = low face; default all six) with peak damping rate ``sigma`` (0: the default
    3 ln(1000) / (2 width h)); CLI ``--sponge W[,SIGMA[,FACES]]``. None, width 0 or faces 0: no sponge.

    ``order`` is the spatial order of the Laplacian: 2 (the 7-point stencil) or 4 (the 13-point one with the odd
    reflection u_{-1} = -u_1 at the Dirichlet walls; CLI ``--order 4``). Order 4 is stable for
    tau sqrt(sum 1/h_d^2) <= sqrt(3)/2 (``courant_eff``) and runs on one native rank, without a sponge.

    ``time_order`` is the order of the time integrator: 2 (leapfrog) or 4 (the modified-equation scheme u^{n+1} = 2u^n -
    u^{n-1} + tau^2 L u^n + tau^4/12 L^2 u^n; CLI ``--time-order 4``). It needs ``order = 4``, is stable for
    tau sqrt(sum 1/h_d^2) <= 3/2 and runs where order 4 runs, without point sources."""

    N: int = 512
    tau: float = 1e-3
    K: int = 20
    L: float = 1.0
    check_every: int = 2
    extra: dict = field(default_factory=dict)
    Ly: float | None = None
    Lz: float | None = None
    sponge: tuple | int | None = None
    order: int = 2
    time_order: int = 2

    def __post_init__(self) -> None:
        if self.order not in (2, 4):
            raise ValueError("order: the spatial order must be 2 or 4")
        if self.time_order not in (2, 4):
            raise ValueError("time_order: the time order must be 2 or 4")
        if self.time_order == 4 and self.order != 4:
            raise ValueError("time_order: 4 needs order = 4")
        if self.sponge is not None:
            sp = self.sponge if isinstance(self.sponge, (tuple, list)) else (self.sponge,)
            if not 1 <= len(sp) <= 3:
                raise ValueError("sponge: (width, sigma, faces)")
            width = int(sp[0])
            sigma = 0.0 if len(sp) < 2 or sp[1] is None else float(sp[1])
            faces = 63 if len(sp) < 3 or sp[2] is None else sp[2]
            if isinstance(faces, str):
                if not faces:
                    raise ValueError("sponge: faces is empty (None selects all six)")
                if any(ch not in "xXyYzZ" for ch in faces):
                    raise ValueError("sponge: faces is a subset of the letters xXyYzZ")
                faces = sum(1 << "xXyYzZ".index(ch) for ch in set(faces))
            faces = int(faces)
            if width < 0:
                raise ValueError("sponge: the width must be >= 0")
            if not (math.isfinite(sigma) and sigma >= 0.0):
                raise ValueError("sponge: sigma must be finite and >= 0 (0 selects the default)")
            if not 0 <= faces <= 63:
                raise ValueError("sponge: faces is a mask of bits 0..5 (x-, x+, y-, y+, z-, z+)")
            if width > 0 and faces and 2 * width > self.N - 1:
                raise ValueError(f"sponge: two layers of width {width} do not fit into the {self.N - 1} interior nodes "
                                 "of an axis (2 * width <= N - 1)")
            self.sponge = (width, sigma, faces) if width > 0 and faces else None
        if self.order == 4 and self.sponge is not None:
            raise ValueError("order: no sponge layers with order = 4 (the damped form of the fourth-order operator is a "
                             "follow-up)")
        if self.N < 2:
            raise ValueError("N must be >= 2")
        if not (self.tau > 0 and math.isfinite(self.tau)):
            raise ValueError("tau must be > 0")
        if self.K < 1:
            raise ValueError("K must be >= 1")
        if not (self.L > 0 and math.isfinite(self.L)):
            raise ValueError("L must be > 0")
        for name in ("Ly", "Lz"):
            v = getattr(self, name)
            if v is not None and not (v > 0 and math.isfinite(v)):
                raise ValueError(f"{name} must be > 0")

    @property
    def edges(self) -> tuple[float, float, float]:
        """(Lx, Ly, Lz)."""
        return (self.L, self.L if self.Ly is None else float(self.Ly), self.L if self.Lz is None else float(self.Lz))

    @property
    def is_box(self) -> bool:
        lx, ly, lz = self.edges
        return ly != lx or lz != lx

    @property
    def h(self) -> float:
        """h_x (a cube's only step)."""
        return self.L / self.N

    @property
    def hs(self) -> tuple[float, float, float]:
        """(h_x, h_y, h_z)."""
        lx, ly, lz = self.edges
        return (lx / self.N, ly / self.N, lz / self.N)

    @property
    def inv_h2_sum(self) -> float:
        """Σ_d 1/h_d², summed as (x + y) + z (problem.hpp::Problem::inv_h2_sum: the same bits)."""
        hx, hy, hz = self.hs
        return (1.0 / (hx * hx) + 1.0 / (hy * hy)) + 1.0 / (hz * hz)

    @property
    def ratios(self) -> tuple[float, float]:
        """(ry, rz) = (h_x²/h_y², h_x²/h_z²), the weights of stencil.hpp::d2sum_box (problem.hpp::Coeffs)."""
        if not self.is_box:
            return (1.0, 1.0)
        hx, hy, hz = self.hs
        return ((hx * hx) / (hy * hy), (hx * hx) / (hz * hz))

    @property
    def a_t(self) -> float:
        if not self.is_box:
            return math.pi * math.sqrt(3.0 / (self.L * self.L))
        lx, ly, lz = self.edges
        return math.pi * math.sqrt((1.0 / (lx * lx) + 1.0 / (ly * ly)) + 1.0 / (lz * lz))

    @property
    def courant(self) -> float:
        """τ·√(Σ 1/h_d²) (cube: τ·√3/h) — the 3-D 7-point leapfrog is stable iff this is ≤ 1."""
        if self.is_box:
            return self.tau * math.sqrt(self.inv_h2_sum)
        return self.tau * math.sqrt(3.0) / self.h

    @property
    def courant_eff(self) -> float:
        """The order-aware Courant number: courant·2/√3 for order 4 (the largest symbol of −h²D₄ is 16/3 against 4), courant
        itself for order 2 (problem.hpp::Problem::courant_eff)."""
        if self.time_order == 4:  # (the step's symbol 2 - z + z^2/12 stays in [-2, 2] iff z = 16/3 courant^2 <= 12)
            return self.courant * (2.0 / 3.0)
        return self.courant * (2.0 / math.sqrt(3.0)) if self.order == 4 else self.courant

    @property
    def courant_limit(self) -> float:
        """``courant`` at the scheme's stability limit: 1, sqrt(3)/2 for order 4, 3/2 for order 4 with time order 4."""
        return 1.5 if self.time_order == 4 else math.sqrt(3.0) / 2.0 if self.order == 4 else 1.0

    @property
    def cfl_ok(self) -> bool:
        return self.courant_eff <= 1.0

    @property
    def tau_max(self) -> float:
        if self.is_box:
            return 1.0 / math.sqrt(self.inv_h2_sum)
        return self.h / math.sqrt(3.0)

    @property
    def cell_updates(self) -> float:
        """N³·K — the reference-derived GCell/s numerator."""
        return float(self.N) ** 3 * self.K

    def check_steps(self) -> list[int]:
        ce = self.check_every
        return [n for n in range(1, self.K + 1) if (ce > 0 and n % ce == 0) or n == self.K]

    def native(self):
        from .._native import load

        C = load()
        kw = {} if self.sponge is None else {"sponge": C.Sponge(*self.sponge)}
        if self.order != 2:
            kw["order"] = self.order
        if self.time_order != 2:
            kw["time_order"] = self.time_order
        if self.Ly is None and self.Lz is None:
            return C.Problem(self.N, self.tau, self.K, self.L, **kw)
        _, ly, lz = self.edges
        return C.Problem(self.N, self.tau, self.K, self.L, Ly=ly, Lz=lz, **kw)

    def as_dict(self) -> dict:
        d = asdict(self)
        d.pop("extra", None)
        if self.Ly is None and self.Lz is None:  # (a cube's dictionary is what it always was)
            d.pop("Ly")
            d.pop("Lz")
        else:
            d["Ly"], d["Lz"] = self.edges[1], self.edges[2]
        if self.order == 2:  # (... and so is a second-order spec's)
            d.pop("order")
        if self.time_order == 2:
            d.pop("time_order")
        if self.sponge is None:  # (... and so is a spec's without a sponge)
            d.pop("sponge")
        else:
            d["sponge"] = list(self.sponge)
        return d


def sin_table(spec: ProblemSpec) -> np.ndarray:
    """sin(π x_i / L), i = 0..N, boundary entries exactly 0 (same values the kernels use)."""
    i = np.arange(spec.N + 1, dtype=np.float64)
    s = np.sin(np.pi * (i * spec.h) / spec.L)
    s[0] = 0.0
    s[-1] = 0.0
    return s


def analytic(spec: ProblemSpec, n: int, dtype=torch.float64, device="cpu") -> torch.Tensor:
    """u_a at step n on the full (N+1)³ node grid."""
    s = torch.as_tensor(sin_table(spec), dtype=dtype, device=device)
    ct = math.cos(spec.a_t * (n * spec.tau))
    return ((s[:, None, None] * s[None, :, None]) * ct) * s[None, None, :]  # stencil.hpp::analytic_row order


# ----------------------------------------------------------------------------------------------------------------
# closed-form oracle
# ----------------------------------------------------------------------------------------------------------------
def oracle_errors(spec: ProblemSpec, steps: list[int] | None = None, dps: int = 50) -> dict[int, tuple[float, float]]:
    """Exact (L∞, RMS-interior) error of the discrete scheme at each step, from the closed form of SURVEY.md §1.6.
    ``order = 4``: λ_h = Σ_d (30 − 32cos(π/N) + 2cos(2π/N))/(12h_d²); ``time_order = 4``: cos θ = 1 − z/2 + z²/24 with
    z = τ²λ_h, the first step's factor and half the recurrence's symbol 2 − z + z²/12."""
    import mpmath as mp

    mp.mp.dps = dps
    N = spec.N
    L = mp.mpf(spec.L)
    h = L / N
    tau = mp.mpf(spec.tau)
    if spec.is_box:
        # λ_h = 4·sin²(π/(2N))·Σ_d 1/h_d²: the same sine table on every axis (sin(π i h_d/L_d) = sin(π i/N))
        Ls = [mp.mpf(e) for e in spec.edges]
        lam = 4 * mp.sin(mp.pi / (2 * N)) ** 2 * mp.fsum(1 / (e / N) ** 2 for e in Ls)
        a_t = mp.pi * mp.sqrt(mp.fsum(1 / e**2 for e in Ls))
    else:
        lam = 3 * (4 / h**2) * mp.sin(mp.pi * h / (2 * L)) ** 2
        a_t = mp.pi * mp.sqrt(3 / L**2)
    if spec.order == 4:
        th = mp.pi / N
        lam = (30 - 32 * mp.cos(th) + 2 * mp.cos(2 * th)) / 12 * mp.fsum(1 / (mp.mpf(e) / N) ** 2 for e in spec.edges)
        a_t = mp.pi * mp.sqrt(mp.fsum(1 / mp.mpf(e) ** 2 for e in spec.edges))
    z = tau**2 * lam
    cos_theta = 1 - z / 2 + z**2 / 24 if spec.time_order == 4 else 1 - z / 2
    theta = mp.acos(cos_theta)
    # max_i |sin(π i/N)|³ and Σ_interior φ² = (Σ_i sin²(π i/N))³
    s_max = max(abs(mp.sin(mp.pi * i / N)) for i in range(N + 1))
    s2 = mp.fsum(mp.sin(mp.pi * i / N) ** 2 for i in range(1, N))
    rms_fac = mp.sqrt(s2**3 / mp.mpf(N - 1) ** 3)
    out = {}
    for n in steps if steps is not None else spec.check_steps():
        d = abs(mp.cos(n * theta) - mp.cos(a_t * n * tau))
        out[n] = (float(d * s_max**3), float(d * rms_fac))
    return out


def oracle_energy(spec: ProblemSpec, n: int, dps: int = 50) -> float:
    """Discrete energy E^{n+1/2} of the eigenmode solve in closed form (cpu.hpp ``cpu_energy`` has the definition).
    u^n = cos(nθ)·φ and φ is an eigenfunction of −Δ_h with eigenvalue λ, so (summation by parts, zero boundary)

        E^{n+1/2} = ½‖φ‖²_V·[(cos((n+1)θ) − cos(nθ))²/τ² + λ·cos((n+1)θ)·cos(nθ)],   ‖φ‖²_V = V·(N/2)³, V = hx·hy·hz

    with λ, θ as in ``oracle_errors``; evaluated in ``dps``-digit arithmetic. It does not depend on n."""
    import mpmath as mp

    mp.mp.dps = dps
    N = spec.N
    tau = mp.mpf(spec.tau)
    hs = [mp.mpf(e) / N for e in spec.edges]
    lam = 4 * mp.sin(mp.pi / (2 * N)) ** 2 * mp.fsum(1 / h**2 for h in hs)
    theta = mp.acos(1 - tau**2 * lam / 2)
    c0, c1 = mp.cos(n * theta), mp.cos((n + 1) * theta)
    norm2 = hs[0] * hs[1] * hs[2] * (mp.mpf(N) / 2) ** 3
    return float(norm2 / 2 * ((c1 - c0) ** 2 / tau**2 + lam * c1 * c0))


# ----------------------------------------------------------------------------------------------------------------
# independent PyTorch fp64 reference solver (second oracle; runs on CPU or GPU)
# ----------------------------------------------------------------------------------------------------------------
def d2sum_torch(u: torch.Tensor, ratios: tuple[float, float] | None = None) -> torch.Tensor:
    """h_x²·Δ_h on the interior of a full node grid: the sum of the three second differences (stencil.hpp::d2sum, same
    operation order as the native kernels). ``ratios`` = (ry, rz): the box form fma(rz, d_z, fma(ry, d_y, d_x))
    (stencil.hpp::d2sum_box)."""
    c = u[1:-1, 1:-1, 1:-1]
    c2 = 2.0 * c
    dx = u[2:, 1:-1, 1:-1] - c2 + u[:-2, 1:-1, 1:-1]
    dy = u[1:-1, 2:, 1:-1] - c2 + u[1:-1, :-2, 1:-1]
    dz = u[1:-1, 1:-1, 2:] - c2 + u[1:-1, 1:-1, :-2]
    if ratios is None:
        return (dx + dy) + dz
    return fma_torch(ratios[1], dz, fma_torch(ratios[0], dy, dx))


def fma_torch(a: float, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """a·b + c rounded once (stencil.hpp's fused leapfrog / first step; torch has no fused multiply-add): the
    elementwise IEEE fma of the native binding, on a host copy."""
    from mpi_cuda_amd._native import load

    bb, cc = torch.broadcast_tensors(b, c)
    bn = bb.detach().to("cpu", torch.float64).contiguous().numpy().ravel()
    cn = cc.detach().to("cpu", torch.float64).contiguous().numpy().ravel()
    an = np.full_like(bn, a)
    r = np.asarray(load().fma_array(an, bn, cn)).reshape(tuple(bb.shape))
    return torch.from_numpy(r).to(b.device)


def laplacian_torch(u: torch.Tensor, h: float) -> torch.Tensor:
    """7-point Δ_h on the interior of a full node grid."""
    return d2sum_torch(u) * (1.0 / (h * h))


def torch_reference_solve(spec: ProblemSpec, device="cpu", return_fields: bool = False):
    """Plain PyTorch fp64 implementation of report.pdf p.5 §2.2. Returns {step: (Linf, RMS)} (+ (u^K, u^{K-1}))."""
    tau2 = spec.tau * spec.tau
    u0 = analytic(spec, 0, device=device)
    u0[0], u0[-1] = 0.0, 0.0
    u0[:, 0], u0[:, -1] = 0.0, 0.0
    u0[:, :, 0], u0[:, :, -1] = 0.0, 0.0
    u1 = torch.zeros_like(u0)
    ih2 = 1.0 / (spec.h * spec.h)
    lam, half_lam = tau2 * ih2, (0.5 * tau2) * ih2  # problem.hpp::Coeffs: the coefficients of d2sum
    ratios = spec.ratios if spec.is_box else None
    u1[1:-1, 1:-1, 1:-1] = fma_torch(half_lam, d2sum_torch(u0, ratios), u0[1:-1, 1:-1, 1:-1])
    denom = float(spec.N - 1) ** 3
    errs = {}
    checks = set(spec.check_steps())

    def err(u, n):
        e = (u[1:-1, 1:-1, 1:-1] - analytic(spec, n, device=device)[1:-1, 1:-1, 1:-1]).abs()
        return float(e.max()), math.sqrt(float((e * e).sum()) / denom)

    if 1 in checks:
        errs[1] = err(u1, 1)
    prev, cur = u0, u1
    for n in range(1, spec.K):
        nxt = torch.zeros_like(cur)
        c = cur[1:-1, 1:-1, 1:-1]
        nxt[1:-1, 1:-1, 1:-1] = fma_torch(lam, d2sum_torch(cur, ratios), 2.0 * c - prev[1:-1, 1:-1, 1:-1])
        prev, cur = cur, nxt
        if n + 1 in checks:
            errs[n + 1] = err(cur, n + 1)
    if return_fields:
        return errs, cur, prev
    return errs
