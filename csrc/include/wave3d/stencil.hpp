// The numerical core shared verbatim by the CPU path and every HIP kernel.
//
// Every translation unit is compiled with -ffp-contract=off, so these expressions are evaluated with the same rounding
// sequence on host and device: this is what makes the GPU field bit-identical to the CPU path and to itself under every
// domain decomposition (the reference's "1-GPU log == 2-GPU log" property, report.pdf p.15-16 §4.3.1-4.3.2).
#pragma once

#include <cmath>

#include "wave3d/common.hpp"

namespace wave3d {

// h²·Δ_h u: the sum of the three second differences of the 7-point Laplacian at a node with centre value c
// (report.pdf p.5 §2.1). The domain is a cube with the same N on every axis, so the differences share one 1/h² factor,
// which the update formulas fold into their coefficient (Coeffs::lam = τ²/h², half_lam = τ²/(2h²)): 12 instead of 15
// f64 operations per node and step in the hot kernels. The differences keep the reference's form
// (u_{i+1} − 2u_i + u_{i−1}): the 512³ log stays identical to the reference's printed digits, which a neighbour-sum
// form (Σ − 6c) does not (it moves the 7th digit of the L∞ lines).
//
// On the device each difference's first half is one v_fma_f64: 2c is exact (a power-of-two scale), so
// fma(−2, c, xp) rounds the same exact value xp − 2c once, as xp − (2c) does — bit-identical to the host form, one
// f64 operation per node and step fewer (no separate 2c; the leapfrog's 2c − old is fma(2, c, −old) likewise).
W3D_HD double d2sum(double c, double xm, double xp, double ym, double yp, double zm, double zp) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (__builtin_fma(-2.0, c, xp) + xm) + (__builtin_fma(-2.0, c, yp) + ym) + (__builtin_fma(-2.0, c, zp) + zm);
#else
  const double c2 = 2.0 * c;
  return (xp - c2 + xm) + (yp - c2 + ym) + (zp - c2 + zm);
#endif
}

// The same sum on a rectangular box (h_d = L_d/N): h_x²·Δ_h u = d_x + ry·d_y + rz·d_z with ry = h_x²/h_y², rz = h_x²/h_z²
// (Coeffs), each difference taken exactly as above and combined as fma(rz, d_z, fma(ry, d_y, d_x)); lam = τ²/h_x² stays
// the single update coefficient. With ry = rz = 1 both fmas are exact-product additions, (d_x + d_y) + d_z rounded as
// d2sum rounds it: the box form fed ratios of 1 reproduces the cube's bits. On the device the ratios are wave-uniform
// kernel arguments (scalar registers): two v_add_f64 become two v_fma_f64 with a scalar operand.
W3D_HD double d2sum_box(double c, double xm, double xp, double ym, double yp, double zm, double zp, double ry,
                        double rz) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fma(rz, __builtin_fma(-2.0, c, zp) + zm,
                       __builtin_fma(ry, __builtin_fma(-2.0, c, yp) + ym, __builtin_fma(-2.0, c, xp) + xm));
#else
  const double c2 = 2.0 * c;
  return std::fma(rz, zp - c2 + zm, std::fma(ry, yp - c2 + ym, xp - c2 + xm));
#endif
}
// (kernels with a compile-time box flag)
template <bool BOX>
W3D_HD double d2sum_t(double c, double xm, double xp, double ym, double yp, double zm, double zp, double ry, double rz) {
  if constexpr (BOX)
    return d2sum_box(c, xm, xp, ym, yp, zm, zp, ry, rz);
  else
    return d2sum(c, xm, xp, ym, yp, zm, zp);
}

// Fourth-order operator (Problem::order = 4). Per axis 12h²·D₄u_i = −u_{i−2} + 16u_{i−1} − 30u_i + 16u_{i+1} − u_{i+2},
// evaluated as fma(16, m1 + p1, fma(−30, c, −(m2 + p2))): two additions and two fused operations, the same IEEE
// sequence on host and device. The 1/12 lives in the update coefficient (Coeffs::lam = τ²/(12h²) for order 4), so
// leapfrog / first_step take d4sum as they take d2sum. The axes are combined as d2sum / d2sum_box combine theirs; with
// ry = rz = 1 the box form rounds as the cube form does. A neighbour at distance 2 that lies outside the domain (the
// centre is node 1 or N − 1 of that axis) is the odd reflection u_{−1} = −u_1, u_{N+1} = −u_{N−1}: the caller passes
// −c for it, never a loaded value.
W3D_HD double d4axis(double c, double m2, double m1, double p1, double p2) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fma(16.0, m1 + p1, __builtin_fma(-30.0, c, -(m2 + p2)));
#else
  return std::fma(16.0, m1 + p1, std::fma(-30.0, c, -(m2 + p2)));
#endif
}
template <bool BOX>
W3D_HD double d4sum_t(double c, double xmm, double xm, double xp, double xpp, double ymm, double ym, double yp, double ypp,
                      double zmm, double zm, double zp, double zpp, double ry, double rz) {
  const double dx = d4axis(c, xmm, xm, xp, xpp), dy = d4axis(c, ymm, ym, yp, ypp), dz = d4axis(c, zmm, zm, zp, zpp);
  if constexpr (BOX) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fma(rz, dz, __builtin_fma(ry, dy, dx));
#else
    return std::fma(rz, dz, std::fma(ry, dy, dx));
#endif
  } else {
    return (dx + dy) + dz;
  }
}

// Leapfrog update u^{n+1} = 2u^n − u^{n−1} + τ² Δ_h u^n (report.pdf p.5 §2.2(3)), with s = d2sum and lam = τ²/h².
// The τ²-term is fused: (2c − old) + lam·s rounded once (one v_fma_f64: 10 instead of 11 f64 operations per node and
// step). Host and device round identically (std::fma is the IEEE fused operation); the printed 128³ / 512³ logs keep
// every digit of the reference's (checked for N = 128, 256, 512 and L = 1, π: profiles/r3/fma_forms.md).
W3D_HD double leapfrog(double c, double old, double s, double lam) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fma(lam, s, __builtin_fma(2.0, c, -old));
#else
  return std::fma(lam, s, 2.0 * c - old);
#endif
}

// Damped leapfrog (sponge layers): u_tt + 2σu_t = Δu with u_t centred in time, (1 + g)·u^{n+1} = 2u^n − (1 − g)·u^{n−1} +
// τ²Δ_h u^n, g = σ(x)·τ ≥ 0. With w = leapfrog(c, old, s, lam), exactly the undamped value, u^{n+1} = (w + g·old)/(1 + g) =
// fma(g, old, w)·r with r = 1.0/(1.0 + g) tabulated (problem.hpp sponge_tables). Where g == 0 the result is w itself,
// not the damped expression fed a zero: a node outside the sponge gets the undamped bits by construction. Von Neumann:
// (1 + g)z² − (2 − λ)z + (1 − g) = 0 with λ ∈ [0, 4] under the undamped CFL limit has |z₁z₂| = (1 − g)/(1 + g) ≤ 1 and,
// for real roots, |z₁ + z₂| = |2 − λ|/(1 + g) ≤ 1 + z₁z₂ = 2/(1 + g): both roots in the closed unit disc for every g ≥ 0,
// so the damping costs no time step.
W3D_HD double leapfrog_damped(double w, double old, double g, double r) {
#if defined(__HIP_DEVICE_COMPILE__)
  return g > 0.0 ? __builtin_fma(g, old, w) * r : w;
#else
  return g > 0.0 ? std::fma(g, old, w) * r : w;
#endif
}

// Second-order first step u^1 = u^0 + τ²/2 Δ_h u^0, using ∂u/∂t = 0 (report.pdf p.5 §2.2(2)); half_lam = τ²/(2h²).
// (fused like leapfrog)
W3D_HD double first_step(double c, double s, double half_lam) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fma(half_lam, s, c);
#else
  return std::fma(half_lam, s, c);
#endif
}

// First step from user-supplied initial data φ = u(·,0), ψ = u_t(·,0) (set_initial): u¹ = φ + τψ + (τ²/2)Δ_h φ, evaluated
// as fma(τ, ψ, first_step(φ, s, half_lam)) — the ψ = 0 value first, exactly as above, then the τψ term added by ONE fma
// applied last. Without ψ the fma is skipped entirely (not fed a zero): u¹ then is first_step's value bit for bit, so
// the eigenmode array given as φ reproduces init_first's u¹.
W3D_HD double first_step_psi(double u1, double psi, double tau) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fma(tau, psi, u1);
#else
  return std::fma(tau, psi, u1);
#endif
}

// Fourth order in time (Problem::time_order = 4; modified equation / Lax–Wendroff):
//   u^{n+1} = 2u^n − u^{n−1} + τ²L_h u^n + (τ⁴/12)·L_h²u^n,
// L_h the fourth-order operator, applied twice through d4sum_t with lam = τ²/(12h_x²) (Coeffs::lam):
//   v = lap_t4(s(u^n), lam) = τ²L_h u^n on every interior node; v is exactly 0 on the six faces and, like u, its own odd
//   reflection beyond a wall (L_h u is odd about a wall where u is), so s(v) takes −v for a distance-2 neighbour outside;
//   u^{n+1} = leapfrog_t4(u^n, u^{n−1}, v, s(v), lam12), lam12 = lam/12: (τ⁴/12)L_h²u = lam12·s(v).
// For the eigenmode s(φ) = −σφ and z = lam·σ: the step's symbol is 2 − z + z²/12 = 2cos(ω_hτ), stable iff 0 ≤ z ≤ 12.
W3D_HD double lap_t4(double s, double lam) { return lam * s; }
W3D_HD double leapfrog_t4(double c, double old, double v, double sv, double lam12) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fma(lam12, sv, __builtin_fma(2.0, c, -old) + v);
#else
  return std::fma(lam12, sv, (2.0 * c - old) + v);
#endif
}
// Its first step, local error O(τ⁵): u¹ = φ + ½τ²L_hφ + (τ⁴/24)L_h²φ + τ(ψ + (τ²/6)L_hψ). With vφ = lap_t4(s(φ), lam):
//   u¹ = first_step_t4(φ, vφ, s(vφ), lam24), lam24 = lam/24 — for the eigenmode the factor 1 − z/2 + z²/24 = cos(ω_hτ);
//   with ψ: u¹ = first_step_t4_psi(u¹, ψ, s(ψ), lam6, τ), lam6 = lam/6, applied last and skipped entirely without ψ
//   (first_step_psi's convention).
W3D_HD double first_step_t4(double c, double v, double sv, double lam24) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fma(lam24, sv, __builtin_fma(0.5, v, c));
#else
  return std::fma(lam24, sv, std::fma(0.5, v, c));
#endif
}
W3D_HD double first_step_t4_psi(double u1, double psi, double spsi, double lam6, double tau) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fma(tau, __builtin_fma(lam6, spsi, psi), u1);
#else
  return std::fma(tau, std::fma(lam6, spsi, psi), u1);
#endif
}

// IEEE fused multiply-add on the host (bindings: the numpy emulators' rounding primitive)
inline double fma_exact(double a, double b, double c) { return std::fma(a, b, c); }

// The error check's analytic value u_a = φ·cos(a_t t) at a node: ((s_x·s_y)·ct)·s_z. The row factor (s_x·s_y)·ct is
// shared by a whole z row (one product per node), and the squared error is accumulated with one fma (err_acc).
W3D_HD double analytic_row(double sx, double sy, double ct) { return (sx * sy) * ct; }
W3D_HD double err_sq_acc(double e, double acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fma(e, e, acc);
#else
  return std::fma(e, e, acc);
#endif
}

// φ at a global node from the separable table (boundary entries are exact zeros, see problem.hpp::sin_table).
W3D_HD double phi(const double* s, i64 gi, i64 gj, i64 gk) { return (s[gi] * s[gj]) * s[gk]; }

}  // namespace wave3d
