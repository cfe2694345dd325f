// Problem specification: PDE, grid, scheme coefficients, analytic solution, CFL guard.
//
// Reference behaviour (AICCer1/MPI-CUDA, documents only — see SURVEY.md §1):
//   * u_tt = Δu on [0,L]^3, homogeneous Dirichlet on all faces        (report.pdf p.4 §1)
//   * grid x_i = i*h, h = L/N, nodes 0..N (N = number of intervals)   (report.pdf p.5 §2; SURVEY §1.2 VERIFIED)
//   * u^0 = φ, u^1 = u^0 + τ²/2 Δ_h u^0, u^{n+1} = 2u^n − u^{n−1} + τ² Δ_h u^n   (report.pdf p.5 §2.2)
//   * analytic u_a = sin(πx/L) sin(πy/L) sin(πz/L) cos(a_t t), a_t = π√3/L        (report.pdf p.4 §1)
//   * CLI positional "N tau K [L]"                                   (report.pdf p.15 §4.2.4)
//   * rectangular box [0,Lx]×[0,Ly]×[0,Lz] with the same N per axis: u_a = Π_d sin(π x_d/L_d)·cos(a_t t),
//     a_t = π√(1/Lx²+1/Ly²+1/Lz²), h_d = L_d/N (report.pdf p.4 §1). The sine table is the cube's:
//     sin(π·i·h_d/L_d) = sin(π·i/N) on every axis.
#pragma once

#include <cmath>
#include <string>
#include <vector>

#include "wave3d/common.hpp"

namespace wave3d {

// Absorbing sponge layer next to a subset of the six faces: u_tt + 2σ(x)u_t = Δu with σ > 0 only inside the layer
// (sponge_tables below has the profile; stencil.hpp::leapfrog_damped the update). width = 0 or faces = 0: no sponge, and
// nothing anywhere changes.
struct Sponge {
  int width = 0;       // W: nodes 1 .. W−1 from a damped face are damped
  double sigma = 0.0;  // peak damping rate; ≤ 0: the default 3·ln(1000)/(2·W·h_a) per axis
  int faces = 63;      // bits 0..5: x−, x+, y−, y+, z−, z+
  bool on() const { return width > 0 && (faces & 63) != 0; }
};

struct Problem {
  i64 N = 512;        // number of intervals per axis → (N+1)^3 nodes
  double tau = 1e-3;  // time step
  int K = 20;         // number of time steps
  double L = 1.0;     // edge length in x (Lx); a cube's only edge
  double Ly = 0.0;    // edge lengths in y and z of a rectangular box; ≤ 0: "= L"
  double Lz = 0.0;
  Sponge sponge;      // absorbing layers (off by default)
  int order = 2;      // spatial order of the Laplacian: 2 (7-point) or 4 (13-point, stencil.hpp d4sum_t)
  int time_order = 2; // order of the time integrator: 2 (leapfrog) or 4 (stencil.hpp leapfrog_t4; needs order = 4)

  double Lx() const { return L; }
  double edge_y() const { return Ly > 0.0 ? Ly : L; }
  double edge_z() const { return Lz > 0.0 ? Lz : L; }
  // A problem whose three edges are equal is a cube: it keeps the cube's expressions below (and the cube's kernels),
  // so giving Ly = Lz = L changes no bit of a cube's results.
  bool is_box() const { return edge_y() != L || edge_z() != L; }
  double h() const { return L / static_cast<double>(N); }
  double hx() const { return h(); }
  double hy() const { return edge_y() / static_cast<double>(N); }
  double hz() const { return edge_z() / static_cast<double>(N); }
  i64 nodes() const { return N + 1; }
  // Σ_d 1/h_d², summed as (x + y) + z (the Python side uses the same order: same bits)
  double inv_h2_sum() const {
    const double a = hx(), b = hy(), c = hz();
    return (1.0 / (a * a) + 1.0 / (b * b)) + 1.0 / (c * c);
  }
  // a_t = π·sqrt(1/Lx² + 1/Ly² + 1/Lz²)
  double a_t() const {
    if (!is_box()) return M_PI * std::sqrt(3.0 / (L * L));
    const double ly = edge_y(), lz = edge_z();
    return M_PI * std::sqrt((1.0 / (L * L) + 1.0 / (ly * ly)) + 1.0 / (lz * lz));
  }
  // Courant number for the 3D 7-point leapfrog: stable iff τ·sqrt(Σ 1/h_d²) ≤ 1 (cube: τ·sqrt(3)/h).
  double courant() const { return is_box() ? tau * std::sqrt(inv_h2_sum()) : tau * std::sqrt(3.0) / h(); }
  bool cfl_ok() const { return courant() <= 1.0; }
  // Order-aware guard. The largest symbol of −h²D₄ is 16/3 against 4 for the second-order difference, so the fourth-
  // order leapfrog is stable iff τ·sqrt(Σ 1/h_d²) ≤ sqrt(3)/2: the effective Courant number is courant()·2/sqrt(3).
  // order = 2: courant() itself, the same bits.
  // time_order = 4: the step's symbol 2 − z + z²/12 stays in [−2, 2] iff 0 ≤ z ≤ 12 with z ≤ (16/3)·courant()², so the
  // limit is courant() ≤ 3/2 and the effective number courant()·(2/3). time_order = 2 keeps its expressions and bits.
  double courant_eff() const {
    if (time_order == 4) return courant() * (2.0 / 3.0);
    return order == 4 ? courant() * (2.0 / std::sqrt(3.0)) : courant();
  }
  // courant() at the stability limit of the scheme: 1 (order 2), sqrt(3)/2 (order 4), 3/2 (order 4, time order 4)
  double courant_limit() const { return time_order == 4 ? 1.5 : order == 4 ? std::sqrt(3.0) / 2.0 : 1.0; }
  bool cfl_ok_eff() const { return courant_eff() <= 1.0; }
  // Largest stable τ for this grid (second-order operator; order 4: sqrt(3)/2 of it).
  double tau_max() const { return is_box() ? 1.0 / std::sqrt(inv_h2_sum()) : h() / std::sqrt(3.0); }
  // Cell updates of one full solve (reference convention for GCell/s: N³·K).
  double cell_updates() const { return static_cast<double>(N) * N * N * K; }

  void validate() const {
    W3D_REQUIRE(N >= 2, "N must be >= 2");
    W3D_REQUIRE(tau > 0.0 && std::isfinite(tau), "tau must be > 0");
    W3D_REQUIRE(K >= 1, "K must be >= 1");
    W3D_REQUIRE(L > 0.0 && std::isfinite(L), "L must be > 0");
    W3D_REQUIRE(std::isfinite(Ly) && std::isfinite(Lz), "box edges must be finite");
    W3D_REQUIRE(order == 2 || order == 4, "order: the spatial order must be 2 or 4");
    W3D_REQUIRE(order == 2 || !sponge.on(), "order: no sponge layers with order = 4 (the damped form of the fourth-order "
                                            "operator is a follow-up)");
    W3D_REQUIRE(time_order == 2 || time_order == 4, "time_order: the time order must be 2 or 4");
    W3D_REQUIRE(time_order == 2 || order == 4, "time_order: 4 needs order = 4");
    W3D_REQUIRE(sponge.width >= 0, "sponge: the width must be >= 0");
    W3D_REQUIRE(!sponge.on() || 2 * static_cast<i64>(sponge.width) <= N - 1,
                "sponge: two layers of width " + std::to_string(sponge.width) + " do not fit into the " +
                    std::to_string(N - 1) + " interior nodes of an axis (2 * width <= N - 1)");
    W3D_REQUIRE(std::isfinite(sponge.sigma) && (sponge.sigma >= 0.0 || !sponge.on()),
                "sponge: sigma must be finite and >= 0 (0 selects the default)");
    W3D_REQUIRE(sponge.faces >= 0 && sponge.faces <= 63, "sponge: faces is a mask of bits 0..5 (x-, x+, y-, y+, z-, z+)");
  }
};

// Scheme coefficients shared by every kernel (CPU and GPU use the same values → same bits).
struct Coeffs {
  double ihx2, ihy2, ihz2;  // 1/h_d²
  double tau2;              // τ²
  double half_tau2;         // τ²/2
  double lam;               // τ²/h²: the update coefficient of d2sum (stencil.hpp); order 4: τ²/(12h²), that of d4sum_t
  double half_lam;          // (τ²/2)/h²; order 4: (τ²/2)/(12h²)
  // Rectangular box (stencil.hpp::d2sum_box): the y and z differences are weighted by h_x²/h_y², h_x²/h_z² and lam,
  // half_lam carry 1/h_x². `box` selects that form in every kernel; a cube has box = false, ry = rz = 1.
  double ry = 1.0, rz = 1.0;
  bool box = false;
  int order = 2;            // Problem::order
  int time_order = 2;       // Problem::time_order
  double lam12 = 0.0, lam24 = 0.0, lam6 = 0.0;  // time order 4 (stencil.hpp leapfrog_t4, first_step_t4): lam/12, /24, /6

  // force_box (tests): the box form also for a cube — with ry = rz = 1 it must reproduce the cube form's bits
  static Coeffs from(const Problem& p, bool force_box = false) {
    Coeffs c;
    const double h = p.h();
    c.ihx2 = 1.0 / (h * h);
    c.ihy2 = c.ihx2;
    c.ihz2 = c.ihx2;
    c.tau2 = p.tau * p.tau;
    c.half_tau2 = 0.5 * c.tau2;
    c.lam = c.tau2 * c.ihx2;
    c.half_lam = c.half_tau2 * c.ihx2;
    if (p.is_box()) {
      const double hy = p.hy(), hz = p.hz();
      c.ihy2 = 1.0 / (hy * hy);
      c.ihz2 = 1.0 / (hz * hz);
      c.ry = (h * h) / (hy * hy);
      c.rz = (h * h) / (hz * hz);
    }
    c.box = p.is_box() || force_box;
    c.order = p.order;
    if (p.order == 4) {  // (the 1/12 of the fourth-order difference; order 2 never comes here: no bit of it changes)
      c.lam = c.lam / 12.0;
      c.half_lam = c.half_lam / 12.0;
    }
    c.time_order = p.time_order;
    if (p.time_order == 4) {
      c.lam12 = c.lam / 12.0;
      c.lam24 = c.lam / 24.0;
      c.lam6 = c.lam / 6.0;
    }
    return c;
  }
};

// 1-D factor of the initial condition, sin(π x_i / L) for i = 0..N, with the two boundary entries forced to an exact 0.
// u^0(i,j,k) = (s[i]·s[j])·s[k]; because the boundary entries are 0 the same product also yields the Dirichlet zeros,
// so every kernel (init, first step, error check) evaluates φ by the identical expression.
//
// The returned table is EXTENDED by one zero entry on each side: element [g+1] holds node g for g = -1..N+1, so ghost
// nodes just outside the domain (which some ranks allocate) evaluate to 0 without a branch. Kernels receive &t[1].
inline std::vector<double> sin_table_ext(const Problem& p) {
  std::vector<double> s(static_cast<size_t>(p.N + 3), 0.0);
  const double h = p.h();
  for (i64 i = 1; i < p.N; ++i) {
    const double x = static_cast<double>(i) * h;
    s[static_cast<size_t>(i + 1)] = std::sin(M_PI * x / p.L);
  }
  return s;  // s[1] (node 0) and s[N+1] (node N) stay exact zeros
}

// Sponge coefficients. For a node d nodes from a damped face of axis a, 1 ≤ d < W, the 1-D value is
//   g_a = (τ·sigma_a)·(q·q),  q = (W − d)/W      (a quadratic ramp; 0 for d ≥ W and on or outside the boundary),
// the larger of the two where both faces of the axis reach the node, and r_a = 1.0/(1.0 + g_a) entry by entry. Default
// sigma_a = 3·ln(1000)/(2·W·h_a): the continuous two-way amplitude reflection 1e-3 of a quadratic profile at c = 1.
// Each table is extended by one entry on each side like sin_table_ext: element [i + 1] holds node i = −1..N+1. A node's
// coefficients are g = fmax(fmax(gx[i], gy[j]), gz[k]) and r = fmin(fmin(rx[i], ry[j]), rz[k]) — no division and no
// rounding where they are used, and r belongs to the same entry as g because 1/(1 + g) is monotone.
struct SpongeView {  // pointers to node 0 of the six tables (host or device), indexable −1..N+1
  const double *gx = nullptr, *gy = nullptr, *gz = nullptr, *rx = nullptr, *ry = nullptr, *rz = nullptr;
};
struct SpongeTables {
  std::vector<double> g[3], r[3];  // N + 3 entries each
  SpongeView view() const {
    return SpongeView{g[0].data() + 1, g[1].data() + 1, g[2].data() + 1, r[0].data() + 1, r[1].data() + 1, r[2].data() + 1};
  }
};
inline double sponge_sigma(const Problem& p, int axis) {
  if (p.sponge.sigma > 0.0) return p.sponge.sigma;
  const double h = axis == 0 ? p.hx() : (axis == 1 ? p.hy() : p.hz());
  return (3.0 * std::log(1000.0)) / ((2.0 * static_cast<double>(p.sponge.width)) * h);
}
inline SpongeTables sponge_tables(const Problem& p) {
  SpongeTables t;
  const i64 W = p.sponge.width;
  for (int a = 0; a < 3; ++a) {
    t.g[a].assign(static_cast<size_t>(p.N + 3), 0.0);
    t.r[a].assign(static_cast<size_t>(p.N + 3), 1.0);
    if (!p.sponge.on()) continue;
    const double ts = p.tau * sponge_sigma(p, a);
    const bool lo = (p.sponge.faces >> (2 * a)) & 1, hi = (p.sponge.faces >> (2 * a + 1)) & 1;
    for (i64 i = 1; i < p.N; ++i) {
      double g = 0.0;
      for (int side = 0; side < 2; ++side) {
        const i64 d = side == 0 ? i : p.N - i;
        if (!(side == 0 ? lo : hi) || d >= W) continue;
        const double q = static_cast<double>(W - d) / static_cast<double>(W);
        g = std::fmax(g, ts * (q * q));
      }
      t.g[a][static_cast<size_t>(i + 1)] = g;
      t.r[a][static_cast<size_t>(i + 1)] = 1.0 / (1.0 + g);
    }
  }
  return t;
}

// cos(a_t · n · τ): the time factor of the analytic solution at step n.
inline double time_factor(const Problem& p, int n) { return std::cos(p.a_t() * (static_cast<double>(n) * p.tau)); }

}  // namespace wave3d
