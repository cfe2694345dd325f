// CPU path: sequential / OpenMP solver kernels on the same local layout as the GPU path.
//
// Covers the reference's sequential (wave.cpp) and OpenMP (openmpwave.cpp) programs (readme.md:33-36, report.pdf
// p.20-21 §5.1-5.2) and is the bit-exact baseline the HIP kernels are tested against.
#pragma once

#include "wave3d/decomp.hpp"
#include "wave3d/problem.hpp"

namespace wave3d {

// Local compute sub-box (local node indices, half-open).
struct LBox {
  i64 x0 = 0, x1 = 0, y0 = 0, y1 = 0, z0 = 0, z1 = 0;
  bool empty() const { return x1 <= x0 || y1 <= y0 || z1 <= z0; }
  i64 count() const { return empty() ? 0 : (x1 - x0) * (y1 - y0) * (z1 - z0); }
};

inline LBox compute_box(const Layout& l) { return LBox{l.cx0, l.cx1, l.cy0, l.cy1, l.cz0, l.cz1}; }

// Shell / interior split of a rank's compute box for the overlapped single-step schedule: the interior is the box minus
// one layer on every side that has a neighbour (nb[axis][side]); the shell is the rest, in ≤ 6 disjoint boxes (x faces
// whole, y faces inside the x range, z faces inside x and y). The one definition: GpuSolver and the Python side
// (mpi_cuda_amd.parallel.decomp.split_boxes, through the binding) both call it.
inline void shell_split(const LBox& full, const bool nb[3][2], std::vector<LBox>& shell, LBox& interior) {
  shell.clear();
  interior = full;
  if (nb[0][0]) interior.x0 += 1;
  if (nb[0][1]) interior.x1 -= 1;
  if (nb[1][0]) interior.y0 += 1;
  if (nb[1][1]) interior.y1 -= 1;
  if (nb[2][0]) interior.z0 += 1;
  if (nb[2][1]) interior.z1 -= 1;
  auto push = [&](LBox b) {
    if (!b.empty()) shell.push_back(b);
  };
  if (!full.empty()) {
    const i64 ix0 = imin(imax(interior.x0, full.x0), full.x1), ix1 = imax(interior.x1, ix0);
    const i64 iy0 = imin(imax(interior.y0, full.y0), full.y1), iy1 = imax(interior.y1, iy0);
    if (nb[0][0]) push(LBox{full.x0, full.x0 + 1, full.y0, full.y1, full.z0, full.z1});
    if (nb[0][1]) push(LBox{imax(full.x1 - 1, full.x0 + (nb[0][0] ? 1 : 0)), full.x1, full.y0, full.y1, full.z0, full.z1});
    if (nb[1][0]) push(LBox{ix0, ix1, full.y0, full.y0 + 1, full.z0, full.z1});
    if (nb[1][1]) push(LBox{ix0, ix1, imax(full.y1 - 1, full.y0 + (nb[1][0] ? 1 : 0)), full.y1, full.z0, full.z1});
    if (nb[2][0]) push(LBox{ix0, ix1, iy0, iy1, full.z0, full.z0 + 1});
    if (nb[2][1]) push(LBox{ix0, ix1, iy0, iy1, imax(full.z1 - 1, full.z0 + (nb[2][0] ? 1 : 0)), full.z1});
  }
  if (interior.x1 < interior.x0 || interior.y1 < interior.y0 || interior.z1 < interior.z0) interior = LBox{};
}

// Shell / interior split of a deep-tb unit whose exchange overlaps the rest of the pass (GpuSolver::tb_split). The
// neighbours need the w = (next pass depth) nodes next to each face with a neighbour (edges and corners included). In
// y and z the shell is made of whole rows / columns of the pass's tile grid (tile edge T ≥ w), so the shell boxes
// recompute nothing the interior also computes; a remainder row narrower than w is replaced by the w rows next to
// the face (its own one-row box: the core ends a row earlier). In z every cut lies an EVEN number of nodes from the
// box's first node (the remainder box is widened to keep it so), so every sub-box starts and — unless it ends at the
// rank's last node — ends on a whole 16-byte pair: the pair-tiled pass stores whole pairs and never writes a node of
// another box. In x the shell is w planes of the remaining (y, z) core (recomputing S − 1 planes at the seam).
// Boxes: the y border rows (whole x, whole z), the z border columns of the rows between (whole x), then the core's
// x-face slabs; the interior is the core between the x slabs. Slab ranks (neighbours in x only): the two x slabs.
inline void deep_split(const LBox& full, const bool nb[3][2], i64 w, i64 T, std::vector<LBox>& shells,
                       LBox& interior) {
  shells.clear();
  interior = full;
  // core range along a tiled axis: the border is the first / last tile row of the box, or — when the last row is a
  // remainder narrower than w — the w (z: w rounded to a whole pair from the box start) rows next to the face
  auto grid = [&](i64 b0, i64 b1, bool lo, bool hi, bool pair, i64& c0, i64& c1) {
    const i64 nt = ceil_div(b1 - b0, T), rem = (b1 - b0) - (nt - 1) * T;
    c0 = lo ? imin(b0 + T, b1) : b0;
    i64 cut = rem >= w ? b0 + (nt - 1) * T : b1 - w;
    if (pair) cut = b0 + ((cut - b0) & ~i64{1});
    c1 = hi ? imax(cut, c0) : b1;
  };
  i64 ya, yb, za, zb;
  grid(full.y0, full.y1, nb[1][0], nb[1][1], false, ya, yb);
  grid(full.z0, full.z1, nb[2][0], nb[2][1], true, za, zb);
  auto add = [&](const LBox& b) {
    if (!b.empty()) shells.push_back(b);
  };
  add(LBox{full.x0, full.x1, full.y0, ya, full.z0, full.z1});
  add(LBox{full.x0, full.x1, yb, full.y1, full.z0, full.z1});
  add(LBox{full.x0, full.x1, ya, yb, full.z0, za});
  add(LBox{full.x0, full.x1, ya, yb, zb, full.z1});
  interior = LBox{full.x0, full.x1, ya, yb, za, zb};
  if (interior.empty()) {
    interior = LBox{};
    return;
  }
  if (nb[0][0]) {
    add(LBox{full.x0, imin(full.x0 + w, full.x1), ya, yb, za, zb});
    interior.x0 = imin(full.x0 + w, full.x1);
  }
  if (nb[0][1]) {
    const i64 x = imax(full.x1 - w, interior.x0);
    add(LBox{x, full.x1, ya, yb, za, zb});
    interior.x1 = x;
  }
}

// Resume / loaded-field start: the rank's padded local array (owned nodes and every ghost layer that lies inside the
// domain; ghosts beyond the global boundary and the row padding 0) from a GLOBAL (N+1)³ C-order field. With ghosts
// of any depth filled from the global field, the first pass after a resume needs no halo exchange.
void global_to_local(const Layout& l, const double* global, double* local);

// User-supplied initial data (set_initial): the layout φ / ψ are sliced into — the rank's box with one ghost layer more
// than the solve layout on every axis, so the first step can be evaluated on every ghost node of the solve layout —
// and the slicing itself: global_to_local, then exact zeros on the six global faces (their values are ignored).
inline Layout initial_layout(const Problem& p, const Layout& solve) {
  const Box b{solve.gx0, solve.gx0 + solve.nx, solve.gy0, solve.gy0 + solve.ny, solve.gz0, solve.gz0 + solve.nz};
  return make_layout(p, b, 16, solve.xg + 1, solve.yg + 1, solve.zg + 1);
}
void initial_to_local(const Layout& src, const double* global, double* local);

// The eigenmode φ = (s_x·s_y)·s_z (stencil.hpp phi: cpu_init_first's u⁰) as a local array in `src` = initial_layout(...),
// zeros outside the global grid: what a solve with a speed field and no set_initial starts from.
std::vector<double> eigenmode_local(const Problem& p, const Layout& src);

// Variable wave speed u_tt = c²(x)·Δu: c is a GLOBAL (N+1)³ C-order field, face values ignored. speed_to_local checks
// every global interior value (finite and > 0, otherwise refused with "speed:"), returns their minimum and maximum, and
// fills two local arrays in the layout `l`, ghost layers included: c2[p] = c·c and lamf[p] = Coeffs::lam·c2[p], one
// rounding each, both exact zeros on and outside the global boundary and in the padding (either pointer may be null).
// The update then is stencil.hpp leapfrog(cur, old, s, lamf[p]) and the first step first_step(φ, s, 0.5·lamf[p]): with
// c ≡ 1 lamf[p] == Coeffs::lam and every bit is the constant-speed solve's. speed_cfl refuses courant()·max c > 1
// unless `force`.
struct SpeedRange {
  double cmin = 0.0, cmax = 0.0;
};
SpeedRange speed_to_local(const Problem& p, const Layout& l, const double* c_global, double* lamf, double* c2);
void speed_cfl(const Problem& p, const SpeedRange& r, bool force);


// Error accumulator: L∞ and Σe² over the updated (interior) nodes.
struct ErrAcc {
  double max = 0.0;
  double sum = 0.0;
};

// Set the OpenMP thread count (<=0 keeps the runtime default). Returns the effective count.
int cpu_set_threads(int n);
int cpu_max_threads();

// u0 = φ and u1 = u0 + τ²/2 Δ_h u0 over the whole local allocation, ghosts included (they are analytic, so no halo
// exchange is needed before the first leapfrog step). `s` = &sin_table_ext[1].
void cpu_init_first(const Layout& l, const Coeffs& c, const double* s, double* u0, double* u1);

// First step from stored initial data: u0 = φ and u1 = φ + τψ + (τ²/2)Δ_h φ (stencil.hpp first_step, first_step_psi;
// psi = nullptr: ψ = 0, its term skipped) over the whole allocation of the solve layout `l`, ghosts included; zeros on
// and outside the global boundary and in the padding. phi / psi: local arrays in `src` = initial_layout(...), filled
// by initial_to_local. With ψ absent and φ the eigenmode array, u1 equals cpu_init_first's bit for bit.
// lamf != nullptr (a speed field, layout `l`): the node's coefficient is 0.5·lamf[p] (exact) instead of Coeffs::half_lam.
// Coeffs::order = 4: Δ_h is the fourth-order operator (stencil.hpp d4sum_t) with the odd reflection at nodes 1 and N − 1.
void cpu_first_step_field(const Layout& l, const Layout& src, const Coeffs& c, double tau, const double* phi,
                          const double* psi, double* u0, double* u1, const double* lamf = nullptr);

// Discrete energy of two stored levels a = u^n, b = u^{n+1} (leapfrog conserves it exactly in exact arithmetic):
//   E^{n+1/2} = V/2 · [ Σ ((b − a)/τ)² + Σ_d (1/h_d²) Σ_{edges (p,q) along d} (b_p − b_q)(a_p − a_q) ],  V = hx·hy·hz,
// every grid edge counted once, by its lower endpoint, over the owned nodes of `l` (boundary nodes hold 0). Per node:
// kinetic ((b − a)·(1/τ))², potential ((b_x+ − b)(a_x+ − a))·ihx2 + ((b_y+ − b)(a_y+ − a))·ihy2 + ((b_z+ − b)(a_z+ − a))·ihz2
// — k_energy evaluates the same expressions, so the two differ by their summation order alone. Plain fixed loop order:
// one accumulator per z row, the rows of a plane added in y order, the planes in x order (the same bits for every
// thread count); depth = the additions on the longest path, nz + ny + nx.
struct EnergySums {
  double kin = 0.0, pot = 0.0;  // Σ kinetic terms, Σ potential terms (unscaled)
  double abs = 0.0;             // Σ |kinetic term| + Σ |each edge product|: the scale of the summation error
  i64 depth = 0;
};
// c2 != nullptr (a speed field, layout `l`): the conserved quantity carries the mass weight, kinetic term
// ((b − a)·(1/τ))² / c2[p] at every node with c2[p] > 0 (the global interior; elsewhere b − a = 0); the potential term is
// unchanged. c2 == nullptr: the code path and its bits are what they were.
EnergySums cpu_energy(const Layout& l, const Coeffs& c, double tau, const double* a, const double* b,
                      const double* c2 = nullptr);
inline double energy_value(const Problem& p, double kin, double pot) {
  return (0.5 * ((p.hx() * p.hy()) * p.hz())) * (kin + pot);
}

// u^{n+1} = 2u^n − u^{n−1} + τ²Δ_h u^n on `box`, written in place over u^{n−1} (`old_out`).
// If acc != nullptr also accumulates the error vs the analytic solution φ·ct over the box.
// sponge != nullptr: the damped update (stencil.hpp leapfrog_damped) with the node's g = max, r = min of the three 1-D
// tables (problem.hpp sponge_tables; global indices); a node with g = 0 gets the undamped bits.
// lamf != nullptr: a speed field (speed_to_local, layout `l`) — the coefficient of node p is lamf[p] instead of Coeffs::lam.
// Coeffs::order = 4: the fourth-order operator (stencil.hpp d4sum_t; a layout that spans the domain, no sponge, no lamf).
// A neighbour at distance 2 of node 1 / N − 1 of an axis is the odd reflection −u, never a load: the ghost layer is not read.
void cpu_leapfrog(const Layout& l, const Coeffs& c, const double* cur, double* old_out, const LBox& box,
                  const double* s, double ct, ErrAcc* acc, const SpongeView* sponge = nullptr,
                  const double* lamf = nullptr);

// Fourth order in time (Coeffs::time_order = 4, which needs order = 4; stencil.hpp leapfrog_t4): a step applies the
// fourth-order operator twice, through a third field v in the solve layout that spans the domain.
//   cpu_lap4:        v = lam·s(u) (lap_t4) on the nodes of `box` (inside the global interior); nothing else of v is
//                    written. The caller keeps v's six faces at exact zeros (a zeroed array that only this writes).
//   cpu_leapfrog44:  u^{n+1} = leapfrog_t4(u^n, u^{n−1}, v, s(v), lam12) in place over u^{n−1}; v over the WHOLE interior
//                    must be cpu_lap4's of `cur`. The error check is cpu_leapfrog's.
//   cpu_first_step_t4: u⁰ = φ everywhere (as cpu_first_step_field stores it), u¹ on the interior by first_step_t4 /
//                    first_step_t4_psi; ψ's operator takes ψ from the source layout; v is scratch (left = lam·s(φ)).
// A distance-2 neighbour outside the domain is −centre in both applications; no ghost layer is read.
void cpu_lap4(const Layout& l, const Coeffs& c, const double* u, double* v, const LBox& box);
void cpu_leapfrog44(const Layout& l, const Coeffs& c, const double* cur, const double* v, double* old_out, const LBox& box,
                    const double* s, double ct, ErrAcc* acc);
void cpu_first_step_t4(const Layout& l, const Layout& src, const Coeffs& c, double tau, const double* phi,
                       const double* psi, double* v, double* u0, double* u1);

// Sponge layers and the fused passes. An undamped pass of `steps` steps from damped levels u^{n−1}, u^n differs from
// the damped one only within reach of the layers: u^{n+steps} on the slabs d < W + steps − 1 from each damped face (d:
// nodes from the face), u^{n+steps−1} on d < W + steps − 2. sponge_boxes returns disjoint local boxes whose union is
// exactly the union of the slabs d < W + steps − 1, clipped to the interior, with opposite slabs merged where they
// meet; cut as shell_split cuts: x slabs whole, y slabs inside the remaining x range, z slabs inside both (≤ 6 boxes).
// reach = W + steps − 1 for the default; sponge_reach_boxes takes the reach itself.
inline std::vector<LBox> sponge_reach_boxes(const Problem& p, const Layout& l, i64 reach) {
  std::vector<LBox> out;
  if (!p.sponge.on() || reach <= 0) return out;
  const i64 N = p.N;
  // per axis: the damped intervals [a0, a1) ∪ [b0, b1) of global nodes and the interval [c0, c1) between them
  i64 iv[3][2][2], mid[3][2];
  for (int a = 0; a < 3; ++a) {
    const bool lo = (p.sponge.faces >> (2 * a)) & 1, hi = (p.sponge.faces >> (2 * a + 1)) & 1;
    i64 a1 = lo ? imin(reach, N) : 1;       // low slab: nodes 1 .. reach − 1
    i64 b0 = hi ? imax(N - reach + 1, 1) : N;  // high slab: nodes N − reach + 1 .. N − 1
    if (lo && hi && a1 >= b0) {  // the two slabs meet: one interval
      a1 = N;
      b0 = N;
    }
    b0 = imax(b0, a1);
    iv[a][0][0] = 1;
    iv[a][0][1] = a1;
    iv[a][1][0] = b0;
    iv[a][1][1] = N;
    mid[a][0] = a1;
    mid[a][1] = b0;
  }
  const i64 g0[3] = {l.gx0, l.gy0, l.gz0};
  auto push = [&](const i64 r[3][2]) {
    const LBox b{r[0][0] - g0[0], r[0][1] - g0[0], r[1][0] - g0[1], r[1][1] - g0[1], r[2][0] - g0[2], r[2][1] - g0[2]};
    if (!b.empty()) out.push_back(b);
  };
  for (int a = 0; a < 3; ++a)
    for (int side = 0; side < 2; ++side) {
      i64 r[3][2];
      for (int b = 0; b < 3; ++b) {
        // earlier axes: the range their slabs left; this axis: the slab; later axes: the whole interior
        r[b][0] = b < a ? mid[b][0] : (b == a ? iv[a][side][0] : 1);
        r[b][1] = b < a ? mid[b][1] : (b == a ? iv[a][side][1] : N);
      }
      push(r);
    }
  return out;
}
inline std::vector<LBox> sponge_boxes(const Problem& p, const Layout& l, int steps) {
  return sponge_reach_boxes(p, l, static_cast<i64>(p.sponge.width) + steps - 1);
}

// Point sources u_tt = Δu + Σ_q w_q(t) δ(x − x_q), δ discretised as 1/(hx·hy·hz) at the node: the addend of sample w at
// a source node is a = τ²·w / (hx·hy·hz), evaluated by this one expression on every backend. The first level gets ½·a⁰
// (the first step is a half step), level m + 1 gets a^m.
inline double source_addend(const Problem& p, double w) { return ((p.tau * p.tau) * w) / ((p.hx() * p.hy()) * p.hz()); }
// Validates a source list (Q global nodes strictly inside the grid, w[K][Q] finite; refusals start with "sources:") and
// returns the scaled addends a[K][Q].
std::vector<double> source_addends(const Problem& p, const i64* ijk, int Q, const double* w);

// Response of a ZERO field to one source over a pass of s = 1..5 steps n → n + s (the leapfrog update is linear, so a
// forced pass = the unforced pass + this): from r^{n−1} = r^n = 0, step k = 1..s advances with d2sum_t / leapfrog in
// cpu_leapfrog's argument order and then adds a[k − 1] at `node` (first_is_start: the pass is the start, s = 1, and the
// addend is ½·a[0]). out_last = r^{n+s}, out_prev = r^{n+s−1} on the kSourceSide³ cube around the node, C order, cell
// (i, j, k) = node + (i, j, k) − kSourceRadius; non-zero only within L1 distance s − 1 / s − 2 of the node, and nodes on
// or outside the global boundary stay +0.0. The bit-exact oracle of k_source_cone.
constexpr int kSourceMaxSteps = 5;
constexpr int kSourceRadius = kSourceMaxSteps;
constexpr int kSourceSide = 2 * kSourceRadius + 1;
constexpr int kSourceCells = kSourceSide * kSourceSide * kSourceSide;
void cpu_source_response(const Problem& p, const Coeffs& c, const i64 node[3], const double* a, bool first_is_start, int s,
                         double* out_last, double* out_prev);

// Error of a stored field vs φ·ct over `box` (used for step 1 and for the standalone error check).
void cpu_error(const Layout& l, const double* u, const LBox& box, const double* s, double ct, ErrAcc* acc);

// Pack / unpack one y or z face between the field and a contiguous buffer (x faces are contiguous already).
void cpu_pack_face(const Layout& l, const Face& f, const double* u, double* buf);
void cpu_unpack_face(const Layout& l, const Face& f, const double* buf, double* u);

}  // namespace wave3d

// ------------------------------------------------------------------------------------------------------------------
// Whole-domain CPU solver (the reference's sequential `wave` / OpenMP `wave3dOMP` programs).
// ------------------------------------------------------------------------------------------------------------------
#include <vector>

namespace wave3d {

struct CpuResult {
  std::vector<int> steps;
  std::vector<double> max_err, rms_err;
  double solve_s = 0.0, init_s = 0.0, compute_s = 0.0, check_s = 0.0;
  // the reference's CPU phase columns (report.pdf p.16): boundary = halo faces packed / unpacked,
  // exchange = waiting for the neighbours (and the final error reduction); ranks: each the max over ranks
  double boundary_s = 0.0, exchange_s = 0.0;
  // the slowest rank's own init / compute / boundary / exchange (they add up to its solve time; the per-phase maxima
  // above come from different ranks and overlap in time)
  double slow_phases[4] = {0.0, 0.0, 0.0, 0.0};
  bool finite = true;
};

class CpuSolver {
 public:
  CpuSolver(const Problem& p, int check_every = 2, int threads = 0);
  CpuResult run();
  // Problem::order = 4: every step uses the fourth-order operator, the start (eigenmode or set_initial) goes through
  // cpu_first_step_field; a box, receivers and sources work as before. Refused with messages starting "order:": a sponge
  // (Problem::validate), set_speed, energy / energy_sums, set_state.
  // Problem::time_order = 4 (with order = 4): every step is cpu_lap4 + cpu_leapfrog44, the start cpu_first_step_t4;
  // receivers work as before. Refused with "time_order:": set_sources (the forcing's τ⁴ terms are a follow-up).
  // With Problem::sponge set every step is the damped one (stencil.hpp leapfrog_damped); the start levels, set_initial,
  // set_state, receivers, sources (added after the damped step, as after the plain one) and energy work as before. The
  // error columns then have no meaning, and the energy decays.
  // Start every following run() at step n0 from u^{n0−1} = prev and u^{n0} = cur (global (N+1)³ fields) instead of
  // the analytic initial condition: the leapfrog continues to K and checks the steps after n0.
  void set_state(const double* prev_global, const double* cur_global, int n0);
  // Start every following run() from user-supplied initial data φ = u(·,0), ψ = u_t(·,0) (global (N+1)³ fields, face
  // values ignored; psi_global = nullptr: ψ = 0): u⁰, u¹ by cpu_first_step_field, then the ordinary steps from n = 1.
  // The error columns then are the difference from the eigenmode. It and set_state replace each other.
  void set_initial(const double* phi_global, const double* psi_global);
  // Variable wave speed: every following run() solves u_tt = c²(x)·Δu with c a global (N+1)³ field (speed_to_local; face
  // values ignored, interior values finite and > 0; courant()·max c ≤ 1 unless `force`). nullptr clears it. The update
  // takes its coefficient from lamf[p]; without set_initial the start is the eigenmode array through the first-step-field
  // path (cpu_init_first's u⁰, and its u¹ where c = 1). Sources, receivers, sponge layers and set_state work as before;
  // the error columns then mean nothing, and energy() carries the mass weight 1/c².
  void set_speed(const double* c_global, bool force = false);
  bool speed() const { return !lamf_.empty(); }
  SpeedRange speed_range() const { return speed_range_; }
  // Receivers: R global nodes (ijk: R triples, each index in 0..N; duplicates allowed) whose value every following run()
  // reads from the stored field after the start and after every cpu_leapfrog step — the plain definition, the oracle
  // of the GPU record kernels. R = 0 removes them. traces(): the last run()'s (K+1) × R values, row n = u^n (NaN in the
  // rows below n0 − 1 of a resumed run).
  void set_receivers(const i64* ijk, int R);
  const std::vector<double>& traces() const { return traces_; }
  int receivers() const { return static_cast<int>(recv_off_.size()); }
  // Point sources: Q global nodes strictly inside the grid (ijk: Q triples; a node listed twice is added twice) and the
  // wavelet samples w[K][Q], row m = w_q(m·τ). Every following run() adds, in list order, ½·a_q⁰ to u¹[x_q] after the
  // start levels are stored, and a_q^m to u^{m+1}[x_q] after the plain leapfrog step m → m + 1 (m ≥ 1), with a =
  // source_addend(w) — the plain definition, the oracle of the GPU source kernel. The error columns of the log then have
  // no meaning (the eigenmode is no longer the solution). Q = 0 removes the sources. Not together with set_state.
  void set_sources(const i64* ijk, int Q, const double* w);
  int sources() const { return static_cast<int>(src_off_.size()); }
  // E^{K−1/2} of the last run()'s u^{K−1}, u^K (which = 0), or E^{1/2} of its u⁰, u¹ (which = 1; after set_initial)
  double energy(int which) const;
  // the sums behind energy(which): kin, pot, abs (the error scale) and the summation depth
  EnergySums energy_sums(int which) const;
  // u^K (which = 0) or u^{K-1} (which = 1), padded local layout (single rank = whole domain).
  const std::vector<double>& field(int which) const { return which == 0 ? u_[final_] : u_[1 - final_]; }
  const Layout& layout() const { return lay_; }
  const Problem& problem() const { return prob_; }
  std::vector<int> check_steps() const;

 private:
  Problem prob_;
  int check_every_;
  Layout lay_;
  std::vector<double> u_[2];
  std::vector<double> v_;                // time order 4: τ²L_h u^n (zeros outside the interior); empty otherwise
  std::vector<double> s_;
  SpongeTables sponge_;                  // Problem::sponge's coefficient tables (empty: no sponge)
  int final_ = 1;
  int resume_n_ = 0;                     // > 0: start step of a resumed run
  std::vector<double> resume_[2];        // local u^{n0−1}, u^{n0}
  bool initial_ = false;                 // set_initial: runs start from init_[0] = φ, init_[1] = ψ (empty: none)
  Layout init_lay_;
  std::vector<double> init_[2];
  EnergySums e_start_;                   // of u⁰, u¹ of the last run() after set_initial
  std::vector<double> lamf_, c2_;        // set_speed: lam·c² and c² in lay_ (empty: constant speed 1)
  SpeedRange speed_range_;
  std::vector<i64> recv_off_;            // receivers: Layout::off of each node
  std::vector<double> traces_;           // [K + 1][R] of the last run()
  std::vector<i64> src_off_;             // sources: Layout::off of each node ...
  std::vector<double> src_a_;            // ... and the scaled addends a[K][Q]
  int runs_ = 0;
};

}  // namespace wave3d
