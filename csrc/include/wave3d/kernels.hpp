// Hand-written CDNA4 (gfx950) HIP kernels: launch interface.
//
//   k_init_first  : u⁰ = φ and u¹ = u⁰ + τ²/2·Δ_h u⁰ in one write-only pass (16 B/node), ghosts included
//                   (reference kernels K1 + K2).
//   k_leapfrog    : the hot loop — 2.5-D tiled 7-point leapfrog, x-marching register queue, LDS-staged (y,z) tile,
//                   16-byte node pairs, in place over u^{n−1}, Dirichlet BC by construction, optional fused error
//                   epilogue (reference kernels K3 + K4 + K5).
//   k_reduce      : fixed-order reduction of per-block error partials (deterministic).
//   k_pack/unpack : strided y/z halo faces ↔ contiguous RCCL staging buffers (reference kernel K6).
#pragma once

#include <vector>

#include <hip/hip_runtime.h>

#include "wave3d/cpu.hpp"
#include "wave3d/decomp.hpp"
#include "wave3d/deep_plan.hpp"
#include "wave3d/problem.hpp"
#include "wave3d/schedule.hpp"
#include "wave3d/tiling.hpp"

namespace wave3d {

// Error partial: x = L∞ candidate, y = Σe².
using Partial = double2;

// Number of error partials (v0: workgroups, v1: waves) a leapfrog launch over `boxes` writes.
int leapfrog_blocks(const Layout& l, const LBox* boxes, int nbox, const LeapfrogTiling& t);

void launch_init_first(const Layout& l, const Coeffs& c, const double* d_s, double* u0, double* u1,
                       hipStream_t stream);

// u¹ and u² (the first leapfrog step) computed analytically from φ in one write-only pass, ghosts included:
// bit-identical to launch_init_first followed by one launch_leapfrog over the whole interior. With `partials`
// the error of u² vs φ·ct2 over the owned interior is reduced per workgroup (init_two_partials() of them).
int init_two_partials(const Layout& l);
void launch_init_two(const Layout& l, const Coeffs& c, const double* d_s, double* u1, double* u2, double ct2,
                     Partial* partials, hipStream_t stream);

// First step from stored initial data (kernels_initial.hip): u⁰ = φ, u¹ = φ + τψ + (τ²/2)Δ_h φ (stencil.hpp
// first_step / first_step_psi; psi = nullptr: ψ = 0, the term is skipped) over the WHOLE solve layout `l` — owned and
// ghost nodes, exact zeros on and outside the global boundary, in the padding and the zero slot. phi / psi are device
// buffers in `src` = make_layout(prob, box, 16, l.xg + 1, l.yg + 1, l.zg + 1) filled by initial_to_local (cpu.hpp).
// lamf != nullptr (a speed field, cpu.hpp speed_to_local: device array in layout `l`): the VARC instantiation, the node's
// coefficient is 0.5·lamf[p] — bit-identical to cpu_first_step_field with the same array.
// Coeffs::order = 4: the ORDER4 instantiation (d4sum_t, −centre for a distance-2 neighbour outside the grid; no lamf).
void launch_first_step_field(const Layout& l, const Layout& src, const Coeffs& c, double tau, const double* phi,
                             const double* psi, double* u0, double* u1, hipStream_t stream, const double* lamf = nullptr);

// Discrete energy of two stored levels a = u^n, b = u^{n+1} over the owned nodes of `l` (cpu.hpp cpu_energy has the
// formula; edges to the upper neighbours read the ghost layer, so the fields must be valid there: one rank, or fresh
// ghosts). launch_energy writes energy_partials(l) partials (x: kinetic sum, y: potential sum), launch_energy_reduce
// adds them in a fixed order into out[0]; E = energy_value(problem, out[0].x, out[0].y). energy_depth(l): the depth D
// of that reduction tree (kernels_initial.hip, k_energy's header).
int energy_partials(const Layout& l);
int energy_depth(const Layout& l);
void launch_energy(const Layout& l, const Coeffs& c, double tau, const double* a, const double* b, Partial* partials,
                   hipStream_t stream);
void launch_energy_reduce(const Partial* partials, int n, Partial* out, hipStream_t stream);

// Receivers (kernels_record.hip; schedule.hpp Receiver / plan_receivers). `table`: `count` receivers in device memory;
// `trace`: rows of `rtotal` doubles, row m = level u^m, a receiver's column = its `slot`.
//   launch_record_cone   : the levels u^{n+1} .. u^{n+steps} (steps = 2..5) at every receiver of the table, recomputed
//                          from the inputs prev = u^{n−1}, cur = u^n of a pass of `steps` steps on layout l — read on the
//                          L1 ball of radius steps (cur) / steps − 1 (prev) around the receiver, never on or outside the
//                          global boundary; bit-identical to `steps` cpu_leapfrog steps. Receivers on a global face get
//                          +0.0. Needs ghosts `steps` deep on every axis the rank does not span.
//   launch_record_gather : row n from a stored level: trace[n][slot] = field[off].
void launch_record_cone(const Layout& l, const Coeffs& c, const double* prev, const double* cur, int n, int steps,
                        const Receiver* table, int count, double* trace, i64 rtotal, hipStream_t stream);
void launch_record_gather(const double* field, int n, const Receiver* table, int count, double* trace, i64 rtotal,
                          hipStream_t stream);

// Point sources (kernels_source.hip; schedule.hpp Source / plan_sources; the oracle: cpu.hpp cpu_source_response).
// Adds the response of a zero field to the forcing of a pass n → n + steps (steps = 1..5) to the pass's stored outputs:
// out_last (u^{n+steps}) on the L1 ball of radius steps − 1 around every source of `table`, out_prev (u^{n+steps−1}) on
// radius steps − 2 — on the nodes inside the global interior and inside the allocation of layout l (ghost layers
// included; the source node itself may lie outside it), nothing else is addressed. `a`: device array [K][Q] of scaled
// addends (cpu.hpp source_addend), column = Source::slot; step k adds a[n + k − 1]. start: the start level (n = 0,
// steps = 1): out_last = u¹ gets ½·a[0]. One launch per colour class, in class order: class c = table[class_begin[c] ..
// class_begin[c + 1]) (class_begin: host array of classes + 1 entries); the balls of a class are disjoint, so the
// adds are plain loads and stores. With rcount > 0 (not for the start) level n + k's response at every receiver of
// `rtable` within distance k − 1 of a source is added to trace[n + k][slot], k = 1..steps. Needs ghosts `steps` deep on
// every axis the rank does not span; a null out_prev is refused.
void launch_source_cone(const Layout& l, const Coeffs& c, double* out_prev, double* out_last, int n, int steps, bool start,
                        const Source* table, const int* class_begin, int classes, const double* a, i64 Q,
                        const Receiver* rtable, int rcount, double* trace, i64 rtotal, hipStream_t stream);

// Runs one leapfrog step over up to 6 boxes in a single launch. If `partials` is non-null the error vs φ·ct is reduced
// per workgroup into partials[0 .. leapfrog_blocks()).
// sponge != nullptr: the damped step of the sponge layers (the DAMP instantiations; the tables live in device memory,
// problem.hpp SpongeView); bit-identical to cpu_leapfrog with the same tables.
// lamf != nullptr: a speed field (cpu.hpp speed_to_local; device array in layout `l`): the VARC instantiations, which
// load the thread's lamf pair one plane ahead with the plane's other loads (32 instead of 24 bytes per node);
// bit-identical to cpu_leapfrog with the same array. Not with 8 rows per wave; with a sponge at 1 or 2 rows (and the LDS
// variant) only — leapfrog_speed_supported says which, launch_leapfrog refuses the rest.
bool leapfrog_speed_supported(const LeapfrogTiling& t, bool sponge);
void launch_leapfrog(const Layout& l, const Coeffs& c, const double* cur, double* old_out, const LBox* boxes, int nbox,
                     const double* d_s, double ct, Partial* partials, const LeapfrogTiling& t, hipStream_t stream,
                     const SpongeView* sponge = nullptr, const double* lamf = nullptr);

// The fourth-order single step (kernels_stencil4.hip, k_leapfrog4; Problem::order = 4, Coeffs::order = 4 whose lam carries
// the 1/12): launch_leapfrog's contract — up to 6 boxes inside the global interior in one launch, in place over u^{n−1},
// partials per workgroup in launch order (leapfrog4_blocks of them) — on one rank's layout that spans the whole domain.
// Bit-identical to cpu_leapfrog with the same coefficients. Its tile is leapfrog4_ty(t) = 8 or 16 rows (t.ty below 16:
// 8; four rows have fewer threads than halo slots); t.variant / t.rows are not looked at. min_chunk: the fewest planes
// of an x chunk (each chunk re-reads four planes). The ghost layer, the row padding and the planes outside the grid are
// never used as data: the distance-2 neighbour of node 1 / N − 1 is −centre.
int leapfrog4_ty(const LeapfrogTiling& t);
int leapfrog4_blocks(const Layout& l, const LBox* boxes, int nbox, const LeapfrogTiling& t, int min_chunk = 16);
void launch_leapfrog4(const Layout& l, const Coeffs& c, const double* cur, double* old_out, const LBox* boxes, int nbox,
                      const double* d_s, double ct, Partial* partials, const LeapfrogTiling& t, hipStream_t stream,
                      int min_chunk = 16);

// Fourth order in time (kernels_stencil44.hip; Problem::time_order = 4, Coeffs of such a problem): a step is two launches
// with launch_leapfrog4's contract (boxes, tiling, min_chunk, one rank's layout that spans the domain).
//   launch_lap4:       k_lap4, v = lam·s(u) on the interior nodes of the boxes and nothing else — bit-identical to cpu_lap4.
//                      v's six faces must hold exact zeros (a buffer zeroed once that only this writes).
//   launch_leapfrog44: k_leapfrog44, u^{n+1} = leapfrog_t4(u^n, u^{n−1}, v, s(v), lam12) in place over u^{n−1}, with v =
//                      launch_lap4's of `cur` over the whole interior; partials as launch_leapfrog4 (leapfrog44_blocks of
//                      them). Bit-identical to cpu_leapfrog44.
//   launch_first_step_t4: u⁰ = φ, v = lam·s(φ), u¹ by first_step_t4 / first_step_t4_psi (k_first_step_field for u⁰, k_lap4,
//                      k_first_step_t4) — bit-identical to cpu_first_step_t4; φ, ψ as launch_first_step_field takes them.
// The ghost layer, the row padding and the planes outside the grid of u, u^{n−1} and v are never used as data.
int leapfrog44_blocks(const Layout& l, const LBox* boxes, int nbox, const LeapfrogTiling& t, int min_chunk = 16);
void launch_lap4(const Layout& l, const Coeffs& c, const double* u, double* v, const LBox* boxes, int nbox,
                 const LeapfrogTiling& t, hipStream_t stream, int min_chunk = 16);
void launch_leapfrog44(const Layout& l, const Coeffs& c, const double* cur, const double* v, double* old_out,
                       const LBox* boxes, int nbox, const double* d_s, double ct, Partial* partials,
                       const LeapfrogTiling& t, hipStream_t stream, int min_chunk = 16);
void launch_first_step_t4(const Layout& l, const Layout& src, const Coeffs& c, double tau, const double* phi,
                          const double* psi, double* v, double* u0, double* u1, const LeapfrogTiling& t,
                          hipStream_t stream);

// Sponge layers on the fused schedule (kernels_sponge.hip). An LDS pass of `steps` steps runs undamped; its two stored
// outputs differ from the damped levels only on the slabs cpu.hpp sponge_boxes returns, which this recomputes from the
// pass's INPUTS prev = u^{n−1}, cur = u^n with the damped operator: it writes out2 = u^{n+steps} and out1 =
// u^{n+steps−1} on `box` (steps = 2..5), bit-identical to `steps` damped cpu_leapfrog steps. It reads the inputs on `box`
// grown by `steps` and clipped to the domain, never addresses a node on or outside the global boundary (those count
// as +0.0) and writes nothing outside `box`. One rank that spans the whole domain; four distinct buffers; `tables` in
// device memory. sponge_box_prepare raises the kernels' dynamic-LDS limit (call before capturing a launch).
void sponge_box_prepare();
void launch_sponge_box(const Layout& l, const Coeffs& c, const SpongeView& tables, const double* prev, const double* cur,
                       double* out1, double* out2, const LBox& box, int steps, hipStream_t stream);

// Temporal blocking: TWO leapfrog steps in one pass over HBM (u^{n+1}, u^{n+2} from u^{n−1}, u^n), 16 instead of
// 24 compulsory bytes per node-step. Needs every node of `box` to be updatable without a halo exchange (single rank:
// box = the whole global interior) and four distinct buffers (the redundant halo rows of step 1 read u^{n−1} that a
// neighbouring wave may not yet have consumed, so nothing is overwritten in place). If `partials` is non-null the
// error of u^{n+2} vs φ·ct2 is reduced per wave.
// [sx0, sx1): local x range where stage-1 (u^{n+1}) values are real; it extends one plane beyond `box` towards a
// neighbouring rank of a slab decomposition (those ghost planes are recomputed redundantly from 2-deep halos).
// Default (sx0 > sx1): this rank's updated region.
int leapfrog2_partials(const Layout& l, const LBox& box, const Leapfrog2Tiling& t);
void launch_leapfrog2(const Layout& l, const Coeffs& c, const double* prev, const double* cur, double* out1,
                      double* out2, const LBox& box, const double* d_s, double ct2, Partial* partials,
                      const Leapfrog2Tiling& t, hipStream_t stream, i64 sx0 = 1, i64 sx1 = 0, const double* lamf = nullptr);
// (lamf != nullptr: a speed field in layout `l` — both stages, the recomputed halo rows and the spare z lanes read lamf at
// their own node: 20 instead of 16 bytes per node-step; bit-identical to two cpu_leapfrog steps with the same array)

// Deep temporal blocking: S = 2..4 leapfrog steps in one pass, all intermediate levels in LDS (32 × 32 (y,z) tiles
// marching in x (or in x chunks when the tiles alone do not fill the GPU), one workgroup per CU). Reads u^{n−1}, u^n;
// writes u^{n+S−1} into out1 and u^{n+S} into out2: 32/S compulsory bytes per node-step. Same preconditions as
// launch_leapfrog2 with S−1 stage-1 planes beyond the box. The launch arguments: PassArgs below.
//
// Slab peer-push transport of an LDS pass (x faces only; every slab rank has the same plane geometry, so a plane's
// in-plane offsets are the same on both sides). The pass
//   * marches the upper face segment [x1 − T, x1) first, then [x0, x1 − T) (faces_first), so both face regions are
//     produced at the start of the pass;
//   * stores u^{n+S} of planes [0, T) / [nx − T, nx) and u^{n+S−1} of planes [0, T−1) / [nx − T + 1, nx) a second time,
//     straight into the lower / upper neighbour's staging over xGMI (fwd2 / fwd1: the neighbour's staging plane 0 of
//     the matching side and pass parity; nullptr: no neighbour);
//   * reads its own ghost planes [−T, 0) / [nx, nx + T) of u^n and u^{n−1} from its staging (gcur / gprev, plane 0 =
//     ghost plane −T resp. nx) instead of the field buffers;
//   * waits (wait_epoch > 0) for both neighbours' flags to reach wait_epoch before its first load, and raises its slot
//     in both neighbours' flags (rflag) to signal_epoch once every workgroup's stores are visible (the workgroup that
//     brings `done` to done_target).
struct TbPush {
  int on = 0, faces_first = 0;
  int T = 0;                          // ghost depth (planes) = the deepest pass
  int nx = 0;                         // this rank's planes
  double* fwd1[2] = {nullptr, nullptr};        // [lo, hi] neighbour staging for u^{n+S−1}
  double* fwd2[2] = {nullptr, nullptr};        // ... for u^{n+S}
  const double* gprev[2] = {nullptr, nullptr}; // own staging holding the ghost planes of u^{n−1} [lo, hi]
  const double* gcur[2] = {nullptr, nullptr};  // ... of u^n
  unsigned* flags = nullptr;          // own flags: [0] raised by the lower neighbour, [1] by the upper
  unsigned* rflag[2] = {nullptr, nullptr};     // this rank's slot in the lower / upper neighbour's flags
  int wait_side[2] = {0, 0};
  unsigned wait_epoch = 0, signal_epoch = 0;
  unsigned cp_wait = 0;               // host side: epoch the command processor waits for before the launch (0: none)
  unsigned tag = 0;                   // integrity check: the kernel compares it with its argument (else status = 2)
  int acquire = 1;                    // system-scope acquire at the pass start (perf attribution only: 0)
  unsigned* done = nullptr;           // workgroups done (local counter, zeroed per solve)
  unsigned done_target = 0;
  unsigned* status = nullptr;         // set to 1 when a wait timed out
  unsigned long long spin_ticks = 0;  // wait bound (100 MHz wall clock)
};

// Fused z-face pack of a 3-D block pass that precedes an exchange: stages S−1 and S store the owned
// nodes of the two z-face message parts (deep_plan.hpp: direction (0, 0, ∓1), w = the next pass's depth deep for
// u^{n+S}, w − 1 for u^{n+S−1}) straight into the send staging next to their field store. The z faces are the strided
// ones — rows of w ≤ 4 doubles one pitch apart, which a pack kernel reads at a fraction of the copy rate; x / y faces,
// edges and corners are whole-row copies and stay with k_box_copy. Send-region nodes on the global boundary are never
// computed and never written: the receiving pass loads the zero slot for them, not their ghosts (kernel `ld`).
struct TbPack {
  double* zf[2][2] = {};  // [low / high z face][field 0: u^{n+S}, 1: u^{n+S−1}]: the part in the send staging (or null)
  int w = 0;              // band width of u^{n+S}; u^{n+S−1}: w − 1
  int ny = 0, nz = 0;     // owned box
};

// Write back and invalidate every XCD's L2 (and the L1s): enough workgroups to reach every CU each run a system-scope
// fence. Called once after allocating uncached buffers: lines of the same physical memory that a freed CACHED
// allocation left dirty in some L2 would otherwise be evicted over the new buffer's contents later (measured: an
// intermittent O(1) error in a fresh push staging after other solvers had been freed).
void l2_flush_all(hipStream_t stream);
// Raise the dynamic-LDS limit of every instantiation (call before capturing launches into a graph).
void leapfrog_tb_prepare(bool push = false);  // push: also the push-transport instantiations
size_t leapfrog_tb_lds_bytes(int stages);
int leapfrog_tb_partials(const Layout& l, const LBox& box, const LeapfrogTbTiling& t);

// What a launch of an LDS S-step pass (S = tiling.stages) takes besides the layout, the coefficients, its box or boxes
// and the stream.
struct PassArgs {
  const double *prev = nullptr, *cur = nullptr;  // u^{n−1}, u^n
  double *out1 = nullptr, *out2 = nullptr;       // u^{n+S−1}, u^{n+S}: four distinct buffers
  // (out1 = nullptr, the pair-tiled pass only: u^{n+S−1} is not stored — a solve's last pass, whose u^{K−1} GpuSolver
  // rebuilds on first use; out2 and the partials are what they are with out1 set. Not with tiling.ghost_x1.)
  const double* d_s = nullptr;                   // sin table, global index −1..N+1
  double ct[5] = {0, 0, 0, 0, 0};                // ct[k−1]: the time factor of u^{n+k}
  int check_mask = 0;            // bit k−1: error check of u^{n+k} ...
  Partial* partials = nullptr;   // ... whose partials go to partials + (k−1)·level_stride (nullptr: no check)
  int level_stride = 0;          // 0: the launch's block count (leapfrog_tb_partials())
  // > 0: a padded grid (several launches sharing one level's partial slots, each of grid_blocks entries): the extra
  // workgroups have no tile and write (0, 0) partials, so every slot entry a reduction reads is written
  int grid_blocks = 0;
  LeapfrogTbTiling tiling;
  LBox real = tb_default_real();  // stage-real ranges (tiling.hpp)
  // the pass starts at n = 1 from u⁰ = φ and u¹ computed in the kernel (init_first's formulas, bit-identical): prev /
  // cur are not read, it writes u^S, u^{S+1} with no HBM reads
  bool analytic_start = false;
  // a speed field (cpu.hpp speed_to_local; device array in layout `l`): the pair-tiled pass's VARC instantiations,
  // S = 2..kP2VarcMaxStages — every stage takes lamf[p] of its own node, 40/S instead of 32/S bytes per node-step,
  // bit-identical to S cpu_leapfrog steps with the same array. Refused ("speed: ...") with analytic_start, out1 = nullptr,
  // push or pack, and wherever the launch would not run on the pair-tiled kernel.
  const double* lamf = nullptr;
  // slab peer-push transport and fused z-face pack (k_leapfrog_tb only): the host copy, which the launcher reads, and
  // the same entry in device memory, which the kernel reads
  const TbPush *push = nullptr, *push_dev = nullptr;
  const TbPack *pack = nullptr, *pack_dev = nullptr;
};

// What both launchers fill alike in their kernel parameters (TbParams / P2Params: the field names agree), after the
// plan set p.nblocks: buffers from the plane the x ghosts start at, coefficients, check mask and partials,
// the grid padded to grid_blocks (xper stays the active blocks' per-XCD share: else the remap would hand every tile to
// the first XCDs — measured: a slab rank's 256 tiles on 4 of 8 XCDs, passes 2.2x slower). false: nothing to launch.
// (p.lamf where the parameters have one — P2Params; k_leapfrog_tb has no coefficient form and its launcher refuses one)
template <class Params>
auto set_pass_lamf(Params& p, const double* v, int) -> decltype(p.lamf = v, void()) {
  p.lamf = v;
}
template <class Params>
void set_pass_lamf(Params&, const double*, long) {}

template <class Params>
bool fill_pass_params(Params& p, const Layout& l, const Coeffs& c, const PassArgs& a, const char* name) {
  W3D_REQUIRE(a.out1 != a.out2 && (a.analytic_start || (a.prev != a.out1 && a.prev != a.out2 && a.cur != a.out1 &&
                                                         a.cur != a.out2)),
              std::string(name) + " needs four distinct buffers");
  if (p.nblocks == 0) return false;
  const LeapfrogTbTiling& t = a.tiling;
  if (a.grid_blocks > 0) {
    W3D_REQUIRE(a.grid_blocks >= p.nblocks && (!t.xcd_remap || a.grid_blocks % 8 == 0),
                std::string(name) + ": bad grid_blocks");
    p.nblocks = a.grid_blocks;
  }
  const i64 kb = (l.xg - 1) * l.plane;  // x base only: in-plane offsets are plane-relative (non-negative)
  p.prev = a.analytic_start ? nullptr : a.prev + kb;
  p.cur = a.analytic_start ? nullptr : a.cur + kb;
  p.out1 = a.out1 != nullptr ? a.out1 + kb : nullptr;
  p.out2 = a.out2 + kb;
  set_pass_lamf(p, a.lamf != nullptr ? a.lamf + kb : nullptr, 0);
  p.s = a.d_s;
  p.tau2 = c.lam;  // τ²/h² and τ²/(2h²): the coefficients of d2sum
  p.half_tau2 = c.half_lam;
  p.ry = c.ry;
  p.rz = c.rz;
  p.check_mask = a.partials != nullptr ? (a.check_mask & ((1 << t.stages) - 1)) : 0;
  p.partials = p.check_mask != 0 ? a.partials : nullptr;
  W3D_REQUIRE(a.level_stride == 0 || a.level_stride >= p.nblocks,
              std::string(name) + ": level stride below the block count");
  p.lstride = a.level_stride > 0 ? a.level_stride : p.nblocks;
  constexpr int nct = static_cast<int>(sizeof(p.ct) / sizeof(p.ct[0]));
  for (int k = 0; k < nct; ++k) p.ct[k] = k < t.stages ? a.ct[k] : 0.0;
  return true;
}

// Dispatches to the pair-tiled pass where pass_kernel (pass_grid.hpp) says so.
void launch_leapfrog_tb(const Layout& l, const Coeffs& c, const LBox& box, const PassArgs& a, hipStream_t stream);

// The pair-tiled S-step pass (kernels_leapfrog_p2.hip): the same contract as launch_leapfrog_tb for boxes inside the
// rank's y/z range that start and end on whole 16-byte pairs (leapfrog_p2_supported) and S = 2..5 (analytic start:
// 2..4); no push / fused pack. Up to kP2MaxBoxes boxes in ONE launch (one grid, the x-chunk target shared by work), for
// the overlapped schedules' shell boxes; their partials share one slot of `grid_blocks` entries.
int leapfrog_p2_partials(const Layout& l, const LBox& box, const LeapfrogTbTiling& t);
// (tests) the pair-tiled pass's thread → position table for S stages (kNT descriptors: (a+2) | (b+2)<<8 | lv<<16 |
// kind<<20) and its geometry {E, HY, HZ, PZ, tile, LDS bytes at xlen 512 (pass, analytic start), max xlen (same)}
std::vector<int> leapfrog_p2_table(int stages, std::vector<long>* geometry = nullptr);
void leapfrog_p2_prepare();
void launch_leapfrog_p2_boxes(const Layout& l, const Coeffs& c, const LBox* boxes, int nbox, const PassArgs& a,
                              hipStream_t stream);

// Error of a stored field vs φ·ct over `box` (step 1 / standalone check). Writes leapfrog-compatible partials and
// returns how many.
int error_blocks(const Layout& l, const LBox& box);
void launch_error(const Layout& l, const double* u, const LBox& box, const double* d_s, double ct, Partial* partials,
                  hipStream_t stream);

// out[0] = (max_i partials[i].x, Σ_i partials[i].y), in a fixed order.
void launch_reduce(const Partial* partials, int n, Partial* out, hipStream_t stream);
// Several independent reductions in one launch (one workgroup each, k_reduce's order: bit-identical results).
struct ReduceJob {
  const Partial* in;
  int n;
  Partial* out;
};
void launch_reduce_batch(const ReduceJob* jobs, int njobs, hipStream_t stream);

// S-deep exchange regions (deep_plan.hpp) <-> contiguous staging buffers. The job table is built once per plan and kept
// in device memory. mode 0: pack the send regions of u^{n+S} (u_s) and u^{n+S−1} (u_s1) into buf; 1: unpack buf into
// their receive (ghost) regions; 2: fill the receive regions with NaN (--poison-ghosts).
struct BoxJob {
  i64 buf;        // offset of the region in the staging buffer
  int count;      // nodes in the region
  int field;      // 0: u_s, 1: u_s1
  int x0, y0, z0; // first node (local)
  int ny, nz;     // extents of the region in y and z
  int blk0;       // first workgroup of this job
};
struct BoxCopyTable {
  BoxJob* jobs = nullptr;  // device
  int njobs = 0, nblocks = 0;
};
// skip_zfaces: leave out the parts of the pure z-face messages (direction (0, 0, ±1)): the pass packs them (TbPack)
BoxCopyTable make_box_copy_table(const DeepPlan& plan, bool recv_side, bool skip_zfaces = false);
void free_box_copy_table(BoxCopyTable& t);
void launch_box_copy(const Layout& l, const BoxCopyTable& t, int mode, double* u_s, double* u_s1, double* buf,
                     hipStream_t stream);

// Cross-rank flag words (copy-engine transport): one launch first waits until every word of `wait` equals wait.value
// (bounded by wait.ticks; a timeout sets *wait.status = 1), then stores signal.value into every word of `signal`.
struct FlagOp {
  static constexpr int kMax = 32;
  unsigned* addr[kMax] = {};
  int n = 0;
  unsigned value = 0;
  unsigned* status = nullptr;
  unsigned long long ticks = 0;
};
void launch_flag_sync(const FlagOp& wait, const FlagOp& signal, hipStream_t stream);

// Order-independent hash of the owned nodes of field f (Σ mix64(bits ^ mix64(global index)) mod 2⁶⁴), added into *out
// (zeroed by the caller): equal for bit-identical fields whatever the decomposition (GpuSolver::field_hash).
void launch_field_hash(const Layout& l, const double* f, unsigned long long* out, hipStream_t stream);

// Pack all strided faces of `plan` from `u` into `buf`, or unpack `buf` into the ghost layers of `u`.
void launch_pack(const Layout& l, const HaloPlan& plan, const double* u, double* buf, hipStream_t stream);
void launch_unpack(const Layout& l, const HaloPlan& plan, const double* buf, double* u, hipStream_t stream);

}  // namespace wave3d
