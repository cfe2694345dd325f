// Tiling knobs of the leapfrog kernels and the Layout arithmetic that says where each kernel applies: what the host-side
// schedule (schedule.hpp) needs to know about the kernels. No HIP header; kernels.hpp holds the launch interface.
#pragma once

#include "wave3d/cpu.hpp"
#include "wave3d/decomp.hpp"

namespace wave3d {

// Tiling knobs of the leapfrog kernel (runtime-selectable so the tuner/bench can sweep them).
struct LeapfrogTiling {
  int variant = 1;        // 0 = LDS-staged workgroup tile (k_leapfrog_lds), 1 = register-queue waves (k_leapfrog_rq)
  int rows = 2;           // variant 1: rows (y) per wave held in registers (1, 2, 4 or 8)
  int ty = 8;             // variant 0: tile rows (y) per workgroup; block = 64 × ty threads
  int target_blocks = 0;  // x-chunking aims for at least this many work items (v0: workgroups, v1: waves; 0 = auto)
  bool xcd_remap = true;  // give each XCD a contiguous range of tiles (L2 reuse of tile halos)
  bool nt_store = true;   // non-temporal stores of u^{n+1} (measured faster on MI355X, profiles/)
};

// The two-step pass (launch_leapfrog2, kernels.hpp).
struct Leapfrog2Tiling {
  int rows = 2;           // output rows per wave (1, 2 or 4)
  int occupancy = 0;      // rows = 2 only: >= 3 builds for 3 waves/SIMD (register cap, some spills)
  int target_waves = 0;   // x-chunking target (0 = auto)
  bool xcd_remap = true;
  bool nt_store = true;
};

// The LDS S-step passes (launch_leapfrog_tb, kernels.hpp).
constexpr int kTbTile = 32;  // (y, z) tile edge of the LDS S-step passes (leapfrog_tb_kernel.hpp tbk::kTile)
struct LeapfrogTbTiling {
  int stages = 4;         // steps per pass: 2..4 (k_leapfrog_tb), 2..5 (k_leapfrog_p2)
  int threads = 1024;     // workgroup size (768 or 1024)
  int init_threads = 768; // ... of the analytic-start pass (measured at 512³, S = 3: 768 → 932 µs, 1024 → 1027 µs;
                          // the S = 4 passes go the other way: 768 → 1123 µs, 1024 → 1076 µs)
  bool xcd_remap = true;  // (stores are always non-temporal: measured faster at every S)
  bool xcd_blocks = false; // with xcd_remap: each XCD owns a square-ish tile block, not two-row strips (measured: no gain)
  int target_blocks = 256; // fewer (y,z) tiles than this: split x into chunks (one workgroup per CU at 1 WG/CU)
  int min_chunk = 16;      // ... of at least this many planes (each chunk recomputes S−1 planes on both sides)
  bool p2 = true;          // the pair-tiled pass (k_leapfrog_p2, S ≤ 5) wherever it applies (leapfrog_p2_supported)
  // (pair-tiled pass only) bit 0 / 1: also store u^{n+S−1} on the x ghost plane −1 / nx where a box starts / ends at
  // the rank's first / last plane. The pass computes that plane anyway (level S−1 reaches one node beyond the box), so
  // the slab exchange that follows sends S − 2 planes of u^{n+S−1} per face instead of S − 1 (schedule.cpp
  // plan_units). The 4-step k_leapfrog_tb refuses it.
  int ghost_x1 = 0;
};

// Stage-real ranges of an LDS pass: per axis, where the intermediate levels hold real values (S−1 nodes into the
// S-deep ghosts towards neighbouring ranks); lo > hi: the axis default (x: compute box, y/z: no restriction).
inline LBox tb_default_real() { return LBox{1, 0, 1, 0, 1, 0}; }

// Whether the pair-tiled S-step pass (kernels_leapfrog_p2.hip) runs `box` at this depth: any box inside the rank's
// compute range in y/z (the whole range: one rank, x slabs, a 3-D block's whole box; or a sub-box: the overlapped
// schedule's shells and interior, cpu.hpp deep_split) whose pairs start on 16-byte nodes and which ends on a whole pair
// unless it ends at the rank's last node: the pass stores whole pairs, so a box ending in the middle of a pair would
// also write the first node of the next box (beyond the rank's last node the second node of a pair is a ghost, which
// the next exchange rewrites)
inline bool leapfrog_p2_supported(const Layout& l, const LBox& box, int stages) {
  const LBox full = compute_box(l);
  return stages >= 2 && stages <= 5 && l.yg >= 1 && l.zg >= 1 && box.y0 >= full.y0 && box.y1 <= full.y1 &&
         box.z0 >= full.z0 && box.z1 <= full.z1 && (box.z0 + l.zg + l.zs) % 2 == 0 &&
         (box.z1 == full.z1 || (box.z1 - box.z0) % 2 == 0);
}
// deepest pair-tiled pass built with a coefficient field (PassArgs::lamf; kernels_leapfrog_p2_varc_s*.hip)
constexpr int kP2VarcMaxStages = 4;
constexpr int kP2MaxBoxes = 6;  // boxes per pair-tiled launch (deep_split: up to 6 shells)

}  // namespace wave3d
