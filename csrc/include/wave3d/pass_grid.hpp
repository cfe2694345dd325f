// Workgroup counts of the LDS S-step passes, decided on the host from integers alone (no HIP header): the (y, z) tile
// grid times the x chunks of one box (k_leapfrog_tb and the pair-tiled k_leapfrog_p2), the shares of a launch over
// several boxes, the width of the error-partial slot every launch of a solver fills, and whether a rank's shell boxes
// go into one launch. The launchers (kernels_leapfrog_tb.hip, kernels_leapfrog_p2.hip) and GpuSolver call this code, so
// a slot is sized by the same arithmetic that later fills it; csrc/tests/test_core.cpp sweeps it over the rank shapes
// the project is built for.
#pragma once

#include "wave3d/leapfrog_p2_geometry.hpp"
#include "wave3d/tiling.hpp"

namespace wave3d {

static_assert(p2k::kT == kTbTile, "both LDS pass families tile (y, z) by the same edge");

// workgroup grid of one box of a launch: nty × ntz tiles, each marched in nxc chunks of xlen planes, from workgroup
// blk0 of the launch on
struct PassBoxGrid {
  int nty = 0, ntz = 0;
  int xlen = 1, nxc = 0;
  int blk0 = 0;
  int tiles() const { return nty * ntz; }
  int blocks() const { return nty * ntz * nxc; }
};

// ---- the pair-tiled pass (k_leapfrog_p2)

// LDS budget of a pass: the largest x chunk whose sin table still fits next to the planes (the analytic start uses
// the same planes: its φ values are table products)
inline int p2_max_xlen(int S) {
  const size_t cap = 160 * 1024 - 2 * 16 * sizeof(double) - 256;  // minus the reduction arrays (+ alignment slack)
  size_t base = 0;
  switch (S) {
    case 2: base = p2k::p2_lds_bytes<2>(0); break;
    case 3: base = p2k::p2_lds_bytes<3>(0); break;
    case 4: base = p2k::p2_lds_bytes<4>(0); break;
    default: base = p2k::p2_lds_bytes<5>(0); break;
  }
  if (base >= cap) return 0;
  return static_cast<int>((cap - base) / sizeof(double)) - (2 * S + 4);
}

// grid of a pass of S steps over the non-empty box b: the (y, z) tile grid times the x chunks
inline PassBoxGrid p2_box_grid(const LBox& b, const LeapfrogTbTiling& t, int S) {
  PassBoxGrid g;
  g.nty = static_cast<int>(ceil_div(b.y1 - b.y0, kTbTile));
  g.ntz = static_cast<int>(ceil_div(b.z1 - b.z0, kTbTile));
  const int tiles = g.tiles();
  const i64 nxb = b.x1 - b.x0;
  i64 want = 1;
  // x chunks when the tile grid alone leaves CUs idle (at least min_chunk planes each), or when the x sin table of
  // the whole range would not fit the LDS. (At most target_blocks workgroups: one CU each. Rounding the chunk count up
  // instead put e.g. a 7 × 7-tile interior box on 294 workgroups — 256 and then a second round of 38.)
  if (t.target_blocks > tiles) want = imin(imax(1, t.target_blocks / tiles), imax(1, nxb / imax(1, t.min_chunk)));
  const int maxlen = p2_max_xlen(S);
  W3D_REQUIRE(maxlen >= 1, "leapfrog_p2: the tile does not fit in LDS");
  want = imax(want, ceil_div(nxb, maxlen));
  g.xlen = static_cast<int>(ceil_div(nxb, want));
  g.nxc = static_cast<int>(ceil_div(nxb, g.xlen));
  return g;  // (unrounded: the launch grid rounds the sum of its boxes up to whole XCD shares)
}

// (either kernel) a launch grid: whole XCD shares under xcd_remap
inline int pass_round(int blocks, const LeapfrogTbTiling& t) {
  return t.xcd_remap ? static_cast<int>(round_up(blocks, 8)) : blocks;
}

// A launch of t.stages steps over n boxes (n ≤ kP2MaxBoxes): one grid, box k from workgroup blk0_k on. With several
// boxes each one's x-chunk target is its share of t.target_blocks by work (tiles × planes), so together they fill the
// GPU once — but a box never gets fewer workgroups than it has tiles, so the sum can exceed the target by up to the
// boxes' tile count (a thin x slab beside long y / z rows keeps all its tiles whatever its share).
struct P2LaunchGrid {
  PassBoxGrid box[kP2MaxBoxes];
  int nbox = 0;
  int nactive = 0;   // workgroups with a tile (Σ over the boxes)
  int nblocks = 0;   // the launch grid (nactive rounded up to whole XCD shares under xcd_remap)
  bool chunked = false;
  int xlen_max = 1;  // the longest chunk (the LDS x sin table)
};
inline P2LaunchGrid p2_launch_grid(const LBox* boxes, int n, const LeapfrogTbTiling& t) {
  W3D_REQUIRE(n >= 1 && n <= kP2MaxBoxes, "leapfrog_p2: too many boxes for one launch");
  auto box_work = [](const LBox& b) {
    return static_cast<double>(ceil_div(imax(0, b.y1 - b.y0), kTbTile) * ceil_div(imax(0, b.z1 - b.z0), kTbTile) *
                               imax(0, b.x1 - b.x0));
  };
  double work = 0.0;
  for (int k = 0; k < n; ++k) work += box_work(boxes[k]);
  P2LaunchGrid pl;
  pl.nbox = n;
  int blk = 0;
  for (int k = 0; k < n; ++k) {
    LeapfrogTbTiling tk = t;
    if (n > 1 && work > 0.0) tk.target_blocks = imax(1, static_cast<int>(t.target_blocks * box_work(boxes[k]) / work));
    const LBox& b = boxes[k];
    PassBoxGrid& g = pl.box[k];
    if (b.x1 > b.x0 && b.y1 > b.y0 && b.z1 > b.z0) g = p2_box_grid(b, tk, t.stages);
    g.blk0 = blk;
    blk += g.blocks();
    if (g.nxc > 1) pl.chunked = true;
    pl.xlen_max = static_cast<int>(imax(pl.xlen_max, g.xlen));
  }
  pl.nactive = blk;
  pl.nblocks = blk == 0 ? 0 : pass_round(blk, t);
  return pl;
}

// error partials per level of a pair-tiled launch over `box`, whatever its stage count
inline int p2_partials(const LBox& box, const LeapfrogTbTiling& t) {
  // (the largest block count over S = 2..5: the chunk length shrinks with S, whose levels share the LDS with the
  // chunk's x sin table — ADVICE r5: S = 2 alone undercounted boxes longer than the S = 5 chunk)
  if (box.x1 <= box.x0 || box.y1 <= box.y0 || box.z1 <= box.z0) return 0;
  int n = 0;
  for (int S = 2; S <= 5; ++S) n = static_cast<int>(imax(n, pass_round(p2_box_grid(box, t, S).blocks(), t)));
  return n;
}

// ---- k_leapfrog_tb (one node per thread; its block count does not depend on the stage count)

inline PassBoxGrid tb_box_grid(const LBox& b, const LeapfrogTbTiling& t) {
  PassBoxGrid g;
  g.nty = static_cast<int>(ceil_div(b.y1 - b.y0, kTbTile));
  g.ntz = static_cast<int>(ceil_div(b.z1 - b.z0, kTbTile));
  const int tiles = g.tiles();
  g.xlen = static_cast<int>(imax(1, b.x1 - b.x0));
  g.nxc = 1;
  // x chunks when the tile grid alone leaves CUs idle (3-D block boxes): at least min_chunk planes per chunk
  if (t.target_blocks > tiles) {
    const i64 nxb = b.x1 - b.x0;
    const i64 want = imin(ceil_div(t.target_blocks, tiles), imax(1, nxb / imax(1, t.min_chunk)));
    g.xlen = static_cast<int>(ceil_div(nxb, imax(1, want)));
    g.nxc = static_cast<int>(ceil_div(nxb, g.xlen));
  }
  return g;
}

// ---- either kernel

// Which kernel family runs a launch of `stages` steps over `box`: the pair-tiled pass where tiling.p2 asks for it and
// it applies — a box it takes (leapfrog_p2_supported), no push transport and no fused pack (both live in
// k_leapfrog_tb), an analytic start of at most 4 steps — else k_leapfrog_tb, which then refuses S = 5. The launcher
// dispatches by this rule, and everything that sizes or plans for a launch (GpuSolver, schedule.cpp) asks it too.
enum class PassKernel { kTb, kP2 };
inline PassKernel pass_kernel(const Layout& l, const LBox& box, int stages, bool p2, bool analytic_start, bool push,
                              bool pack) {
  return p2 && !push && !pack && leapfrog_p2_supported(l, box, stages) && !(analytic_start && stages > 4)
             ? PassKernel::kP2
             : PassKernel::kTb;
}

// The checks a box must pass before either kernel marches it, per axis (g0: the rank's global offset, n: its nodes,
// g: its ghost depth): u^{n+k} (k < S) is read up to S−k nodes beyond the box, so its values there must be real (the
// `real` range) unless they lie beyond the global boundary (structural zeros); u^n is read S nodes beyond the box,
// within the allocation unless beyond the global boundary. Returns `real` with its defaulted axes (lo > hi) resolved:
// x: the compute box; y, z: the whole allocation. yz_real: k_leapfrog_tb, which has y/z real ranges and takes boxes of
// the compute box only; the pair-tiled pass has neither (its box rule is leapfrog_p2_supported), so there only the
// halo depth is checked in y and z. `name` starts the messages.
inline LBox pass_box_check(const Layout& l, const LBox& b, i64 S, LBox real, const char* name, bool yz_real) {
  const LBox full = compute_box(l);
  auto msg = [&](const char* what, const char* ax) { return std::string(name) + what + ax; };
  if (real.x0 > real.x1) real.x0 = full.x0, real.x1 = full.x1;
  if (real.y0 > real.y1) real.y0 = -l.yg, real.y1 = l.ny + l.yg;
  if (real.z0 > real.z1) real.z0 = -l.zg, real.z1 = l.nz + l.zg;
  W3D_REQUIRE(!yz_real || (b.x0 >= full.x0 && b.x1 <= full.x1 && b.y0 >= full.y0 && b.y1 <= full.y1 &&
                           b.z0 >= full.z0 && b.z1 <= full.z1),
              msg(" box outside the compute box", ""));
  auto axis = [&](i64 b0, i64 b1, i64 r0, i64 r1, i64 g0, i64 n, i64 g, bool ranged, const char* ax) {
    W3D_REQUIRE((g0 + b0 - S <= 0 || b0 - S >= -g) && (g0 + b1 + S - 1 >= l.N || b1 + S - 1 < n + g),
                msg(": halo deeper than the ghosts in ", ax));
    if (!ranged) return;
    const bool lo_ok = r0 <= b0 - (S - 1) || g0 + r0 <= 1;
    const bool hi_ok = r1 >= b1 + (S - 1) || g0 + r1 >= l.N;
    W3D_REQUIRE(lo_ok && hi_ok, msg(": stage-1 range does not cover the box halo in ", ax));
    W3D_REQUIRE(r0 >= -g && r1 <= n + g, msg(": real range outside the allocation in ", ax));
  };
  axis(b.x0, b.x1, real.x0, real.x1, l.gx0, l.nx, l.xg, true, "x");
  axis(b.y0, b.y1, real.y0, real.y1, l.gy0, l.ny, l.yg, yz_real, "y");
  axis(b.z0, b.z1, real.z0, real.z1, l.gz0, l.nz, l.zg, yz_real, "z");
  return real;
}

// Error partials per level that a launch_leapfrog_tb over `box` writes: a slot holds either kernel's partials (the
// pair-tiled pass may split x differently).
inline int tb_partials(const Layout& l, const LBox& box, const LeapfrogTbTiling& t) {
  if (box.x1 <= box.x0 || box.y1 <= box.y0 || box.z1 <= box.z0) return 0;
  const int n = pass_round(tb_box_grid(box, t).blocks(), t);
  return t.p2 && leapfrog_p2_supported(l, box, 2) ? static_cast<int>(imax(n, p2_partials(box, t))) : n;
}

// Width of the partial slots of a solver whose compute box is `full`: every launch of a unit pads its grid to this
// many workgroups (grid_blocks), so a reduction reads only written entries. deep_tb: multi-rank units also launch
// sub-boxes of the compute box (shells, interior), whose fewer tiles may be split into more x chunks: at most
// tiles · ceil(target / tiles) < tiles + target blocks.
inline int tb_slot_blocks(const Layout& l, const LBox& full, const LeapfrogTbTiling& t, bool deep_tb) {
  int n = tb_partials(l, full, t);
  if (deep_tb)
    n = static_cast<int>(imax(n, round_up(ceil_div(full.y1 - full.y0, kTbTile) * ceil_div(full.z1 - full.z0, kTbTile) +
                                              t.target_blocks, 8)));
  return n;
}

// Workgroups of ONE pair-tiled launch of t.stages steps over all of a unit's shell boxes (no XCD remap: the boxes'
// workgroups differ in length), or 0 where the boxes get one launch each:
//   * fewer than two boxes, more than a launch holds, or a box the pair-tiled pass does not run (pass_kernel);
//   * the shells' tiles alone fill the GPU (a 2048³ block rank's x-slab shell has 961 tiles of 5 planes beside 63
//     border tiles of 1024 — one grid then runs no faster than three, and measured slower);
//   * the combined grid does not fit the partial slot of `slot` workgroups. Every box keeps at least its tile count
//     whatever its work share (p2_launch_grid), so the sum reaches target_blocks + Σ tiles: an interior rank with
//     11 × 11 tiles at S = 5, target 256, needs 402 workgroups against a slot of 384.
inline int tb_shells_launch_blocks(const Layout& l, const LBox* boxes, int n, LeapfrogTbTiling t, int slot,
                                   bool analytic_start = false, bool push = false, bool pack = false) {
  if (n < 2 || n > kP2MaxBoxes) return 0;
  i64 tiles = 0;
  for (int k = 0; k < n; ++k) {
    if (pass_kernel(l, boxes[k], t.stages, t.p2, analytic_start, push, pack) != PassKernel::kP2) return 0;
    tiles += ceil_div(imax(0, boxes[k].y1 - boxes[k].y0), kTbTile) * ceil_div(imax(0, boxes[k].z1 - boxes[k].z0), kTbTile);
  }
  if (tiles > t.target_blocks) return 0;
  t.xcd_remap = false;
  const int blocks = p2_launch_grid(boxes, n, t).nblocks;
  return blocks <= slot ? blocks : 0;
}

}  // namespace wave3d
