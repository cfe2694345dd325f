// Pair-tiled deep temporal blocking (k_leapfrog_p2, leapfrog_p2_kernel.hpp): S = 2..5 leapfrog steps per HBM pass.
//
// Why a second LDS S-step kernel. The 4-step pass of k_leapfrog_tb (one node per thread and position set) ran at
// 1.0–1.06 ms against ≈0.8 ms for its bytes, and its compute alone took 684 µs (profiles/r4/lds_read2.md): per bulk
// iteration a wave issued ≈570 instructions for 8 node-stages — 240 of them scalar (exec-mask branches per stage and
// position set, 64-bit plane pointers), 13 LDS reads + a write per node-stage, and 9 of 16 waves carried a second,
// partly empty position set that the others waited for at every barrier. S = 5 (one HBM pass fewer per 20-step
// solve) did not fit its registers. This kernel is laid out for CDNA4 from the instruction stream up:
//   * TWO z-adjacent nodes per thread (a 16-byte pair): the y neighbours of both are one ds_read_b128 each, the z
//     neighbours one ds_read_b64 each, the new values one ds_write_b128 — 5 LDS instructions per pair-stage instead of
//     10 — and the loads and stores of a pair are one buffer dwordx4 each;
//   * the tile's own 32 × 32 nodes are exactly waves 0–7 (the lane groups of ds_read_b128 each hold one tile row, so
//     every y-neighbour read is conflict-free); the halo pairs follow in "onion" order, so a wave computes only the
//     stages its deepest pair needs (stage k's region shrinks by one node per side), and the halo waves are dealt to
//     the four SIMDs by stage work (leapfrog_p2_kernel.hpp make_tab): per plane ≈54 pair-stage wave-instructions
//     where position sets × stages would be 62.5, spread within one stage over the SIMDs;
//   * stores and the check run only in waves 0–7 (wave-uniform), Dirichlet zeros are selects on SGPR lane masks
//     (all-true in interior tiles), the x tests of the general planes are scalar: the bulk iteration has no exec-mask
//     branches at all;
//   * planes are addressed through buffer resources (a 32-bit per-thread offset, the plane base in SGPRs; an offset
//     past the plane returns 0 / drops a store), and every wave issues the same vector-memory sequence, so the
//     in-order vmcnt wait of the u^n commit covers exactly its load, not the previous stores;
//   * S = 5 at 128 VGPRs: u^{n−1} and u^n are loaded late (after stages 1 and 2, into registers those stages free),
//     three per-thread LDS bases replace per-plane address registers, and the loop-invariant address folding that
//     LLVM would otherwise hoist is blocked per iteration.
// One pass is bit-identical to S single steps (stencil.hpp formulas and operation order), the analytic-start pass to
// k_init_first + S steps. Tests: tests/test_gpu_kernels.py (test_leapfrog_p2_*).
#include "wave3d/leapfrog_p2_launch.hpp"
#include "wave3d/pass_grid.hpp"

#ifdef W3D_EXPERIMENT_WGTIME
#include <array>
#include <cstdio>
#include <cstdlib>
#include <vector>
#endif

namespace wave3d {

using namespace p2k;

namespace {

// the checks a box must pass (returns `real` resolved); its grid (tiles × x chunks, first workgroup) is g (pass_grid.hpp
// p2_launch_grid)
LBox p2_box(const Layout& l, const LBox& b, const LeapfrogTbTiling& t, LBox real, const PassBoxGrid& g, P2Box& bx) {
  W3D_REQUIRE(leapfrog_p2_supported(l, b, t.stages),
              "leapfrog_p2: the box must lie in the rank's y/z range on whole pairs");
  real = pass_box_check(l, b, t.stages, real, "leapfrog_p2", false);
  bx.x0 = static_cast<int>(b.x0);
  bx.x1 = static_cast<int>(b.x1);
  bx.y0 = static_cast<int>(b.y0);
  bx.z0 = static_cast<int>(b.z0);
  bx.y1 = static_cast<int>(b.y1);
  bx.z1 = static_cast<int>(b.z1);
  bx.blk0 = g.blk0;
  // ghost-plane stores of u^{n+S−1}: only on a side at the rank's face, within the real (computed) range
  const LBox full = compute_box(l);
  bx.gxl = (t.ghost_x1 & 1) && b.x0 == full.x0 ? 1 : 0;
  bx.gxh = (t.ghost_x1 & 2) && b.x1 == full.x1 ? 1 : 0;
  W3D_REQUIRE(!bx.gxl || (real.x0 <= b.x0 - 1 && b.x0 - 1 >= -l.xg), "leapfrog_p2: ghost plane x0 − 1 not computed");
  W3D_REQUIRE(!bx.gxh || (real.x1 >= b.x1 + 1 && b.x1 < l.nx + l.xg), "leapfrog_p2: ghost plane x1 not computed");
  bx.nty = g.nty;
  bx.ntz = g.ntz;
  bx.xlen = g.xlen;
  bx.nxc = g.nxc;
  return real;
}

// A launch over n boxes (n ≤ kP2Boxes): one grid, box k from workgroup blk0_k on; the block counts are the host-side
// arithmetic of pass_grid.hpp (p2_launch_grid), which also sizes the partial slots. nblocks = 0: nothing to launch.
P2Params make_plan_p2(const Layout& l, const LBox* boxes, int n, const LeapfrogTbTiling& t, LBox real, bool init) {
  const int S = t.stages;
  W3D_REQUIRE(S >= 2 && S <= 5, "leapfrog_p2: stages must be 2..5");
  W3D_REQUIRE(!init || S <= 4, "leapfrog_p2: the analytic-start pass takes at most 4 steps");
  W3D_REQUIRE(n >= 1 && n <= kP2Boxes, "leapfrog_p2: too many boxes for one launch");
  W3D_REQUIRE(l.plane < (i64{1} << 27), "leapfrog_p2: plane too large for 32-bit buffer offsets");
  P2Params p{};
  p.plane = l.plane;
  p.pitch = static_cast<int>(l.pitch);
  p.ya = static_cast<int>(l.yg);
  p.za = static_cast<int>(l.zg + l.zs);
  p.ay0 = static_cast<int>(-l.yg);
  p.ay1 = static_cast<int>(l.ny + l.yg);
  p.ax0 = static_cast<int>(-l.xg);
  p.ax1 = static_cast<int>(l.nx + l.xg);
  p.N = static_cast<int>(l.N);
  p.gx0 = static_cast<int>(l.gx0);
  p.gy0 = static_cast<int>(l.gy0);
  p.gz0 = static_cast<int>(l.gz0);
  const P2LaunchGrid gr = p2_launch_grid(boxes, n, t);
  p.nbox = n;
  p.chunked = gr.chunked ? 1 : 0;
  p.xlen_max = gr.xlen_max;
  LBox r = real;  // (the same resolved range from every box)
  for (int k = 0; k < n; ++k) r = p2_box(l, boxes[k], t, real, gr.box[k], p.box[k]);
  p.sx0 = static_cast<int>(r.x0);
  p.sx1 = static_cast<int>(r.x1);
  const int blk = gr.nactive;
  p.nactive = blk;
  if (blk == 0) return p;
  p.nblocks = gr.nblocks;
  p.xcd_remap = t.xcd_remap ? 1 : 0;
  p.xper = p.nblocks / 8;
  return p;
}

#ifdef W3D_EXPERIMENT_WGTIME
// (perf study) every launch gets its own slot of 4 stamps per workgroup in pinned host memory (a captured launch keeps
// its slot: each replay overwrites it, so the file holds the last replay); written to $W3D_WGTIME_OUT at exit as text
// lines "launch S init nblocks" followed by one line of 4 stamps (100 MHz wall clock) per workgroup
struct WgTimeLog {
  unsigned long long* buf = nullptr;
  size_t cap = size_t{1} << 22, used = 0;
  std::vector<std::array<int, 4>> launches;  // S, init, nblocks, offset / 4
};
WgTimeLog& wgtime_log() {
  static WgTimeLog g;
  return g;
}
void wgtime_dump() {
  WgTimeLog& g = wgtime_log();
  const char* path = std::getenv("W3D_WGTIME_OUT");
  if (!path || !g.buf) return;
  FILE* f = std::fopen(path, "w");
  if (!f) return;
  for (size_t l = 0; l < g.launches.size(); ++l) {
    const auto& L = g.launches[l];
    std::fprintf(f, "launch %zu %d %d %d\n", l, L[0], L[1], L[2]);
    for (int b = 0; b < L[2]; ++b) {
      const unsigned long long* q = g.buf + (static_cast<size_t>(L[3]) + b) * 4;
      std::fprintf(f, "%llu %llu %llu %llu\n", q[0], q[1], q[2], q[3]);
    }
  }
  std::fclose(f);
}
unsigned long long* wgtime_slot(int nblocks, int S, bool init) {
  WgTimeLog& g = wgtime_log();
  if (!g.buf) {
    W3D_REQUIRE(hipHostMalloc(reinterpret_cast<void**>(&g.buf), g.cap * sizeof(unsigned long long),
                              hipHostMallocDefault) == hipSuccess,
                "wgtime: pinned buffer");
    std::atexit(wgtime_dump);
  }
  if (nblocks == 0) return g.buf;
  W3D_REQUIRE(g.used + static_cast<size_t>(nblocks) * 4 <= g.cap, "wgtime: log full");
  unsigned long long* q = g.buf + g.used;
  g.launches.push_back({S, init ? 1 : 0, nblocks, static_cast<int>(g.used / 4)});
  g.used += static_cast<size_t>(nblocks) * 4;
  return q;
}
#endif

}  // namespace

int leapfrog_p2_partials(const Layout& l, const LBox& box, const LeapfrogTbTiling& t) {
  (void)l;
  return p2_partials(box, t);
}

std::vector<int> leapfrog_p2_table(int stages, std::vector<long>* geometry) {
  auto one = [&](auto sc) {
    constexpr int S = decltype(sc)::value;
    using G = p2k::Geo<S>;
    constexpr p2k::TabBuild<S> t = p2k::make_tab<S>();
    if (geometry)
      *geometry = {G::E, G::HY, G::HZ, G::PZ, p2k::kT,
                   static_cast<long>(p2k::p2_lds_bytes<S>(p2k::p2_nxt<S>(512))),
                   S <= 4 ? static_cast<long>(p2k::p2_lds_bytes<S>(p2k::p2_nxt<S>(512))) : 0L,
                   static_cast<long>(p2_max_xlen(S)), S <= 4 ? static_cast<long>(p2_max_xlen(S)) : 0L};
    return std::vector<int>(t.t.d, t.t.d + p2k::kNT);
  };
  switch (stages) {
    case 2: return one(std::integral_constant<int, 2>{});
    case 3: return one(std::integral_constant<int, 3>{});
    case 4: return one(std::integral_constant<int, 4>{});
    case 5: return one(std::integral_constant<int, 5>{});
    default: fail("leapfrog_p2_table: stages must be 2..5");
  }
  return {};
}

void leapfrog_p2_prepare() {
#ifdef W3D_EXPERIMENT_WGTIME
  wgtime_slot(0, 0, false);  // (the pinned buffer, before any capture)
#endif
  prepare_p2_s2();
  prepare_p2_s3();
  prepare_p2_s4();
  prepare_p2_s5();
  prepare_p2_box_s2();
  prepare_p2_box_s3();
  prepare_p2_box_s4();
  prepare_p2_box_s5();
  prepare_p2_varc_s2();
  prepare_p2_varc_s3();
  prepare_p2_varc_s4();
}

void launch_leapfrog_p2_boxes(const Layout& l, const Coeffs& c, const LBox* boxes, int nbox, const PassArgs& a,
                              hipStream_t stream) {
  const LeapfrogTbTiling& t = a.tiling;
  // out1 = null: u^{n+S−1} is not stored at all, so nothing may depend on its ghost planes (an exchange after the
  // pass, or z-face packing, never reaches this launcher without one of them: pass_kernel)
  W3D_REQUIRE(a.out1 != nullptr || (t.ghost_x1 == 0 && a.pack == nullptr && a.push == nullptr),
              "leapfrog_p2: a pass without u^{n+S-1} (out1 = null) cannot store its ghost planes (ghost_x1) or pack");
  if (a.lamf != nullptr) {  // a speed field: the VARC load passes, or a refusal — never the constant operator
    W3D_REQUIRE(!a.analytic_start, "speed: the analytic-start pass has no coefficient form (a speed solve has a stored start)");
    W3D_REQUIRE(a.out1 != nullptr, "speed: a pass without u^{n+S-1} (out1 = null) is not built with a coefficient field");
    W3D_REQUIRE(a.pack == nullptr && a.push == nullptr, "speed: no push transport or fused pack with a coefficient field");
    W3D_REQUIRE(t.stages >= 2 && t.stages <= kP2VarcMaxStages,
                "speed: the pair-tiled pass with a coefficient field is built for 2.." + std::to_string(kP2VarcMaxStages) +
                    " steps, not " + std::to_string(t.stages));
    for (int k = 0; k < nbox; ++k)
      W3D_REQUIRE(leapfrog_p2_supported(l, boxes[k], t.stages),
                  "speed: the pair-tiled pass does not take this box (whole pairs inside the rank's y/z range)");
  }
  P2Params p = make_plan_p2(l, boxes, nbox, t, a.real, a.analytic_start);
  if (!fill_pass_params(p, l, c, a, "leapfrog_p2")) return;
  if (a.analytic_start) {  // (the analytic start reads neither: any valid buffer)
    p.prev = p.out2;
    p.cur = p.out2;
  }
#ifdef W3D_EXPERIMENT_WGTIME
  p.wgtime = wgtime_slot(p.nblocks, t.stages, a.analytic_start);
#endif
  if (a.lamf != nullptr) {
    switch (t.stages) {
      case 2: launch_p2_varc_s2(p, p.nblocks, c.box, stream); break;
      case 3: launch_p2_varc_s3(p, p.nblocks, c.box, stream); break;
      default: launch_p2_varc_s4(p, p.nblocks, c.box, stream); break;
    }
  } else if (c.box) {  // (a rectangular box: the BOX instantiations; a cube launches exactly what it always did)
    switch (t.stages) {
      case 2: launch_p2_box_s2(p, p.nblocks, a.analytic_start, stream); break;
      case 3: launch_p2_box_s3(p, p.nblocks, a.analytic_start, stream); break;
      case 4: launch_p2_box_s4(p, p.nblocks, a.analytic_start, stream); break;
      default: launch_p2_box_s5(p, p.nblocks, a.analytic_start, stream); break;
    }
  } else {
    switch (t.stages) {
      case 2: launch_p2_s2(p, p.nblocks, a.analytic_start, stream); break;
      case 3: launch_p2_s3(p, p.nblocks, a.analytic_start, stream); break;
      case 4: launch_p2_s4(p, p.nblocks, a.analytic_start, stream); break;
      default: launch_p2_s5(p, p.nblocks, a.analytic_start, stream); break;
    }
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) fail(std::string("leapfrog_p2 launch: ") + hipGetErrorString(e));
}

}  // namespace wave3d
