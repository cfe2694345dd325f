// The fourth-order march: one application of the fourth-order operator (stencil.hpp d4sum_t) to a marched field q, shared
// by k_leapfrog4 (kernels_stencil4.hip) and k_lap4 / k_leapfrog44 (kernels_stencil44.hip), with its tiling plan and its
// launch dispatch.
//
// 2.5-D like k_leapfrog_lds (kernels_stencil.hip): a workgroup owns a (TY rows × 64 pairs) tile of the (y, z) plane and
// marches along x; each thread owns one 16-byte pair.
//   * x: a five-deep register queue of the thread's own column of q (x−2 … x+2), x+3 prefetched one plane ahead.
//   * y, z: plane x of q goes through a double-buffered LDS tile with a halo of two rows above and below and one pair left
//     and right (one pair = two nodes = the z radius); one barrier per plane. A wave is one tile row, so every LDS read
//     (rows ±1, ±2 and the pairs left and right) is 64 consecutive 16-byte slots: conflict-free whatever the row stride.
//   * `out` is updated in place where the mode reads it.
//   * Walls are handled in registers. The neighbour at distance 2 of node 1 / N − 1 of an axis is −centre (odd
//     reflection), chosen by a select on the node's global index: the ghost layer, the row padding and the planes −1 and
//     N + 1 are never used as data (the x planes and the y rows outside the grid are not even loaded).
//   * The layout spans the whole domain (one rank): a distance-2 neighbour of any other node is a stored node.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "wave3d/device_util.hpp"
#include "wave3d/kernels.hpp"
#include "wave3d/leapfrog_tiles.hpp"
#include "wave3d/stencil.hpp"

namespace wave3d {

// What a march does with l = s(q) at a node. The mode decides which fields are read besides q and the result line, nothing
// else.
enum class March4 {
  Step42,  // q = u^n:          out = leapfrog(q, out, l, coef), coef = lam           (k_leapfrog4)
  Lap,     // q = u^n:          out = lap_t4(l, coef), coef = lam; out is not read    (k_lap4; no check, ordinary stores)
  Step44,  // q = v = lam·s(u): out = leapfrog_t4(u, out, q, l, coef), coef = lam/12  (k_leapfrog44)
};

struct March4Params {
  const double* q;  // the marched field
  const double* u;  // Step44: u^n, centre values only
  double* out;      // Lap: v; Step42, Step44: u^{n−1} in, u^{n+1} out
  const double* s;
  Partial* partials;
  i64 plane, pitch, gx0, gy0, gz0, zs, N;
  double coef, ct;  // coef: see March4
  double ry, rz;    // rectangular box: h_x²/h_y², h_x²/h_z² (1 for a cube: the cube form's bits)
  TileGrid g;
};

template <int TY, March4 MODE, bool CHECK, bool NT>
__device__ __forceinline__ void march4(const March4Params& p) {
  constexpr bool LAP = MODE == March4::Lap, CENTRE = MODE == March4::Step44;
  // halo slots: 2·64 pairs above, 2·64 below, TY left, TY right — one per thread
  static_assert(4 * kLanes + 2 * TY <= kLanes * TY, "halo slots need at least 256 + 2*TY threads (TY >= 5)");
  static_assert(!LAP || (!CHECK && !NT), "k_lap4 has no check and stores v for the next launch to read");
  __shared__ v2d lds[2][TY + 4][kLanes + 2];

  const int lane = static_cast<int>(threadIdx.x);
  const int row = static_cast<int>(threadIdx.y);
  const int tid = row * kLanes + lane;

  TileBox B;
  int tz, ty, tx;
  if (!decode_tile(p.g, tile_of_block(p.g), B, tz, ty, tx)) {
    if (CHECK && tid == 0) p.partials[blockIdx.x] = make_double2(0.0, 0.0);
    return;
  }

  const i64 pzt = B.pz0 + static_cast<i64>(tz) * kLanes;
  const int npe = static_cast<int>(imin(kLanes, B.pz_end - pzt));
  const i64 yt = B.y0 + static_cast<i64>(ty) * TY;
  const int nre = static_cast<int>(imin(TY, B.y1 - yt));
  const i64 xs = B.x0 + static_cast<i64>(tx) * B.xchunk;
  const i64 xe = imin(xs + B.xchunk, B.x1);

  const bool active = row < nre && lane < npe;
  const i64 y = yt + row;
  const i64 o0 = 2 * (pzt + lane);
  const bool ok0 = active && o0 >= B.zo0 && o0 < B.zo1;
  const bool ok1 = active && o0 + 1 >= B.zo0 && o0 + 1 < B.zo1;
  const i64 pitch = p.pitch, plane = p.plane, N = p.N;
  const i64 my = (y + 1) * pitch + o0;

  // walls: global indices of the thread's row and of its two nodes
  const i64 gy = p.gy0 + y, gz0 = p.gz0 + o0 - 1 - p.zs, gz1 = gz0 + 1;
  const bool ylo = gy == 1, yhi = gy == N - 1;
  const bool zlo0 = gz0 == 1, zhi0 = gz0 == N - 1, zlo1 = gz1 == 1, zhi1 = gz1 == N - 1;

  // halo slot of this thread: rows −2, −1 above, +1, +2 below, the pair left, the pair right. hy: the slot's local row
  // (a row outside the grid is not loaded: its slot holds zeros that the wall select never passes on)
  int hr = -1, hc = 0;
  i64 hy = 0, hz = 0;
  if (tid < 4 * kLanes) {
    const int g = tid / kLanes, l = tid - g * kLanes;  // g: 0, 1 above; 2, 3 below
    if (l < npe) {
      hr = g < 2 ? g : nre + g;
      hy = g < 2 ? yt - 2 + g : yt + nre + (g - 2);
      hc = l + 1;
      hz = 2 * (pzt + l);
    }
  } else if (tid < 4 * kLanes + TY) {
    const int r = tid - 4 * kLanes;
    if (r < nre) { hr = r + 2; hy = yt + r; hc = 0; hz = 2 * (pzt - 1); }
  } else if (tid < 4 * kLanes + 2 * TY) {
    const int r = tid - 4 * kLanes - TY;
    if (r < nre) { hr = r + 2; hy = yt + r; hc = npe + 1; hz = 2 * (pzt + npe); }
  }
  const bool hload = hr >= 0 && p.gy0 + hy >= 0 && p.gy0 + hy <= N;
  const i64 hoff = (hy + 1) * pitch + hz;

  const double* __restrict__ q = p.q;
  const double* __restrict__ u = p.u;
  double* __restrict__ out = p.out;
  const v2d zero2 = {0.0, 0.0};
  v2d q2m = zero2, qm = zero2, qc = zero2, qp = zero2, q2p = zero2, uc = zero2, uo = zero2, hv = zero2;
  i64 px = (xs + 1) * plane;  // plane base of x
  if (active) {
    // (a chunk that starts at node 1 primes its queue without plane −1, one that ends at N − 1 never loads plane N + 1)
    if (p.gx0 + xs - 2 >= 0) q2m = ld2(q + px - 2 * plane + my);
    qm = ld2(q + px - plane + my);
    qc = ld2(q + px + my);
    qp = ld2(q + px + plane + my);
    if (p.gx0 + xs + 2 <= N) q2p = ld2(q + px + 2 * plane + my);
    if (CENTRE) uc = ld2(u + px + my);
    if (!LAP) uo = ld2(out + px + my);
  }
  if (hload) hv = ld2(q + px + hoff);

  const double coef = p.coef;
  double emax = 0.0, esum = 0.0;
  double sxy = 0.0, sz0 = 0.0, sz1 = 0.0, sxp = CHECK ? p.s[p.gx0 + xs] : 0.0;
  if (CHECK && active) {
    sxy = p.s[p.gy0 + y];
    sz0 = p.s[gz0];
    sz1 = p.s[gz1];
  }

  for (i64 x = xs; x < xe; ++x, px += plane) {
    const int buf = static_cast<int>((x - xs) & 1);
    const bool more = x + 1 < xe;
    const i64 gx = p.gx0 + x;
    v2d nxt = zero2, uc_n = zero2, uo_n = zero2, hv_n = zero2;
    const double nsxp = CHECK && more ? p.s[gx + 1] : 0.0;  // one plane ahead (in-order vmcnt)
    if (more) {
      if (active) {
        if (gx + 3 <= N) nxt = ld2(q + px + 3 * plane + my);
        if (CENTRE) uc_n = ld2(u + px + plane + my);
        if (!LAP) uo_n = ld2(out + px + plane + my);
      }
      if (hload) hv_n = ld2(q + px + plane + hoff);
    }
    if (active) lds[buf][row + 2][lane + 1] = qc;
    if (hr >= 0) lds[buf][hr][hc] = hv;
    __syncthreads();
    if (active) {
      const v2d ym = lds[buf][row + 1][lane + 1];
      const v2d yp = lds[buf][row + 3][lane + 1];
      const v2d y2m = ylo ? neg2(qc) : lds[buf][row][lane + 1];
      const v2d y2p = yhi ? neg2(qc) : lds[buf][row + 4][lane + 1];
      const v2d zl = lds[buf][row + 2][lane];
      const v2d zr = lds[buf][row + 2][lane + 2];
      const v2d x2m = gx == 1 ? neg2(qc) : q2m;
      const v2d x2p = gx == N - 1 ? neg2(qc) : q2p;
      const double l0 = d4sum_t<true>(qc.x, x2m.x, qm.x, qp.x, x2p.x, y2m.x, ym.x, yp.x, y2p.x, zlo0 ? -qc.x : zl.x, zl.y,
                                      qc.y, zhi0 ? -qc.x : zr.x, p.ry, p.rz);
      const double l1 = d4sum_t<true>(qc.y, x2m.y, qm.y, qp.y, x2p.y, y2m.y, ym.y, yp.y, y2p.y, zlo1 ? -qc.y : zl.y, qc.x,
                                      zr.x, zhi1 ? -qc.y : zr.y, p.ry, p.rz);
      v2d r;
      if constexpr (MODE == March4::Step42) {
        r.x = leapfrog(qc.x, uo.x, l0, coef);
        r.y = leapfrog(qc.y, uo.y, l1, coef);
      } else if constexpr (MODE == March4::Lap) {
        r.x = lap_t4(l0, coef);
        r.y = lap_t4(l1, coef);
      } else {
        r.x = leapfrog_t4(uc.x, uo.x, qc.x, l0, coef);
        r.y = leapfrog_t4(uc.y, uo.y, qc.y, l1, coef);
      }
      double* dst = out + px + my;
      if (ok0 && ok1)
        st2<NT>(dst, r);
      else if (ok0)
        dst[0] = r.x;
      else if (ok1)
        dst[1] = r.y;
      if (CHECK) {
        const double sx = analytic_row(sxp, sxy, p.ct);
        if (ok0) {
          const double e = fabs(r.x - sx * sz0);
          emax = e > emax ? e : emax;
          esum = err_sq_acc(e, esum);
        }
        if (ok1) {
          const double e = fabs(r.y - sx * sz1);
          emax = e > emax ? e : emax;
          esum = err_sq_acc(e, esum);
        }
      }
    }
    q2m = qm;
    qm = qc;
    qc = qp;
    qp = q2p;
    q2p = nxt;
    uc = uc_n;
    uo = uo_n;
    hv = hv_n;
    sxp = nsxp;
  }

  if (CHECK) block_error_store<TY>(emax, esum, lane, row, tid, p.partials);
}

// The tiling of a march: plan_tiles with leapfrog4_ty(t) rows and the chunk floor as an argument (a chunk re-reads four
// planes of q instead of k_leapfrog_lds's two), on one rank's layout that spans the domain. The caller sets the fields,
// coef and ct. `prefix` ("order: ", "time_order: ") starts the messages a caller's own arguments can break.
inline March4Params make_plan4(const Layout& l, const LBox* boxes, int nbox, const LeapfrogTiling& t, int min_chunk,
                               const char* prefix) {
  W3D_REQUIRE(l.nx == l.N + 1 && l.ny == l.N + 1 && l.nz == l.N + 1 && l.xg >= 1 && l.yg >= 1 && l.zg >= 1,
              std::string(prefix) + "the fourth-order step needs one rank's layout that spans the whole domain");
  for (int b = 0; b < nbox; ++b) {
    const LBox& x = boxes[b];
    W3D_REQUIRE(x.empty() || (x.x0 >= l.cx0 && x.x1 <= l.cx1 && x.y0 >= l.cy0 && x.y1 <= l.cy1 && x.z0 >= l.cz0 &&
                              x.z1 <= l.cz1),
                "leapfrog box outside the global interior");
  }
  March4Params p{};
  plan_tiles(l, boxes, nbox, leapfrog4_ty(t), min_chunk, t.target_blocks > 0 ? t.target_blocks : 256 * 8, prefix, p.g);
  // (the pair left of a box's first pair lies inside the row)
  for (int b = 0; b < p.g.nbox; ++b) W3D_REQUIRE(p.g.box[b].pz0 >= 1, "row pitch too small for the pair tiling");
  p.plane = l.plane;
  p.pitch = l.pitch;
  p.gx0 = l.gx0;
  p.gy0 = l.gy0;
  p.gz0 = l.gz0;
  p.zs = l.zs;
  p.N = l.N;
  p.g.xcd_remap = t.xcd_remap ? 1 : 0;
  p.g.nblocks = t.xcd_remap ? static_cast<int>(round_up(p.g.ntiles, 8)) : p.g.ntiles;
  return p;
}

// Runs launch(TY, CHECK, NT) with the tile height and the two switches as std::integral_constant tags: the one place that
// turns (ty, check, nt) into template arguments. ty is leapfrog4_ty's: 8 or 16.
template <class Launch>
void launch4_ty(int ty, bool check, bool nt, Launch launch) {
  const auto with_ty = [&](auto TY) {
    if (check) {
      if (nt)
        launch(TY, std::true_type{}, std::true_type{});
      else
        launch(TY, std::true_type{}, std::false_type{});
    } else {
      if (nt)
        launch(TY, std::false_type{}, std::true_type{});
      else
        launch(TY, std::false_type{}, std::false_type{});
    }
  };
  if (ty == 16)
    with_ty(std::integral_constant<int, 16>{});
  else
    with_ty(std::integral_constant<int, 8>{});
}

}  // namespace wave3d
