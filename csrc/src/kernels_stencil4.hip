// Fourth-order single step (Problem::order = 4): k_leapfrog4. See wave3d/kernels.hpp for the interface and
// stencil.hpp d4sum_t for the operator.
//
// 2.5-D like k_leapfrog_lds (kernels_stencil.hip): a workgroup owns a (TY rows × 64 pairs) tile of the (y, z) plane and
// marches along x; each thread owns one 16-byte pair.
//   * x: a five-deep register queue of the thread's own column (x−2 … x+2), x+3 prefetched one plane ahead.
//   * y, z: plane x goes through a double-buffered LDS tile with a halo of two rows above and below and one pair left
//     and right (one pair = two nodes = the z radius); one barrier per plane. A wave is one tile row, so every LDS read
//     (rows ±1, ±2 and the pairs left and right) is 64 consecutive 16-byte slots: conflict-free whatever the row stride.
//   * u^{n−1} is read in place and u^{n+1} written over it; 24 B/node/step of compulsory traffic, as the second-order step.
//   * Walls are handled in registers. The neighbour at distance 2 of node 1 / N − 1 of an axis is −centre (odd
//     reflection), chosen by a select on the node's global index: the ghost layer, the row padding and the planes −1 and
//     N + 1 are never used as data (the x planes and the y rows outside the grid are not even loaded).
//   * The layout spans the whole domain (one rank): a distance-2 neighbour of any other node is a stored node.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "wave3d/kernels.hpp"
#include "wave3d/stencil.hpp"

namespace wave3d {

#define W3D_HIP_CHECK(expr)                                                                          \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess) ::wave3d::fail(std::string(#expr) + ": " + hipGetErrorString(_e));          \
  } while (0)

namespace {

using v2d = double __attribute__((ext_vector_type(2)));

constexpr int kLanes = 64;
constexpr int kMaxBoxes = 6;

__device__ __forceinline__ v2d ld2(const double* p) { return *reinterpret_cast<const v2d*>(p); }

template <bool NT>
__device__ __forceinline__ void st2(double* p, v2d v) {
  if (NT)
    __builtin_nontemporal_store(v, reinterpret_cast<v2d*>(p));
  else
    *reinterpret_cast<v2d*>(p) = v;
}

__device__ __forceinline__ void wave_reduce(double& m, double& s) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double om = __shfl_xor(m, o, 64);
    const double os = __shfl_xor(s, o, 64);
    m = om > m ? om : m;
    s = s + os;
  }
}

struct Tile4Box {
  i64 x0, x1;    // local x range
  i64 y0, y1;    // local y range
  i64 zo0, zo1;  // row-offset range of the updated nodes
  i64 pz0, pz_end;
  int ntz, nty, xchunk, tile_begin;
};

struct Lf4Params {
  const double* cur;
  double* out;
  const double* s;
  Partial* partials;
  i64 plane, pitch, gx0, gy0, gz0, zs, N;
  double lam, ct;  // lam = τ²/(12h²): the coefficient of d4sum_t
  double ry, rz;   // rectangular box: h_x²/h_y², h_x²/h_z² (1 for a cube: the cube form's bits)
  int nbox, ntiles, nblocks, xcd_remap;
  Tile4Box box[kMaxBoxes];
};

__device__ __forceinline__ v2d neg2(v2d v) {
  v2d r;
  r.x = -v.x;
  r.y = -v.y;
  return r;
}

template <int TY, bool CHECK, bool NT>
__global__ __launch_bounds__(kLanes* TY) void k_leapfrog4(const Lf4Params p) {
  // halo slots: 2·64 pairs above, 2·64 below, TY left, TY right — one per thread
  static_assert(4 * kLanes + 2 * TY <= kLanes * TY, "halo slots need at least 256 + 2*TY threads (TY >= 5)");
  __shared__ v2d lds[2][TY + 4][kLanes + 2];
  __shared__ double red_m[TY], red_s[TY];

  const int lane = static_cast<int>(threadIdx.x);
  const int row = static_cast<int>(threadIdx.y);
  const int tid = row * kLanes + lane;

  int tile = static_cast<int>(blockIdx.x);
  if (p.xcd_remap) {
    const int per = p.nblocks >> 3;
    tile = (static_cast<int>(blockIdx.x) & 7) * per + (static_cast<int>(blockIdx.x) >> 3);
  }
  if (tile >= p.ntiles) {
    if (CHECK && tid == 0) p.partials[blockIdx.x] = make_double2(0.0, 0.0);
    return;
  }
  // select the box (scalar selects, no dynamic indexing of the kernarg struct)
  Tile4Box B = p.box[0];
#pragma unroll
  for (int k = 1; k < kMaxBoxes; ++k)
    if (k < p.nbox && tile >= p.box[k].tile_begin) B = p.box[k];

  int t = tile - B.tile_begin;
  const int tz = t % B.ntz;
  t /= B.ntz;
  const int ty = t % B.nty;
  const int tx = t / B.nty;

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

  const double* __restrict__ cur = p.cur;
  double* __restrict__ out = p.out;
  const v2d zero2 = {0.0, 0.0};
  v2d u2m = zero2, um = zero2, uc = zero2, up = zero2, u2p = zero2, uo = zero2, hv = zero2;
  i64 px = (xs + 1) * plane;  // plane base of x
  if (active) {
    // (a chunk that starts at node 1 primes its queue without plane −1, one that ends at N − 1 never loads plane N + 1)
    if (p.gx0 + xs - 2 >= 0) u2m = ld2(cur + px - 2 * plane + my);
    um = ld2(cur + px - plane + my);
    uc = ld2(cur + px + my);
    up = ld2(cur + px + plane + my);
    if (p.gx0 + xs + 2 <= N) u2p = ld2(cur + px + 2 * plane + my);
    uo = ld2(out + px + my);
  }
  if (hload) hv = ld2(cur + px + hoff);

  const double lam = p.lam;
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
    v2d nxt = zero2, uo_n = zero2, hv_n = zero2;
    const double nsxp = CHECK && more ? p.s[gx + 1] : 0.0;  // one plane ahead (in-order vmcnt)
    if (more) {
      if (active) {
        if (gx + 3 <= N) nxt = ld2(cur + px + 3 * plane + my);
        uo_n = ld2(out + px + plane + my);
      }
      if (hload) hv_n = ld2(cur + px + plane + hoff);
    }
    if (active) lds[buf][row + 2][lane + 1] = uc;
    if (hr >= 0) lds[buf][hr][hc] = hv;
    __syncthreads();
    if (active) {
      const v2d ym = lds[buf][row + 1][lane + 1];
      const v2d yp = lds[buf][row + 3][lane + 1];
      const v2d y2m = ylo ? neg2(uc) : lds[buf][row][lane + 1];
      const v2d y2p = yhi ? neg2(uc) : lds[buf][row + 4][lane + 1];
      const v2d zl = lds[buf][row + 2][lane];
      const v2d zr = lds[buf][row + 2][lane + 2];
      const v2d x2m = gx == 1 ? neg2(uc) : u2m;
      const v2d x2p = gx == N - 1 ? neg2(uc) : u2p;
      const double l0 = d4sum_t<true>(uc.x, x2m.x, um.x, up.x, x2p.x, y2m.x, ym.x, yp.x, y2p.x, zlo0 ? -uc.x : zl.x, zl.y,
                                      uc.y, zhi0 ? -uc.x : zr.x, p.ry, p.rz);
      const double l1 = d4sum_t<true>(uc.y, x2m.y, um.y, up.y, x2p.y, y2m.y, ym.y, yp.y, y2p.y, zlo1 ? -uc.y : zl.y, uc.x,
                                      zr.x, zhi1 ? -uc.y : zr.y, p.ry, p.rz);
      v2d r;
      r.x = leapfrog(uc.x, uo.x, l0, lam);
      r.y = leapfrog(uc.y, uo.y, l1, lam);
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
    u2m = um;
    um = uc;
    uc = up;
    up = u2p;
    u2p = nxt;
    uo = uo_n;
    hv = hv_n;
    sxp = nsxp;
  }

  if (CHECK) {
    wave_reduce(emax, esum);
    if (lane == 0) {
      red_m[row] = emax;
      red_s[row] = esum;
    }
    __syncthreads();
    if (tid == 0) {
      double m = red_m[0], s = red_s[0];
      for (int r = 1; r < TY; ++r) {
        m = red_m[r] > m ? red_m[r] : m;
        s += red_s[r];
      }
      p.partials[blockIdx.x] = make_double2(m, s);
    }
  }
}

struct Plan4 {
  Lf4Params prm;
  int nblocks;
};

// k_leapfrog_lds's tiling (one tile per workgroup, x chunks spread over the boxes by work) with the chunk floor as an
// argument: a chunk re-reads four planes of u^n instead of two.
Plan4 make_plan4(const Layout& l, const LBox* boxes, int nbox, const LeapfrogTiling& t, int min_chunk) {
  W3D_REQUIRE(nbox >= 0 && nbox <= kMaxBoxes, "too many boxes in one leapfrog launch");
  W3D_REQUIRE(min_chunk >= 1, "order: the x chunk floor must be >= 1");
  W3D_REQUIRE(l.nx == l.N + 1 && l.ny == l.N + 1 && l.nz == l.N + 1 && l.xg >= 1 && l.yg >= 1 && l.zg >= 1,
              "order: the fourth-order step needs one rank's layout that spans the whole domain");
  const int ty = leapfrog4_ty(t);
  Plan4 pl{};
  Lf4Params& p = pl.prm;
  p.plane = l.plane;
  p.pitch = l.pitch;
  p.gx0 = l.gx0;
  p.gy0 = l.gy0;
  p.gz0 = l.gz0;
  p.zs = l.zs;
  p.N = l.N;
  const int target = t.target_blocks > 0 ? t.target_blocks : 256 * 8;
  i64 base_total = 0;
  for (int b = 0; b < nbox; ++b) {
    const LBox& x = boxes[b];
    if (x.empty()) continue;
    const i64 zo0 = x.z0 + 1 + l.zs, zo1 = x.z1 + 1 + l.zs;
    base_total += ceil_div((zo1 + 1) / 2 - zo0 / 2, kLanes) * ceil_div(x.y1 - x.y0, ty);
  }
  const i64 want = base_total > 0 ? imax(1, ceil_div(target, base_total)) : 1;
  int nb = 0, tiles = 0;
  for (int b = 0; b < nbox; ++b) {
    const LBox& x = boxes[b];
    if (x.empty()) continue;
    W3D_REQUIRE(x.x0 >= l.cx0 && x.x1 <= l.cx1 && x.y0 >= l.cy0 && x.y1 <= l.cy1 && x.z0 >= l.cz0 && x.z1 <= l.cz1,
                "leapfrog box outside the global interior");
    Tile4Box& tb = p.box[nb];
    tb.x0 = x.x0;
    tb.x1 = x.x1;
    tb.y0 = x.y0;
    tb.y1 = x.y1;
    tb.zo0 = x.z0 + 1 + l.zs;
    tb.zo1 = x.z1 + 1 + l.zs;
    tb.pz0 = tb.zo0 / 2;
    tb.pz_end = (tb.zo1 + 1) / 2;
    // (the pair left of the first pair and the pair right of the last one lie inside the row)
    W3D_REQUIRE(tb.pz0 >= 1 && 2 * tb.pz_end + 2 <= l.pitch, "row pitch too small for the pair tiling");
    tb.ntz = static_cast<int>(ceil_div(tb.pz_end - tb.pz0, kLanes));
    tb.nty = static_cast<int>(ceil_div(x.y1 - x.y0, ty));
    const i64 nxb = x.x1 - x.x0;
    i64 chunk = imax(static_cast<i64>(min_chunk), ceil_div(nxb, want));
    chunk = imin(chunk, nxb);
    tb.xchunk = static_cast<int>(chunk);
    const i64 nxc = ceil_div(nxb, chunk);
    tb.tile_begin = tiles;
    const i64 bt = static_cast<i64>(tb.ntz) * tb.nty * nxc;
    W3D_REQUIRE(tiles + bt < (1ll << 30), "too many tiles");
    tiles += static_cast<int>(bt);
    ++nb;
  }
  p.nbox = nb;
  p.ntiles = tiles;
  p.xcd_remap = t.xcd_remap ? 1 : 0;
  pl.nblocks = t.xcd_remap ? static_cast<int>(round_up(tiles, 8)) : tiles;
  p.nblocks = pl.nblocks;
  return pl;
}

template <int TY>
void launch4_ty(const Lf4Params& p, int nblocks, bool check, bool nt, hipStream_t st) {
  const dim3 block(kLanes, TY), grid(nblocks);
  if (check) {
    if (nt)
      hipLaunchKernelGGL((k_leapfrog4<TY, true, true>), grid, block, 0, st, p);
    else
      hipLaunchKernelGGL((k_leapfrog4<TY, true, false>), grid, block, 0, st, p);
  } else {
    if (nt)
      hipLaunchKernelGGL((k_leapfrog4<TY, false, true>), grid, block, 0, st, p);
    else
      hipLaunchKernelGGL((k_leapfrog4<TY, false, false>), grid, block, 0, st, p);
  }
}

}  // namespace

int leapfrog4_ty(const LeapfrogTiling& t) { return t.ty >= 16 ? 16 : 8; }

int leapfrog4_blocks(const Layout& l, const LBox* boxes, int nbox, const LeapfrogTiling& t, int min_chunk) {
  return make_plan4(l, boxes, nbox, t, min_chunk).nblocks;
}

void launch_leapfrog4(const Layout& l, const Coeffs& c, const double* cur, double* old_out, const LBox* boxes, int nbox,
                      const double* d_s, double ct, Partial* partials, const LeapfrogTiling& t, hipStream_t stream,
                      int min_chunk) {
  W3D_REQUIRE(c.order == 4, "order: launch_leapfrog4 takes the coefficients of an order = 4 problem");
  Plan4 pl = make_plan4(l, boxes, nbox, t, min_chunk);
  if (pl.nblocks == 0) return;
  Lf4Params& p = pl.prm;
  p.cur = cur + l.kbase();
  p.out = old_out + l.kbase();
  p.s = d_s;
  p.partials = partials;
  p.lam = c.lam;
  p.ry = c.ry;
  p.rz = c.rz;
  p.ct = ct;
  const bool check = partials != nullptr;
  if (leapfrog4_ty(t) == 16)
    launch4_ty<16>(p, pl.nblocks, check, t.nt_store, stream);
  else
    launch4_ty<8>(p, pl.nblocks, check, t.nt_store, stream);
  W3D_HIP_CHECK(hipGetLastError());
}

}  // namespace wave3d
