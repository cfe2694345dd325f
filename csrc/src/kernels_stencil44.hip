// Fourth order in time (Problem::time_order = 4): k_lap4, k_leapfrog44 and the first step k_first_step_t4. See
// wave3d/kernels.hpp for the interface and stencil.hpp leapfrog_t4 / first_step_t4 for the scheme.
//
// A step is two launches, each one application of the fourth-order operator (stencil.hpp d4sum_t):
//   k_lap4        v = lam·s(u^n) on the interior nodes of its boxes; it reads u^n and stores v, nothing else.
//   k_leapfrog44  u^{n+1} = leapfrog_t4(u^n, u^{n−1}, v, s(v), lam12), u^{n−1} read in place and overwritten.
// Both march exactly as k_leapfrog4 does (kernels_stencil4.hip; the march is duplicated here so that file and its
// kernels stay as they are): a workgroup owns a (TY rows × 64 pairs) tile of the (y, z) plane and marches along x, a
// five-deep register queue of the thread's own column, a double-buffered LDS tile with a halo of two rows and one pair,
// one barrier per plane, walls by select in registers. In k_lap4 the queue and the tile hold u^n, in k_leapfrog44 they
// hold v; k_leapfrog44 also reads the centre pair of u^n and of u^{n−1}. v's six faces are exact zeros (the buffer is
// zeroed once and only k_lap4 writes it, interior nodes only) and beyond a wall v is −v of the mirror node, by the same
// select as for u: the ghost layer, the row padding and the planes −1 and N + 1 of u, u^{n−1} and v are never used as
// data. Compulsory traffic: 16 B (k_lap4) + 32 B (k_leapfrog44) = 48 B per node and step.
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

struct Tile44Box {
  i64 x0, x1;    // local x range
  i64 y0, y1;    // local y range
  i64 zo0, zo1;  // row-offset range of the updated nodes
  i64 pz0, pz_end;
  int ntz, nty, xchunk, tile_begin;
};

struct Lf44Params {
  const double* q;  // the marched field: u^n (k_lap4) or v (k_leapfrog44)
  const double* u;  // k_leapfrog44: u^n, centre values only
  double* out;      // k_lap4: v; k_leapfrog44: u^{n−1} in, u^{n+1} out
  const double* s;
  Partial* partials;
  i64 plane, pitch, gx0, gy0, gz0, zs, N;
  double coef, ct;  // coef: lam (k_lap4) or lam12 = lam/12 (k_leapfrog44), the coefficient of d4sum_t
  double ry, rz;    // rectangular box: h_x²/h_y², h_x²/h_z² (1 for a cube: the cube form's bits)
  int nbox, ntiles, nblocks, xcd_remap;
  Tile44Box box[kMaxBoxes];
};

__device__ __forceinline__ v2d neg2(v2d v) {
  v2d r;
  r.x = -v.x;
  r.y = -v.y;
  return r;
}

// The march of both kernels. LAP: out = lap_t4(s(q), coef), no other field is read (CHECK and NT are off). Otherwise:
// out = leapfrog_t4(u, out, q, s(q), coef) with k_leapfrog4's error epilogue.
template <int TY, bool LAP, bool CHECK, bool NT>
__device__ __forceinline__ void march44(const Lf44Params& p) {
  // halo slots: 2·64 pairs above, 2·64 below, TY left, TY right — one per thread
  static_assert(4 * kLanes + 2 * TY <= kLanes * TY, "halo slots need at least 256 + 2*TY threads (TY >= 5)");
  static_assert(!LAP || (!CHECK && !NT), "k_lap4 has no check and stores v for the next launch to read");
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
  Tile44Box B = p.box[0];
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
    if (!LAP) {
      uc = ld2(u + px + my);
      uo = ld2(out + px + my);
    }
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
        if (!LAP) {
          uc_n = ld2(u + px + plane + my);
          uo_n = ld2(out + px + plane + my);
        }
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
      if (LAP) {
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

template <int TY>
__global__ __launch_bounds__(kLanes* TY) void k_lap4(const Lf44Params p) {
  march44<TY, true, false, false>(p);
}

template <int TY, bool CHECK, bool NT>
__global__ __launch_bounds__(kLanes* TY) void k_leapfrog44(const Lf44Params p) {
  march44<TY, false, CHECK, NT>(p);
}

// The first step's second half, once per solve: one thread per interior node, written for clarity. u0 = φ and v =
// lam·s(φ) (k_lap4 on u0) are in the solve layout, ψ in the source layout (one ghost layer more). Every address read is
// a node of the global grid: a distance-2 neighbour outside it is −centre.
struct FirstT4Params {
  Layout l, src;
  const double* u0;
  const double* v;
  const double* psi;
  double* u1;
  double lam24, lam6, tau, ry, rz;
};

__device__ __forceinline__ double s4_node(const double* f, i64 P, i64 R, i64 gx, i64 gy, i64 gz, i64 N, double ry,
                                          double rz) {
  const double c = f[0];
  return d4sum_t<true>(c, gx == 1 ? -c : f[-2 * P], f[-P], f[P], gx == N - 1 ? -c : f[2 * P], gy == 1 ? -c : f[-2 * R],
                       f[-R], f[R], gy == N - 1 ? -c : f[2 * R], gz == 1 ? -c : f[-2], f[-1], f[1],
                       gz == N - 1 ? -c : f[2], ry, rz);
}

__global__ __launch_bounds__(256) void k_first_step_t4(const FirstT4Params p) {
  const i64 N = p.l.N;
  // (the layout spans the domain: local indices are global ones)
  const i64 gz = 1 + static_cast<i64>(blockIdx.x) * 256 + threadIdx.x, gy = 1 + blockIdx.y, gx = 1 + blockIdx.z;
  if (gz >= N || gy >= N || gx >= N) return;
  const i64 o = p.l.off(gx, gy, gz);
  const double sv = s4_node(p.v + o, p.l.plane, p.l.pitch, gx, gy, gz, N, p.ry, p.rz);
  double w = first_step_t4(p.u0[o], p.v[o], sv, p.lam24);
  if (p.psi) {
    const double* f = p.psi + p.src.off(gx, gy, gz);
    w = first_step_t4_psi(w, f[0], s4_node(f, p.src.plane, p.src.pitch, gx, gy, gz, N, p.ry, p.rz), p.lam6, p.tau);
  }
  p.u1[o] = w;
}

struct Plan44 {
  Lf44Params prm;
  int nblocks;
};

// k_leapfrog4's tiling (kernels_stencil4.hip make_plan4, duplicated with the march): one tile per workgroup, x chunks
// spread over the boxes by work, the chunk floor an argument.
Plan44 make_plan44(const Layout& l, const LBox* boxes, int nbox, const LeapfrogTiling& t, int min_chunk) {
  W3D_REQUIRE(nbox >= 0 && nbox <= kMaxBoxes, "too many boxes in one leapfrog launch");
  W3D_REQUIRE(min_chunk >= 1, "time_order: the x chunk floor must be >= 1");
  W3D_REQUIRE(l.nx == l.N + 1 && l.ny == l.N + 1 && l.nz == l.N + 1 && l.xg >= 1 && l.yg >= 1 && l.zg >= 1,
              "time_order: the fourth-order step needs one rank's layout that spans the whole domain");
  const int ty = leapfrog4_ty(t);
  Plan44 pl{};
  Lf44Params& p = pl.prm;
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
    Tile44Box& tb = p.box[nb];
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
void launch44_ty(const Lf44Params& p, int nblocks, bool check, bool nt, hipStream_t st) {
  const dim3 block(kLanes, TY), grid(nblocks);
  if (check) {
    if (nt)
      hipLaunchKernelGGL((k_leapfrog44<TY, true, true>), grid, block, 0, st, p);
    else
      hipLaunchKernelGGL((k_leapfrog44<TY, true, false>), grid, block, 0, st, p);
  } else {
    if (nt)
      hipLaunchKernelGGL((k_leapfrog44<TY, false, true>), grid, block, 0, st, p);
    else
      hipLaunchKernelGGL((k_leapfrog44<TY, false, false>), grid, block, 0, st, p);
  }
}

void require_t4(const Coeffs& c) {
  W3D_REQUIRE(c.time_order == 4 && c.order == 4, "time_order: the coefficients of a time_order = 4 problem are needed");
}

}  // namespace

int leapfrog44_blocks(const Layout& l, const LBox* boxes, int nbox, const LeapfrogTiling& t, int min_chunk) {
  return make_plan44(l, boxes, nbox, t, min_chunk).nblocks;
}

void launch_lap4(const Layout& l, const Coeffs& c, const double* u, double* v, const LBox* boxes, int nbox,
                 const LeapfrogTiling& t, hipStream_t stream, int min_chunk) {
  require_t4(c);
  Plan44 pl = make_plan44(l, boxes, nbox, t, min_chunk);
  if (pl.nblocks == 0) return;
  Lf44Params& p = pl.prm;
  p.q = u + l.kbase();
  p.u = nullptr;
  p.out = v + l.kbase();
  p.s = nullptr;
  p.partials = nullptr;
  p.coef = c.lam;
  p.ry = c.ry;
  p.rz = c.rz;
  p.ct = 0.0;
  if (leapfrog4_ty(t) == 16)
    hipLaunchKernelGGL(k_lap4<16>, dim3(pl.nblocks), dim3(kLanes, 16), 0, stream, p);
  else
    hipLaunchKernelGGL(k_lap4<8>, dim3(pl.nblocks), dim3(kLanes, 8), 0, stream, p);
  W3D_HIP_CHECK(hipGetLastError());
}

void launch_leapfrog44(const Layout& l, const Coeffs& c, const double* cur, const double* v, double* old_out,
                       const LBox* boxes, int nbox, const double* d_s, double ct, Partial* partials,
                       const LeapfrogTiling& t, hipStream_t stream, int min_chunk) {
  require_t4(c);
  Plan44 pl = make_plan44(l, boxes, nbox, t, min_chunk);
  if (pl.nblocks == 0) return;
  Lf44Params& p = pl.prm;
  p.q = v + l.kbase();
  p.u = cur + l.kbase();
  p.out = old_out + l.kbase();
  p.s = d_s;
  p.partials = partials;
  p.coef = c.lam12;
  p.ry = c.ry;
  p.rz = c.rz;
  p.ct = ct;
  const bool check = partials != nullptr;
  if (leapfrog4_ty(t) == 16)
    launch44_ty<16>(p, pl.nblocks, check, t.nt_store, stream);
  else
    launch44_ty<8>(p, pl.nblocks, check, t.nt_store, stream);
  W3D_HIP_CHECK(hipGetLastError());
}

void launch_first_step_t4(const Layout& l, const Layout& src, const Coeffs& c, double tau, const double* phi,
                          const double* psi, double* v, double* u0, double* u1, const LeapfrogTiling& t,
                          hipStream_t stream) {
  require_t4(c);
  // u⁰ = φ over the whole allocation and zeros in u¹ outside the interior, as the (4, 2) start stores them (its u¹ on
  // the interior is replaced below); then v = lam·s(φ), then u¹
  launch_first_step_field(l, src, c, tau, phi, nullptr, u0, u1, stream);
  const LBox full{l.cx0, l.cx1, l.cy0, l.cy1, l.cz0, l.cz1};
  launch_lap4(l, c, u0, v, &full, 1, t, stream);
  if (full.empty()) return;
  W3D_REQUIRE(l.gx0 == 0 && l.gy0 == 0 && l.gz0 == 0 && l.N - 1 <= 65535, "time_order: the first step needs one rank's "
                                                                          "layout that spans the domain, N <= 65536");
  FirstT4Params p;
  p.l = l;
  p.src = src;
  p.u0 = u0;
  p.v = v;
  p.psi = psi;
  p.u1 = u1;
  p.lam24 = c.lam24;
  p.lam6 = c.lam6;
  p.tau = tau;
  p.ry = c.ry;
  p.rz = c.rz;
  const dim3 grid(static_cast<unsigned>(ceil_div(l.N - 1, 256)), static_cast<unsigned>(l.N - 1),
                  static_cast<unsigned>(l.N - 1));
  hipLaunchKernelGGL(k_first_step_t4, grid, dim3(256), 0, stream, p);
  W3D_HIP_CHECK(hipGetLastError());
}

}  // namespace wave3d
