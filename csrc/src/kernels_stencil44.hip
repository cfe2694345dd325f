// Fourth order in time (Problem::time_order = 4): k_lap4, k_leapfrog44 and the first step k_first_step_t4. See
// wave3d/kernels.hpp for the interface, stencil.hpp leapfrog_t4 / first_step_t4 for the scheme and
// wave3d/leapfrog4_kernel.hpp for the march.
//
// A step is two launches, each one march (one application of the fourth-order operator, stencil.hpp d4sum_t):
//   k_lap4        v = lam·s(u^n) on the interior nodes of its boxes; it reads u^n and stores v, nothing else (March4::Lap).
//   k_leapfrog44  u^{n+1} = leapfrog_t4(u^n, u^{n−1}, v, s(v), lam12), u^{n−1} read in place and overwritten
//                 (March4::Step44): the queue and the tile hold v, and the centre pair of u^n is one more load per plane.
// v's six faces are exact zeros (the buffer is zeroed once and only k_lap4 writes it, interior nodes only) and beyond a
// wall v is −v of the mirror node, by the same select as for u: the ghost layer, the row padding and the planes −1 and
// N + 1 of u, u^{n−1} and v are never used as data. Compulsory traffic: 16 B (k_lap4) + 32 B (k_leapfrog44) = 48 B per
// node and step.
#include <hip/hip_runtime.h>

#include "wave3d/kernels.hpp"
#include "wave3d/leapfrog4_kernel.hpp"

namespace wave3d {

namespace {

template <int TY>
__global__ __launch_bounds__(kLanes* TY) void k_lap4(const March4Params p) {
  march4<TY, March4::Lap, false, false>(p);
}

template <int TY, bool CHECK, bool NT>
__global__ __launch_bounds__(kLanes* TY) void k_leapfrog44(const March4Params p) {
  march4<TY, March4::Step44, CHECK, NT>(p);
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

void require_t4(const Coeffs& c) {
  W3D_REQUIRE(c.time_order == 4 && c.order == 4, "time_order: the coefficients of a time_order = 4 problem are needed");
}

}  // namespace

int leapfrog44_blocks(const Layout& l, const LBox* boxes, int nbox, const LeapfrogTiling& t, int min_chunk) {
  return make_plan4(l, boxes, nbox, t, min_chunk, "time_order: ").g.nblocks;
}

void launch_lap4(const Layout& l, const Coeffs& c, const double* u, double* v, const LBox* boxes, int nbox,
                 const LeapfrogTiling& t, hipStream_t stream, int min_chunk) {
  require_t4(c);
  March4Params p = make_plan4(l, boxes, nbox, t, min_chunk, "time_order: ");
  if (p.g.nblocks == 0) return;
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
    hipLaunchKernelGGL(k_lap4<16>, dim3(p.g.nblocks), dim3(kLanes, 16), 0, stream, p);
  else
    hipLaunchKernelGGL(k_lap4<8>, dim3(p.g.nblocks), dim3(kLanes, 8), 0, stream, p);
  W3D_HIP_CHECK(hipGetLastError());
}

void launch_leapfrog44(const Layout& l, const Coeffs& c, const double* cur, const double* v, double* old_out,
                       const LBox* boxes, int nbox, const double* d_s, double ct, Partial* partials,
                       const LeapfrogTiling& t, hipStream_t stream, int min_chunk) {
  require_t4(c);
  March4Params p = make_plan4(l, boxes, nbox, t, min_chunk, "time_order: ");
  if (p.g.nblocks == 0) return;
  p.q = v + l.kbase();
  p.u = cur + l.kbase();
  p.out = old_out + l.kbase();
  p.s = d_s;
  p.partials = partials;
  p.coef = c.lam12;
  p.ry = c.ry;
  p.rz = c.rz;
  p.ct = ct;
  launch4_ty(leapfrog4_ty(t), partials != nullptr, t.nt_store, [&](auto TY, auto CHECK, auto NT) {
    hipLaunchKernelGGL((k_leapfrog44<TY.value, CHECK.value, NT.value>), dim3(p.g.nblocks), dim3(kLanes, TY.value), 0,
                       stream, p);
  });
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
