// Fourth-order single step (Problem::order = 4): k_leapfrog4. See wave3d/kernels.hpp for the interface, stencil.hpp
// d4sum_t for the operator and wave3d/leapfrog4_kernel.hpp for the march.
//
// k_leapfrog4 is the march with u^n as the marched field (March4::Step42): the register queue and the LDS tile hold u^n,
// the queue centre is the node's own value, u^{n−1} is read in place and u^{n+1} written over it; 24 B/node/step of
// compulsory traffic, as the second-order step.
#include <hip/hip_runtime.h>

#include "wave3d/kernels.hpp"
#include "wave3d/leapfrog4_kernel.hpp"

namespace wave3d {

namespace {

template <int TY, bool CHECK, bool NT>
__global__ __launch_bounds__(kLanes* TY) void k_leapfrog4(const March4Params p) {
  march4<TY, March4::Step42, CHECK, NT>(p);
}

}  // namespace

int leapfrog4_ty(const LeapfrogTiling& t) { return t.ty >= 16 ? 16 : 8; }

int leapfrog4_blocks(const Layout& l, const LBox* boxes, int nbox, const LeapfrogTiling& t, int min_chunk) {
  return make_plan4(l, boxes, nbox, t, min_chunk, "order: ").g.nblocks;
}

void launch_leapfrog4(const Layout& l, const Coeffs& c, const double* cur, double* old_out, const LBox* boxes, int nbox,
                      const double* d_s, double ct, Partial* partials, const LeapfrogTiling& t, hipStream_t stream,
                      int min_chunk) {
  W3D_REQUIRE(c.order == 4, "order: launch_leapfrog4 takes the coefficients of an order = 4 problem");
  March4Params p = make_plan4(l, boxes, nbox, t, min_chunk, "order: ");
  if (p.g.nblocks == 0) return;
  p.q = cur + l.kbase();
  p.u = nullptr;
  p.out = old_out + l.kbase();
  p.s = d_s;
  p.partials = partials;
  p.coef = c.lam;  // τ²/(12h²): the coefficient of d4sum_t
  p.ry = c.ry;
  p.rz = c.rz;
  p.ct = ct;
  launch4_ty(leapfrog4_ty(t), partials != nullptr, t.nt_store, [&](auto TY, auto CHECK, auto NT) {
    hipLaunchKernelGGL((k_leapfrog4<TY.value, CHECK.value, NT.value>), dim3(p.g.nblocks), dim3(kLanes, TY.value), 0,
                       stream, p);
  });
  W3D_HIP_CHECK(hipGetLastError());
}

}  // namespace wave3d
