// k_leapfrog_tb rectangular-box instantiations (BOX = true): the Laplacian of every stage and of the analytic start is
// stencil.hpp::d2sum_box. Same S, workgroup sizes, check masks and chunk variants as kernels_leapfrog_tb.hip, which
// keeps the cube's. Design: kernels_leapfrog_tb.hip.
#include "wave3d/leapfrog_tb_kernel.hpp"

namespace wave3d {
namespace tbk {

void launch_box(const TbParams& p, int nblocks, const LeapfrogTbTiling& t, bool init, hipStream_t st) {
  switch (t.stages) {
    case 2: launch_s<2, false, true>(p, nblocks, t, init, st); break;
    case 3: launch_s<3, false, true>(p, nblocks, t, init, st); break;
    default: launch_s<4, false, true>(p, nblocks, t, init, st); break;
  }
}

void prepare_box() {
  prepare_nt<2, 768, false, false, true>();
  prepare_nt<3, 768, false, false, true>();
  prepare_nt<4, 768, false, false, true>();
  prepare_nt<2, 768, true, false, true>();
  prepare_nt<3, 768, true, false, true>();
  prepare_nt<4, 768, true, false, true>();
  prepare_nt<2, 1024, false, false, true>();
  prepare_nt<3, 1024, false, false, true>();
  prepare_nt<4, 1024, false, false, true>();
  prepare_nt<2, 1024, true, false, true>();
  prepare_nt<3, 1024, true, false, true>();
  prepare_nt<4, 1024, true, false, true>();
}

}  // namespace tbk
}  // namespace wave3d
