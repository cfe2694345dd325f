// k_leapfrog_p2 rectangular-box instantiations (BOX = true) for S = 3 (normal and analytic-start passes).
// Design: kernels_leapfrog_p2.hip.
#include "wave3d/leapfrog_p2_launch.hpp"

namespace wave3d {
namespace p2k {

void launch_p2_box_s3(const P2Params& p, int nblocks, bool init, hipStream_t st) {
  init ? launch_cm<3, true, true>(p, nblocks, st) : launch_cm<3, false, true>(p, nblocks, st);
}
void prepare_p2_box_s3() {
  prepare_all<3, false, true>();
  prepare_all<3, true, true>();
}

}  // namespace p2k
}  // namespace wave3d
