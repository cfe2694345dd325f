// k_leapfrog_p2 rectangular-box instantiations (BOX = true) for S = 5 (normal passes only, as for the cube).
// Design: kernels_leapfrog_p2.hip.
#include "wave3d/leapfrog_p2_launch.hpp"

namespace wave3d {
namespace p2k {

void launch_p2_box_s5(const P2Params& p, int nblocks, bool init, hipStream_t st) {
  W3D_REQUIRE(!init, "leapfrog_p2: the analytic-start pass takes at most 4 steps");
  launch_cm<5, false, true>(p, nblocks, st);
}
void prepare_p2_box_s5() { prepare_all<5, false, true>(); }

}  // namespace p2k
}  // namespace wave3d
