// k_leapfrog_p2 speed-field instantiations (VARC = true: a coefficient lamf = lam c^2 per node) for S = 2, cube and
// rectangular box, load passes only (a speed solve has a stored start). Design: leapfrog_p2_kernel.hpp, measurements:
// profiles/speed_fused/.
#include "wave3d/leapfrog_p2_launch.hpp"

namespace wave3d {
namespace p2k {

void launch_p2_varc_s2(const P2Params& p, int nblocks, bool box, hipStream_t st) {
  box ? launch_cm<2, false, true, true>(p, nblocks, st) : launch_cm<2, false, false, true>(p, nblocks, st);
}
void prepare_p2_varc_s2() {
  prepare_all<2, false, false, true>();
  prepare_all<2, false, true, true>();
}

}  // namespace p2k
}  // namespace wave3d
