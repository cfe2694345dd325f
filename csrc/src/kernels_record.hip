// Receivers: the value u^n at chosen grid nodes for every level of a solve. See wave3d/kernels.hpp for the interface.
//
//   k_record_gather : trace[n][slot] = field[off] for every receiver of the table — a level that is stored in memory
//                     (the start levels, the output of a single-step unit).
//   k_record_cone   : the s = 2..5 levels a fused pass produces, of which only the last two ever reach memory. u^{n+k}
//                     at node p depends on u^n within L1 distance k of p and on u^{n−1} within distance k − 1, so the s
//                     centre values follow from the pass's INPUTS on the L1 ball of radius s (u^n) / s − 1 (u^{n−1}):
//                     exactly the ghost depth a pass of s steps is given. One workgroup per receiver loads that ball into
//                     LDS, advances it s times on the shrinking ball with stencil.hpp's d2sum_t / leapfrog in
//                     cpu_leapfrog's argument order (bit-identical to the CPU steps, hence to the passes), and stores
//                     the centre value of every level. The pass kernels are not involved.
//
// Nodes on or outside the global boundary are never read and never computed: their LDS cells keep the +0.0 both level
// buffers start with. Only ball nodes are read (never the enclosing cube): the launcher checks that the ball of
// every owned node lies inside the rank's allocation — ghost depth ≥ s on an axis, or the rank spans the whole axis, where
// everything beyond the owned range is outside the global grid.
//
// Resource use (gfx950, -Rpass-analysis=kernel-resource-usage): k_record_cone<false> and <true> 32 VGPRs each, no
// scratch, 21296 B LDS (two 11³ level buffers); k_record_gather 6 VGPRs, no scratch, no LDS.
#include <hip/hip_runtime.h>

#include "wave3d/device_util.hpp"
#include "wave3d/kernels.hpp"
#include "wave3d/stencil.hpp"

namespace wave3d {

namespace {

constexpr int kConeThreads = 256;
constexpr int kConeMaxSteps = 5;
constexpr int kConeSide = 2 * kConeMaxSteps + 1;                  // LDS cube edge (fixed stride for every s)
constexpr int kConeCells = kConeSide * kConeSide * kConeSide;     // 1331 doubles per level

struct ConeParams {
  const double* prev;  // u^{n−1}
  const double* cur;   // u^n
  const Receiver* table;
  double* trace;
  i64 rtotal;          // trace row length
  i64 plane, pitch, N, gx0, gy0, gz0;
  int n, steps;
  double lam, ry, rz;
};

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

template <bool BOX>
__global__ __launch_bounds__(kConeThreads) void k_record_cone(const ConeParams p) {
  __shared__ double lv[2][kConeCells];
  const Receiver rc = p.table[blockIdx.x];
  const int s = p.steps, side = 2 * s + 1, cells = side * side * side;
  const int tid = static_cast<int>(threadIdx.x);
  for (int i = tid; i < 2 * kConeCells; i += kConeThreads) (&lv[0][0])[i] = 0.0;
  __syncthreads();
  const i64 gx = p.gx0 + rc.x, gy = p.gy0 + rc.y, gz = p.gz0 + rc.z;
  // cell (a, b, c) ∈ [−s, s]³ of the receiver's neighbourhood: whether its node is inside the global interior
  auto interior = [&](int a, int b, int c) {
    return gx + a > 0 && gx + a < p.N && gy + b > 0 && gy + b < p.N && gz + c > 0 && gz + c < p.N;
  };
  constexpr int kC = kConeMaxSteps;
  auto cell = [](int a, int b, int c) { return ((a + kC) * kConeSide + (b + kC)) * kConeSide + (c + kC); };
  // level 0 = u^n on the ball of radius s into lv[1], level −1 = u^{n−1} on radius s − 1 into lv[0]
  for (int i = tid; i < cells; i += kConeThreads) {
    const int a = i / (side * side) - s, b = (i / side) % side - s, c = i % side - s;
    const int dist = iabs(a) + iabs(b) + iabs(c);
    if (dist > s || !interior(a, b, c)) continue;
    const i64 o = rc.off + a * p.plane + b * p.pitch + c;
    lv[1][cell(a, b, c)] = p.cur[o];
    if (dist < s) lv[0][cell(a, b, c)] = p.prev[o];
  }
  __syncthreads();
  int io = 0, ic = 1;
  for (int k = 1; k <= s; ++k) {
    // level k on the ball of radius s − k, over level k − 2 (which nothing reads again)
    const double* cu = lv[ic];
    double* out = lv[io];
    for (int i = tid; i < cells; i += kConeThreads) {
      const int a = i / (side * side) - s, b = (i / side) % side - s, c = i % side - s;
      if (iabs(a) + iabs(b) + iabs(c) > s - k || !interior(a, b, c)) continue;
      const int q = cell(a, b, c);
      const double u = cu[q];
      const double lap = d2sum_t<BOX>(u, cu[q - kConeSide * kConeSide], cu[q + kConeSide * kConeSide], cu[q - kConeSide],
                                      cu[q + kConeSide], cu[q - 1], cu[q + 1], p.ry, p.rz);
      out[q] = leapfrog(u, out[q], lap, p.lam);
    }
    __syncthreads();
    if (tid == 0) p.trace[static_cast<i64>(p.n + k) * p.rtotal + rc.slot] = out[cell(0, 0, 0)];
    const int t = io;
    io = ic;
    ic = t;
  }
}

__global__ __launch_bounds__(256) void k_record_gather(const double* field, const Receiver* table, int count,
                                                       double* trace, i64 row, i64 rtotal) {
  const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
  if (i >= count) return;
  const Receiver rc = table[i];
  trace[row * rtotal + rc.slot] = field[rc.off];
}

}  // namespace

void launch_record_cone(const Layout& l, const Coeffs& c, const double* prev, const double* cur, int n, int steps,
                        const Receiver* table, int count, double* trace, i64 rtotal, hipStream_t stream) {
  W3D_REQUIRE(steps >= 2 && steps <= kConeMaxSteps, "record_cone: 2..5 steps");
  W3D_REQUIRE(n >= 1, "record_cone: the inputs are u^{n-1}, u^n with n >= 1");
  // the ball of radius `steps` around every owned node lies inside the allocation (or outside the global grid)
  const i64 g[3] = {l.xg, l.yg, l.zg}, g0[3] = {l.gx0, l.gy0, l.gz0}, ext[3] = {l.nx, l.ny, l.nz};
  for (int a = 0; a < 3; ++a)
    W3D_REQUIRE(g[a] >= steps || (g0[a] == 0 && ext[a] == l.N + 1),
                "record_cone: a pass of " + std::to_string(steps) + " steps needs ghosts that deep on every split axis");
  if (count <= 0) return;
  ConeParams p;
  p.prev = prev;
  p.cur = cur;
  p.table = table;
  p.trace = trace;
  p.rtotal = rtotal;
  p.plane = l.plane;
  p.pitch = l.pitch;
  p.N = l.N;
  p.gx0 = l.gx0;
  p.gy0 = l.gy0;
  p.gz0 = l.gz0;
  p.n = n;
  p.steps = steps;
  p.lam = c.lam;
  p.ry = c.ry;
  p.rz = c.rz;
  if (c.box)
    hipLaunchKernelGGL(k_record_cone<true>, dim3(static_cast<unsigned>(count)), dim3(kConeThreads), 0, stream, p);
  else
    hipLaunchKernelGGL(k_record_cone<false>, dim3(static_cast<unsigned>(count)), dim3(kConeThreads), 0, stream, p);
  W3D_HIP_CHECK(hipGetLastError());
}

void launch_record_gather(const double* field, int n, const Receiver* table, int count, double* trace, i64 rtotal,
                          hipStream_t stream) {
  W3D_REQUIRE(n >= 0, "record_gather: level below 0");
  if (count <= 0) return;
  hipLaunchKernelGGL(k_record_gather, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, stream, field, table,
                     count, trace, static_cast<i64>(n), rtotal);
  W3D_HIP_CHECK(hipGetLastError());
}

}  // namespace wave3d
