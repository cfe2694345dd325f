// Point sources: u_tt = Δu + Σ_q w_q(t) δ(x − x_q). See wave3d/kernels.hpp for the interface.
//
// The leapfrog update is linear, so a pass of s steps n → n + s with a forcing term equals the same pass without it
// plus the response of a ZERO field to the forcing alone. That response depends on the source node, the addends
// a[n .. n + s) and Coeffs only, and is non-zero only within L1 distance s − 1 (level n + s) / s − 2 (level n + s − 1)
// of the node. k_source_cone computes it in LDS and adds it to the pass's two stored levels; the pass kernels are not
// involved.
//
//   k_source_cone : one workgroup per source of one colour class (schedule.hpp plan_sources: the balls of a class are
//                   disjoint, so the field update is plain loads, adds and stores — no atomics). Two zeroed 11³ level
//                   buffers; step k = 1..s advances the ball of radius k − 1 with stencil.hpp's d2sum_t / leapfrog in
//                   cpu_leapfrog's argument order and then adds a[n + k − 1][slot] at the centre (the start level: ½·a[0]):
//                   bit-identical to cpu_source_response. With receivers, level k's value at every owned receiver within
//                   distance k − 1 is added to trace row n + k (k_record_cone recomputed those rows without forcing).
//                   With s = 1 the ball is the node and the kernel is out0[node] += a: the CPU definition itself.
//
// Nodes on or outside the global boundary are never computed (their LDS cells keep +0.0) and never written. The source
// node may lie outside the rank's allocation (a neighbour's source whose ball reaches into this rank's ghost planes):
// every ball node is tested against the allocation's index range before its offset is used, so nothing outside the
// allocation is addressed.
//
// Resource use (gfx950, -Rpass-analysis=kernel-resource-usage): k_source_cone<false> 30 VGPRs, <true> 28 VGPRs, no
// scratch, 21296 B LDS each (two 11³ level buffers).
#include <hip/hip_runtime.h>

#include "wave3d/device_util.hpp"
#include "wave3d/kernels.hpp"
#include "wave3d/stencil.hpp"

namespace wave3d {

namespace {

constexpr int kSrcThreads = 256;
constexpr int kSrcMaxSteps = 5;
constexpr int kSrcSide = 2 * kSrcMaxSteps + 1;                // LDS cube edge (fixed stride for every s)
constexpr int kSrcCells = kSrcSide * kSrcSide * kSrcSide;     // 1331 doubles per level

struct SourceParams {
  double* out0;         // u^{n+s}
  double* out1;         // u^{n+s−1}
  const Source* table;  // this class's sources
  const double* a;      // [K][Q]
  i64 Q;
  const Receiver* rtable;  // owned receivers (rcount = 0: none)
  double* trace;
  i64 rtotal;
  int rcount;
  i64 plane, pitch, N, gx0, gy0, gz0;
  i64 x0, x1, y0, y1, z0, z1;  // the allocation's local node range, half-open
  int n, steps, start;
  double lam, ry, rz;
};

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

template <bool BOX>
__global__ __launch_bounds__(kSrcThreads) void k_source_cone(const SourceParams p) {
  __shared__ double lv[2][kSrcCells];
  const Source sc = p.table[blockIdx.x];
  const int s = p.steps, r = s - 1, side = 2 * r + 1, cells = side * side * side;
  const int tid = static_cast<int>(threadIdx.x);
  for (int i = tid; i < 2 * kSrcCells; i += kSrcThreads) (&lv[0][0])[i] = 0.0;
  __syncthreads();
  const i64 gx = p.gx0 + sc.x, gy = p.gy0 + sc.y, gz = p.gz0 + sc.z;
  // cell (a, b, c) ∈ [−r, r]³ of the source's neighbourhood: whether its node is inside the global interior
  auto interior = [&](int a, int b, int c) {
    return gx + a > 0 && gx + a < p.N && gy + b > 0 && gy + b < p.N && gz + c > 0 && gz + c < p.N;
  };
  constexpr int kC = kSrcMaxSteps;
  auto cell = [](int a, int b, int c) { return ((a + kC) * kSrcSide + (b + kC)) * kSrcSide + (c + kC); };
  int io = 0, ic = 1;
  for (int k = 1; k <= s; ++k) {
    // level k on the ball of radius k − 1, over level k − 2 (which nothing reads again)
    const double* cu = lv[ic];
    double* out = lv[io];
    for (int i = tid; i < cells; i += kSrcThreads) {
      const int a = i / (side * side) - r, b = (i / side) % side - r, c = i % side - r;
      if (iabs(a) + iabs(b) + iabs(c) > k - 1 || !interior(a, b, c)) continue;
      const int q = cell(a, b, c);
      const double u = cu[q];
      const double lap = d2sum_t<BOX>(u, cu[q - kSrcSide * kSrcSide], cu[q + kSrcSide * kSrcSide], cu[q - kSrcSide],
                                      cu[q + kSrcSide], cu[q - 1], cu[q + 1], p.ry, p.rz);
      out[q] = leapfrog(u, out[q], lap, p.lam);
    }
    __syncthreads();
    if (tid == 0) {
      const double a = p.a[static_cast<i64>(p.n + k - 1) * p.Q + sc.slot];
      out[cell(0, 0, 0)] += p.start ? 0.5 * a : a;
    }
    __syncthreads();
    // receivers: level n + k at every owned receiver inside this level's ball (a scan of the table per level)
    for (int i = tid; i < p.rcount; i += kSrcThreads) {
      const Receiver rc = p.rtable[i];
      const i64 dx = rc.x - sc.x, dy = rc.y - sc.y, dz = rc.z - sc.z;
      const i64 dist = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz);
      if (dist > k - 1) continue;
      p.trace[static_cast<i64>(p.n + k) * p.rtotal + rc.slot] +=
          out[cell(static_cast<int>(dx), static_cast<int>(dy), static_cast<int>(dz))];
    }
    const int t = io;
    io = ic;
    ic = t;
  }
  // lv[ic] = r^{n+s} (radius s − 1), lv[io] = r^{n+s−1} (radius s − 2): added to the stored levels on the nodes of the
  // ball that lie inside the global interior and inside this rank's allocation
  const double* last = lv[ic];
  const double* prev = lv[io];
  for (int i = tid; i < cells; i += kSrcThreads) {
    const int a = i / (side * side) - r, b = (i / side) % side - r, c = i % side - r;
    const int dist = iabs(a) + iabs(b) + iabs(c);
    if (dist > r || !interior(a, b, c)) continue;
    const i64 x = sc.x + a, y = sc.y + b, z = sc.z + c;
    if (x < p.x0 || x >= p.x1 || y < p.y0 || y >= p.y1 || z < p.z0 || z >= p.z1) continue;
    const i64 o = sc.off + a * p.plane + b * p.pitch + c;
    const int q = cell(a, b, c);
    p.out0[o] += last[q];
    if (dist < r) p.out1[o] += prev[q];
  }
}

}  // namespace

void launch_source_cone(const Layout& l, const Coeffs& c, double* out_prev, double* out_last, int n, int steps, bool start,
                        const Source* table, const int* class_begin, int classes, const double* a, i64 Q,
                        const Receiver* rtable, int rcount, double* trace, i64 rtotal, hipStream_t stream) {
  W3D_REQUIRE(steps >= 1 && steps <= kSrcMaxSteps, "source_cone: 1..5 steps");
  W3D_REQUIRE(out_prev != nullptr && out_last != nullptr, "source_cone: both output levels are needed (a pass that "
                                                          "drops u^{n+s-1} cannot be corrected)");
  W3D_REQUIRE(start ? (n == 0 && steps == 1) : n >= 1, "source_cone: the start is the one step 0 -> 1; a pass starts at n >= 1");
  W3D_REQUIRE(rcount == 0 || (rtable != nullptr && trace != nullptr && !start), "source_cone: bad receiver arguments");
  // the rank's ghost planes receive the same correction as their owners' nodes: they must be as deep as the pass
  const i64 g[3] = {l.xg, l.yg, l.zg}, g0[3] = {l.gx0, l.gy0, l.gz0}, ext[3] = {l.nx, l.ny, l.nz};
  for (int k = 0; k < 3; ++k)
    W3D_REQUIRE(g[k] >= steps || (g0[k] == 0 && ext[k] == l.N + 1),
                "source_cone: a pass of " + std::to_string(steps) + " steps needs ghosts that deep on every split axis");
  SourceParams p;
  p.out0 = out_last;
  p.out1 = out_prev;
  p.a = a;
  p.Q = Q;
  p.rtable = rtable;
  p.trace = trace;
  p.rtotal = rtotal;
  p.rcount = rcount;
  p.plane = l.plane;
  p.pitch = l.pitch;
  p.N = l.N;
  p.gx0 = l.gx0;
  p.gy0 = l.gy0;
  p.gz0 = l.gz0;
  p.x0 = -l.xg;
  p.x1 = l.nx + l.xg;
  p.y0 = -l.yg;
  p.y1 = l.ny + l.yg;
  p.z0 = -l.zg;
  p.z1 = l.nz + l.zg;
  p.n = n;
  p.steps = steps;
  p.start = start ? 1 : 0;
  p.lam = c.lam;
  p.ry = c.ry;
  p.rz = c.rz;
  for (int k = 0; k < classes; ++k) {  // one launch per colour class, in class order
    const int count = class_begin[k + 1] - class_begin[k];
    if (count <= 0) continue;
    p.table = table + class_begin[k];
    if (c.box)
      hipLaunchKernelGGL(k_source_cone<true>, dim3(static_cast<unsigned>(count)), dim3(kSrcThreads), 0, stream, p);
    else
      hipLaunchKernelGGL(k_source_cone<false>, dim3(static_cast<unsigned>(count)), dim3(kSrcThreads), 0, stream, p);
    W3D_HIP_CHECK(hipGetLastError());
  }
}

}  // namespace wave3d
