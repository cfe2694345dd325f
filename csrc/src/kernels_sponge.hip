// Sponge layers on the fused schedule. See wave3d/kernels.hpp (launch_sponge_box) for the interface.
//
// The LDS pass kernels know nothing of the sponge: a fused unit of s steps runs undamped, and its two stored outputs are
// wrong only within reach of the layers (cpu.hpp sponge_boxes: the slabs d < W + s − 1 from each damped face).
// k_sponge_box recomputes those slabs from the unit's INPUTS u^{n−1}, u^n with the damped operator and stores both
// levels over the pass's outputs. The four-buffer rotation keeps the inputs intact until the next pass (what
// k_record_cone relies on as well).
//
//   * One workgroup per 3-D tile of kTX × kTY × kTZ = 8 × 8 × 16 own nodes, with a halo of s nodes on every side.
//   * Two LDS arrays of the grown tile, (8 + 2s) × (8 + 2s) × (16 + 2s) doubles each (s = 5: 18 × 18 × 26, 134 784 B for the
//     two); level k + 1 overwrites level k − 1 in place (a cell reads only its own old value from that array). All s steps
//     happen in LDS, on the tile grown by s − k at step k, with stencil.hpp's d2sum_t / leapfrog / leapfrog_damped in
//     cpu_leapfrog's argument order: bit-identical to s damped CPU steps.
//   * Cells on or outside the global boundary are never read and never computed: they keep the +0.0 both arrays start
//     with. Reads are clipped to the own nodes grown by s (never the whole grown tile of a clipped edge tile).
//   * The 1-D sponge tables of the grown tile sit in LDS too; a node's g = max, r = min of its three entries.
//   * 512 threads = 16 rows × 32 z lanes: consecutive lanes hold consecutive z cells (conflict-free LDS phases, the grown
//     z extent ≤ 26 fits one row of lanes), rows of the (x, y) plane are dealt to the 16 lane rows.
//   * Both levels are stored in 16-byte pairs where both nodes of an aligned pair belong to the tile, single nodes at
//     odd tile ends.
#include <hip/hip_runtime.h>

#include "wave3d/device_util.hpp"
#include "wave3d/kernels.hpp"
#include "wave3d/stencil.hpp"

namespace wave3d {

namespace {

constexpr int kTX = 8, kTY = 8, kTZ = 16;  // own nodes of a tile
constexpr int kThreads = 512;
constexpr int kZLanes = 32, kRows = kThreads / kZLanes;
constexpr int kMaxSteps = 5;
constexpr int kTabLen = kTZ + 2 * kMaxSteps;  // the longest grown tile edge

struct SpongeBoxParams {
  const double* prev;  // u^{n−1}
  const double* cur;   // u^n
  double* out1;        // u^{n+s−1}
  double* out2;        // u^{n+s}
  SpongeView sp;       // device tables, global node index
  i64 plane, pitch, base;  // base = Layout::off(0, 0, 0)
  i64 N, gx0, gy0, gz0;
  i64 x0, x1, y0, y1, z0, z1;  // the box (local nodes)
  int ntx, nty, ntz;
  double lam, ry, rz;
};

template <int S, bool BOX>
__global__ __launch_bounds__(kThreads) void k_sponge_box(const SpongeBoxParams p) {
  constexpr int DX = kTX + 2 * S, DY = kTY + 2 * S, DZ = kTZ + 2 * S, CELLS = DX * DY * DZ;
  static_assert(DZ <= kZLanes, "a grown z row must fit one row of lanes");
  extern __shared__ double lds[];
  double* lv0 = lds;
  double* lv1 = lds + CELLS;
  double* tg = lds + 2 * CELLS;   // [3][kTabLen]: g along x, y, z of the grown tile
  double* tr = tg + 3 * kTabLen;  // ... and r

  const int tid = static_cast<int>(threadIdx.x);
  const int lz = tid & (kZLanes - 1), lr = tid >> 5;
  int t = static_cast<int>(blockIdx.x);
  const int tz = t % p.ntz;
  t /= p.ntz;
  const int ty = t % p.nty;
  const int tx = t / p.nty;
  // own nodes of this tile (local), clipped to the box
  const i64 ox0 = p.x0 + static_cast<i64>(tx) * kTX, ox1 = imin(ox0 + kTX, p.x1);
  const i64 oy0 = p.y0 + static_cast<i64>(ty) * kTY, oy1 = imin(oy0 + kTY, p.y1);
  const i64 oz0 = p.z0 + static_cast<i64>(tz) * kTZ, oz1 = imin(oz0 + kTZ, p.z1);
  // LDS cell (a, b, c) holds local node (ox0 − S + a, oy0 − S + b, oz0 − S + c); the global interior in cell coordinates
  const int ia0 = static_cast<int>(1 - p.gx0 - (ox0 - S)), ia1 = static_cast<int>(p.N - p.gx0 - (ox0 - S));
  const int ib0 = static_cast<int>(1 - p.gy0 - (oy0 - S)), ib1 = static_cast<int>(p.N - p.gy0 - (oy0 - S));
  const int ic0 = static_cast<int>(1 - p.gz0 - (oz0 - S)), ic1 = static_cast<int>(p.N - p.gz0 - (oz0 - S));
  const int ex = static_cast<int>(ox1 - ox0), ey = static_cast<int>(oy1 - oy0), ez = static_cast<int>(oz1 - oz0);
  auto lo = [](int own0, int grow, int int0) { return max(own0 - grow, int0); };
  auto hi = [](int own1, int grow, int int1) { return min(own1 + grow, int1); };

  for (int i = tid; i < 2 * CELLS; i += kThreads) lds[i] = 0.0;
  if (tid < 3 * kTabLen) {
    const int ax = tid / kTabLen, q = tid - ax * kTabLen;
    const i64 g = (ax == 0 ? p.gx0 + ox0 : (ax == 1 ? p.gy0 + oy0 : p.gz0 + oz0)) - S + q;
    const int len = ax == 0 ? DX : (ax == 1 ? DY : DZ);
    double gv = 0.0, rv = 1.0;
    if (q < len && g >= -1 && g <= p.N + 1) {
      gv = (ax == 0 ? p.sp.gx : (ax == 1 ? p.sp.gy : p.sp.gz))[g];
      rv = (ax == 0 ? p.sp.rx : (ax == 1 ? p.sp.ry : p.sp.rz))[g];
    }
    tg[tid] = gv;
    tr[tid] = rv;
  }
  __syncthreads();

  // u^n on the own nodes grown by S, u^{n−1} grown by S − 1, both clipped to the global interior
  {
    const int a0 = lo(S, S, ia0), a1 = hi(S + ex, S, ia1), b0 = lo(S, S, ib0), b1 = hi(S + ey, S, ib1);
    const int c0 = lo(S, S, ic0), c1 = hi(S + ez, S, ic1);
    const int pa0 = lo(S, S - 1, ia0), pa1 = hi(S + ex, S - 1, ia1), pb0 = lo(S, S - 1, ib0), pb1 = hi(S + ey, S - 1, ib1);
    const int pc0 = lo(S, S - 1, ic0), pc1 = hi(S + ez, S - 1, ic1);
    const int nb = b1 - b0, rows = (a1 - a0) * nb;
    const int c = c0 + lz;
    if (nb > 0 && c < c1) {
      for (int row = lr; row < rows; row += kRows) {
        const int a = a0 + row / nb, b = b0 + row % nb;
        const i64 o = p.base + (ox0 - S + a) * p.plane + (oy0 - S + b) * p.pitch + (oz0 - S + c);
        const int q = (a * DY + b) * DZ + c;
        lv1[q] = p.cur[o];
        if (a >= pa0 && a < pa1 && b >= pb0 && b < pb1 && c >= pc0 && c < pc1) lv0[q] = p.prev[o];
      }
    }
  }
  __syncthreads();

  double* cu = lv1;   // level k − 1
  double* out = lv0;  // level k − 2, overwritten by level k
#pragma unroll
  for (int k = 1; k <= S; ++k) {
    const int gr = S - k;
    const int a0 = lo(S, gr, ia0), a1 = hi(S + ex, gr, ia1), b0 = lo(S, gr, ib0), b1 = hi(S + ey, gr, ib1);
    const int c0 = lo(S, gr, ic0), c1 = hi(S + ez, gr, ic1);
    const int nb = b1 - b0, rows = (a1 - a0) * nb;
    const int c = c0 + lz;
    if (nb > 0 && c < c1) {
      const double gz = tg[2 * kTabLen + c], rz = tr[2 * kTabLen + c];
      for (int row = lr; row < rows; row += kRows) {
        const int a = a0 + row / nb, b = b0 + row % nb;
        const int q = (a * DY + b) * DZ + c;
        const double u = cu[q], old = out[q];
        const double lap = d2sum_t<BOX>(u, cu[q - DY * DZ], cu[q + DY * DZ], cu[q - DZ], cu[q + DZ], cu[q - 1], cu[q + 1],
                                        p.ry, p.rz);
        const double w = leapfrog(u, old, lap, p.lam);
        const double g = fmax(fmax(tg[a], tg[kTabLen + b]), gz);
        const double r = fmin(fmin(tr[a], tr[kTabLen + b]), rz);
        out[q] = leapfrog_damped(w, old, g, r);
      }
    }
    __syncthreads();
    double* sw = cu;
    cu = out;
    out = sw;
  }
  // cu = u^{n+S}, out = u^{n+S−1} on the own nodes: 16-byte pairs aligned in memory, single nodes at odd ends
  const i64 zoff = p.base + oz0;                 // in-row offset of the first own node
  const i64 zal = zoff & ~i64{1};                // ... rounded down to a pair
  const int npair = static_cast<int>((zoff + ez + 1 - zal) / 2);  // pairs that hold an own node (≤ 9)
  for (int i = tid; i < ex * ey * 16; i += kThreads) {
    const int pr = i & 15, b = (i >> 4) % ey, a = (i >> 4) / ey;
    if (pr >= npair) continue;
    const int e0 = static_cast<int>(zal - zoff) + 2 * pr;  // own z index of the pair's first node (−1: before the tile)
    const bool ok0 = e0 >= 0, ok1 = e0 + 1 < ez;
    const int q = ((S + a) * DY + (S + b)) * DZ + S + e0;
    const i64 o = (ox0 + a) * p.plane + (oy0 + b) * p.pitch + zal + 2 * pr;
    if (ok0 && ok1) {
      v2d v1, v2;
      v1.x = out[q];
      v1.y = out[q + 1];
      v2.x = cu[q];
      v2.y = cu[q + 1];
      *reinterpret_cast<v2d*>(p.out1 + o) = v1;
      *reinterpret_cast<v2d*>(p.out2 + o) = v2;
    } else if (ok0) {
      p.out1[o] = out[q];
      p.out2[o] = cu[q];
    } else if (ok1) {
      p.out1[o + 1] = out[q + 1];
      p.out2[o + 1] = cu[q + 1];
    }
  }
}

template <int S>
constexpr size_t lds_bytes() {
  return (2 * static_cast<size_t>(kTX + 2 * S) * (kTY + 2 * S) * (kTZ + 2 * S) + 6 * kTabLen) * sizeof(double);
}

template <int S, bool BOX>
void prepare_one() {
  W3D_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sponge_box<S, BOX>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes<S>())));
}

template <int S>
void launch_s(const SpongeBoxParams& p, bool box, unsigned blocks, hipStream_t stream) {
  if (box)
    hipLaunchKernelGGL((k_sponge_box<S, true>), dim3(blocks), dim3(kThreads), lds_bytes<S>(), stream, p);
  else
    hipLaunchKernelGGL((k_sponge_box<S, false>), dim3(blocks), dim3(kThreads), lds_bytes<S>(), stream, p);
}

}  // namespace

void sponge_box_prepare() {
  static const bool done = [] {
    prepare_one<2, false>();
    prepare_one<3, false>();
    prepare_one<4, false>();
    prepare_one<5, false>();
    prepare_one<2, true>();
    prepare_one<3, true>();
    prepare_one<4, true>();
    prepare_one<5, true>();
    return true;
  }();
  (void)done;
}

void launch_sponge_box(const Layout& l, const Coeffs& c, const SpongeView& tables, const double* prev, const double* cur,
                       double* out1, double* out2, const LBox& box, int steps, hipStream_t stream) {
  W3D_REQUIRE(steps >= 2 && steps <= kMaxSteps, "sponge_box: 2..5 steps");
  W3D_REQUIRE(prev != out1 && prev != out2 && cur != out1 && cur != out2 && out1 != out2 && prev != cur,
              "sponge_box needs four distinct buffers");
  // one rank: every node of the global interior lies inside the allocation, so the grown box clipped to the interior does
  W3D_REQUIRE(l.gx0 == 0 && l.gy0 == 0 && l.gz0 == 0 && l.nx == l.N + 1 && l.ny == l.N + 1 && l.nz == l.N + 1,
              "sponge_box: one rank that spans the whole domain");
  if (box.empty()) return;
  W3D_REQUIRE(box.x0 >= l.cx0 && box.x1 <= l.cx1 && box.y0 >= l.cy0 && box.y1 <= l.cy1 && box.z0 >= l.cz0 && box.z1 <= l.cz1,
              "sponge_box: the box must lie inside the updated region");
  W3D_REQUIRE(l.pitch % 2 == 0 && l.plane % 2 == 0, "sponge_box: rows must start on whole pairs");
  sponge_box_prepare();
  SpongeBoxParams p;
  p.prev = prev;
  p.cur = cur;
  p.out1 = out1;
  p.out2 = out2;
  p.sp = tables;
  p.plane = l.plane;
  p.pitch = l.pitch;
  p.base = l.off(0, 0, 0);
  p.N = l.N;
  p.gx0 = l.gx0;
  p.gy0 = l.gy0;
  p.gz0 = l.gz0;
  p.x0 = box.x0;
  p.x1 = box.x1;
  p.y0 = box.y0;
  p.y1 = box.y1;
  p.z0 = box.z0;
  p.z1 = box.z1;
  p.ntx = static_cast<int>(ceil_div(box.x1 - box.x0, kTX));
  p.nty = static_cast<int>(ceil_div(box.y1 - box.y0, kTY));
  p.ntz = static_cast<int>(ceil_div(box.z1 - box.z0, kTZ));
  p.lam = c.lam;
  p.ry = c.ry;
  p.rz = c.rz;
  const i64 blocks = static_cast<i64>(p.ntx) * p.nty * p.ntz;
  W3D_REQUIRE(blocks < (1ll << 31), "sponge_box: too many tiles");
  switch (steps) {
    case 2: launch_s<2>(p, c.box, static_cast<unsigned>(blocks), stream); break;
    case 3: launch_s<3>(p, c.box, static_cast<unsigned>(blocks), stream); break;
    case 4: launch_s<4>(p, c.box, static_cast<unsigned>(blocks), stream); break;
    default: launch_s<5>(p, c.box, static_cast<unsigned>(blocks), stream); break;
  }
  W3D_HIP_CHECK(hipGetLastError());
}

}  // namespace wave3d
