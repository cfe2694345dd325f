// User-supplied initial data: the first step from stored fields, and the discrete energy of two stored levels.
// See wave3d/kernels.hpp for the interface.
//
//   k_first_step_field : u⁰ = φ and u¹ = φ + τψ + (τ²/2)Δ_h φ from device-resident φ (and ψ), written over the whole solve
//                        layout (owned and ghost nodes, padding and zero slot), so the first pass needs no exchange.
//   k_energy           : per-workgroup partials of the kinetic and the potential sum of E^{n+1/2} over the owned nodes.
//   k_energy_reduce    : their fixed-order sum (one workgroup), so two calls on the same fields return the same bits.
//
// Both whole-field kernels move nodes in 16-byte pairs like the other whole-field kernels. φ / ψ live in a layout with
// one ghost layer more than the solve layout on every axis: its rows are shifted so that the same node sits at a column
// of the same parity in both layouts (Layout::zs is derived from cz0 + zg in both), so a pair of the one is a pair of
// the other.
#include <hip/hip_runtime.h>

#include "wave3d/device_util.hpp"
#include "wave3d/kernels.hpp"
#include "wave3d/stencil.hpp"

namespace wave3d {

namespace {

// ---------------------------------------------------------------------------------------------------------------
// first step from stored fields
// ---------------------------------------------------------------------------------------------------------------
struct FirstStepParams {
  double* u0;
  double* u1;
  const double* phi;  // source layout (one ghost layer more than the solve layout), faces and outside nodes 0
  const double* psi;  // ... or null: ψ = 0, its term is skipped
  i64 plane, N, nx, ny, nz, gx0, gy0, gz0, zs, xg, yg, zg;  // solve layout
  i64 s_plane, s_pitch, s_zs;                               // source layout (ghost depths xg + 1, yg + 1, zg + 1)
  int pairs_per_row, pairs_per_plane;
  double half_lam, ry, rz, tau;
  const double* lamf;  // VARC: lam·c² per node in the SOLVE layout (the pair at this thread's own store offset)
};

// One thread per 16-byte pair of the solve layout's plane blockIdx.y (k_init_first's grid). A pair with a valid node
// (inside the rank's ghost range and the global grid) loads the centre pair of φ; a pair with an interior node also
// the x∓1 / y∓1 pairs and the two z neighbours outside the pair (scalars: the pair left of a row's first pair would
// start before the row). Every address read belongs to a node within one layer of a valid node, which the source
// layout's extra ghost layer holds.
// Cube and box share one code path: the kernel never reads Coeffs::box, it always evaluates d2sum_box with Coeffs::ry /
// rz. For a cube Coeffs::from fills ry = rz = 1.0, and the box form fed ratios of 1 rounds exactly as d2sum does
// (stencil.hpp), so the cube's bits depend on those two fields being 1.0 — as in k_init_first.
// VARC: a speed field — the coefficient of a node is 0.5·lamf[p] (exact), the pair loaded at the thread's store offset.
// ORDER4: the fourth-order operator (stencil.hpp d4sum_t). The x∓2 / y∓2 pairs and the pairs left and right are loaded
// only where the node they serve is not next to that wall; there the neighbour is −centre. Every address read belongs to
// a node of the global grid within two layers of an interior node, which the source layout (ghost depth ≥ 2) holds.
template <bool VARC, bool ORDER4 = false>
__global__ __launch_bounds__(256) void k_first_step_field(const FirstStepParams p) {
  const int q = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
  if (q >= p.pairs_per_plane) return;
  const i64 ix = static_cast<i64>(blockIdx.y) - p.xg;
  const int r = q / p.pairs_per_row;
  const int c = q - r * p.pairs_per_row;
  const i64 iy = r - p.yg;
  const i64 iz0 = 2 * static_cast<i64>(c) - p.zg - p.zs;
  const i64 gx = p.gx0 + ix, gy = p.gy0 + iy;
  const bool xy_ok = gx >= 0 && gx <= p.N && gy >= 0 && gy <= p.N;
  const bool xy_in = gx > 0 && gx < p.N && gy > 0 && gy < p.N;
  bool ok[2], in[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const i64 iz = iz0 + e, gz = p.gz0 + iz;
    ok[e] = xy_ok && iz >= -p.zg && iz < p.nz + p.zg && gz >= 0 && gz <= p.N;
    in[e] = ok[e] && xy_in && gz > 0 && gz < p.N;
  }
  v2d w0, w1;
  w0.x = w0.y = 0.0;
  w1.x = w1.y = 0.0;
  if (ok[0] || ok[1]) {
    // the pair's first node in the source layout (an even column, as in the solve layout)
    const i64 so = (ix + p.xg + 1) * p.s_plane + (iy + p.yg + 1) * p.s_pitch + (iz0 + p.zg + 1 + p.s_zs);
    const double* f = p.phi + so;
    const v2d cv = ld2(f);
    w0.x = ok[0] ? cv.x : 0.0;
    w0.y = ok[1] ? cv.y : 0.0;
    if (in[0] || in[1]) {
      const v2d xm = ld2(f - p.s_plane), xp = ld2(f + p.s_plane), ym = ld2(f - p.s_pitch), yp = ld2(f + p.s_pitch);
      double a[2] = {0.0, 0.0};
      v2d hl;
      hl.x = hl.y = p.half_lam;
      if (VARC) {
        const v2d lf = ld2(p.lamf + static_cast<i64>(blockIdx.y) * p.plane + 2 * static_cast<i64>(q));
        hl.x = 0.5 * lf.x;
        hl.y = 0.5 * lf.y;
      }
      if constexpr (ORDER4) {
        const i64 N = p.N, gz0 = p.gz0 + iz0, gz1 = gz0 + 1;
        v2d ncv;
        ncv.x = -cv.x;
        ncv.y = -cv.y;
        const v2d x2m = gx == 1 ? ncv : ld2(f - 2 * p.s_plane), x2p = gx == N - 1 ? ncv : ld2(f + 2 * p.s_plane);
        const v2d y2m = gy == 1 ? ncv : ld2(f - 2 * p.s_pitch), y2p = gy == N - 1 ? ncv : ld2(f + 2 * p.s_pitch);
        if (in[0]) {
          const double zm = f[-1], z2m = gz0 == 1 ? ncv.x : f[-2], z2p = gz0 == N - 1 ? ncv.x : f[2];
          a[0] = first_step(cv.x, d4sum_t<true>(cv.x, x2m.x, xm.x, xp.x, x2p.x, y2m.x, ym.x, yp.x, y2p.x, z2m, zm, cv.y, z2p,
                                                p.ry, p.rz), hl.x);
        }
        if (in[1]) {
          const double zp = f[2], z2m = gz1 == 1 ? ncv.y : f[-1], z2p = gz1 == N - 1 ? ncv.y : f[3];
          a[1] = first_step(cv.y, d4sum_t<true>(cv.y, x2m.y, xm.y, xp.y, x2p.y, y2m.y, ym.y, yp.y, y2p.y, z2m, cv.x, zp, z2p,
                                                p.ry, p.rz), hl.y);
        }
      } else {
      if (in[0]) {
        const double zm = f[-1];
        a[0] = first_step(cv.x, d2sum_box(cv.x, xm.x, xp.x, ym.x, yp.x, zm, cv.y, p.ry, p.rz), hl.x);
      }
      if (in[1]) {
        const double zp = f[2];
        a[1] = first_step(cv.y, d2sum_box(cv.y, xm.y, xp.y, ym.y, yp.y, cv.x, zp, p.ry, p.rz), hl.y);
      }
      }
      if (p.psi) {
        const v2d sv = ld2(p.psi + so);
        if (in[0]) a[0] = first_step_psi(a[0], sv.x, p.tau);
        if (in[1]) a[1] = first_step_psi(a[1], sv.y, p.tau);
      }
      w1.x = a[0];
      w1.y = a[1];
    }
  }
  const i64 o = static_cast<i64>(blockIdx.y) * p.plane + 2 * static_cast<i64>(q);
  st2<false>(p.u0 + o, w0);
  st2<false>(p.u1 + o, w1);
}

// ---------------------------------------------------------------------------------------------------------------
// discrete energy
// ---------------------------------------------------------------------------------------------------------------
constexpr int kEnergyThreads = 256;
constexpr int kEnergyXChunk = 8;  // planes one thread sums before the wave reduction

struct EnergyParams {
  const double* a;  // u^n (the field's first element: columns below are whole-row columns, whose parity makes the pairs)
  const double* b;  // u^{n+1}
  Partial* partials;
  i64 plane, pitch, zs, xg, yg, zg, N, nx, ny, nz, gx0, gy0, gz0;
  i64 kp0;     // first pair column / 2 holding an owned node
  int npairs;  // pairs per row holding owned nodes
  double inv_tau, ihx2, ihy2, ihz2;
};

// Per-node terms (the same expressions, in the same order, as cpu_energy): kinetic ((b − a)·(1/τ))², potential
// ((b_x+ − b)(a_x+ − a))·ihx2 + ((b_y+ − b)(a_y+ − a))·ihy2 + ((b_z+ − b)(a_z+ − a))·ihz2 — every grid edge by its lower
// endpoint; an edge leaving the global grid contributes an exact 0.
//
// Reduction tree, depth D = energy_depth(layout):
//   thread   : the two nodes of its pair are added (1), then up to kEnergyXChunk planes serially (kEnergyXChunk)
//   wave     : 6 butterfly levels
//   workgroup: its 4 waves serially (3)                                           → one partial per workgroup (B of them)
//   k_energy_reduce (one workgroup of 1024): ceil(B / 1024) partials per thread serially, 6 butterfly levels, 16 waves
//              serially (15)
//   D = 1 + kEnergyXChunk + 6 + 3 + ceil(B / 1024) + 6 + 15,  B = ceil(nx / kEnergyXChunk) · ceil(ny · npairs / 256)
__global__ __launch_bounds__(kEnergyThreads) void k_energy(const EnergyParams p) {
  __shared__ double red_k[kEnergyThreads / 64], red_p[kEnergyThreads / 64];
  const i64 q = static_cast<i64>(blockIdx.x) * kEnergyThreads + threadIdx.x;
  double kin = 0.0, pot = 0.0;
  if (q < p.ny * p.npairs) {
    const i64 y = q / p.npairs;
    const i64 col = 2 * (p.kp0 + q % p.npairs);  // column of the pair's first node in its row
    const i64 z0 = col - p.zg - p.zs;            // its local z (Layout::off: column = z + zg + zs)
    const i64 x0 = static_cast<i64>(blockIdx.y) * kEnergyXChunk;
    const i64 x1 = imin(x0 + kEnergyXChunk, p.nx);
    const bool own0 = z0 >= 0 && z0 < p.nz, own1 = z0 + 1 >= 0 && z0 + 1 < p.nz;
    const bool ey = p.gy0 + y + 1 <= p.N;
    const bool ez0 = p.gz0 + z0 + 1 <= p.N, ez1 = p.gz0 + z0 + 2 <= p.N;
    const i64 o = (y + p.yg) * p.pitch + col;
    v2d a = ld2(p.a + (x0 + p.xg) * p.plane + o), b = ld2(p.b + (x0 + p.xg) * p.plane + o);
    for (i64 x = x0; x < x1; ++x) {
      const double* pa = p.a + (x + p.xg) * p.plane + o;
      const double* pb = p.b + (x + p.xg) * p.plane + o;
      const v2d ax = ld2(pa + p.plane), bx = ld2(pb + p.plane);
      const v2d ay = ld2(pa + p.pitch), by = ld2(pb + p.pitch);
      const double az = pa[2], bz = pb[2];
      const bool ex = p.gx0 + x + 1 <= p.N;
      double k0 = 0.0, k1 = 0.0, p0 = 0.0, p1 = 0.0;
      if (own0) {
        const double v = (b.x - a.x) * p.inv_tau;
        k0 = v * v;
        const double tx = ex ? ((bx.x - b.x) * (ax.x - a.x)) * p.ihx2 : 0.0;
        const double ty = ey ? ((by.x - b.x) * (ay.x - a.x)) * p.ihy2 : 0.0;
        const double tz = ez0 ? ((b.y - b.x) * (a.y - a.x)) * p.ihz2 : 0.0;
        p0 = (tx + ty) + tz;
      }
      if (own1) {
        const double v = (b.y - a.y) * p.inv_tau;
        k1 = v * v;
        const double tx = ex ? ((bx.y - b.y) * (ax.y - a.y)) * p.ihx2 : 0.0;
        const double ty = ey ? ((by.y - b.y) * (ay.y - a.y)) * p.ihy2 : 0.0;
        const double tz = ez1 ? ((bz - b.y) * (az - a.y)) * p.ihz2 : 0.0;
        p1 = (tx + ty) + tz;
      }
      kin += k0 + k1;
      pot += p0 + p1;
      a = ax;
      b = bx;
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    kin += __shfl_xor(kin, s, 64);
    pot += __shfl_xor(pot, s, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red_k[w] = kin;
    red_p[w] = pot;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double k = red_k[0], s = red_p[0];
    for (int r = 1; r < kEnergyThreads / 64; ++r) {
      k += red_k[r];
      s += red_p[r];
    }
    p.partials[static_cast<i64>(blockIdx.y) * gridDim.x + blockIdx.x] = make_double2(k, s);
  }
}

// out[0] = (Σ partials.x, Σ partials.y) in a fixed order (k_reduce's shape, both components summed)
__global__ __launch_bounds__(1024) void k_energy_reduce(const Partial* __restrict__ in, int n, Partial* out) {
  __shared__ double sk[16], sp[16];
  double k = 0.0, s = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const Partial v = in[i];
    k += v.x;
    s += v.y;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    k += __shfl_xor(k, o, 64);
    s += __shfl_xor(s, o, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sk[w] = k;
    sp[w] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double kk = sk[0], ss = sp[0];
    for (int r = 1; r < 16; ++r) {
      kk += sk[r];
      ss += sp[r];
    }
    out[0] = make_double2(kk, ss);
  }
}

struct EnergyGrid {
  i64 kp0 = 0;
  int npairs = 0, bx = 0, by = 0;
};

EnergyGrid energy_grid(const Layout& l) {
  EnergyGrid g;
  if (l.nx <= 0 || l.ny <= 0 || l.nz <= 0) return g;
  const i64 c0 = l.zg + l.zs, c1 = l.nz - 1 + l.zg + l.zs;  // columns of the first / last owned node of a row
  g.kp0 = c0 / 2;
  g.npairs = static_cast<int>(c1 / 2 - g.kp0 + 1);
  g.bx = static_cast<int>(ceil_div(l.ny * g.npairs, kEnergyThreads));
  g.by = static_cast<int>(ceil_div(l.nx, kEnergyXChunk));
  return g;
}

}  // namespace

void launch_first_step_field(const Layout& l, const Layout& src, const Coeffs& c, double tau, const double* phi,
                             const double* psi, double* u0, double* u1, hipStream_t stream, const double* lamf) {
  W3D_REQUIRE(src.xg == l.xg + 1 && src.yg == l.yg + 1 && src.zg == l.zg + 1 && src.nx == l.nx && src.ny == l.ny &&
                  src.nz == l.nz && src.gx0 == l.gx0 && src.gy0 == l.gy0 && src.gz0 == l.gz0,
              "first step: the source layout must be the solve layout's box with one ghost layer more");
  W3D_REQUIRE((src.zg + src.zs - l.zg - l.zs) % 2 == 0 && src.pitch % 2 == 0 && l.pitch % 2 == 0,
              "first step: the two layouts' pairs do not line up");
  W3D_REQUIRE(l.plane / 2 < (1ll << 31), "plane too large for the first-step kernel");
  W3D_REQUIRE(l.nx + 2 * l.xg <= 65535, "too many planes for the first-step kernel grid");
  FirstStepParams p;
  p.u0 = u0;
  p.u1 = u1;
  p.phi = phi;
  p.psi = psi;
  p.plane = l.plane;
  p.N = l.N;
  p.nx = l.nx;
  p.ny = l.ny;
  p.nz = l.nz;
  p.gx0 = l.gx0;
  p.gy0 = l.gy0;
  p.gz0 = l.gz0;
  p.zs = l.zs;
  p.xg = l.xg;
  p.yg = l.yg;
  p.zg = l.zg;
  p.s_plane = src.plane;
  p.s_pitch = src.pitch;
  p.s_zs = src.zs;
  p.pairs_per_row = static_cast<int>(l.pitch / 2);
  p.pairs_per_plane = static_cast<int>(l.plane / 2);
  p.half_lam = c.half_lam;
  p.ry = c.ry;
  p.rz = c.rz;
  p.tau = tau;
  p.lamf = lamf;
  const dim3 grid(static_cast<unsigned>(ceil_div(p.pairs_per_plane, 256)), static_cast<unsigned>(l.nx + 2 * l.xg));
  if (c.order == 4) {
    W3D_REQUIRE(!lamf, "order: no speed field with order = 4");
    W3D_REQUIRE(l.nx == l.N + 1 && l.ny == l.N + 1 && l.nz == l.N + 1, "order: the fourth-order first step needs one rank's "
                                                                     "layout that spans the whole domain");
    hipLaunchKernelGGL((k_first_step_field<false, true>), grid, dim3(256), 0, stream, p);
  } else if (lamf)
    hipLaunchKernelGGL(k_first_step_field<true>, grid, dim3(256), 0, stream, p);
  else
    hipLaunchKernelGGL(k_first_step_field<false>, grid, dim3(256), 0, stream, p);
  W3D_HIP_CHECK(hipGetLastError());
}

int energy_partials(const Layout& l) {
  const EnergyGrid g = energy_grid(l);
  return g.bx * g.by;
}

int energy_depth(const Layout& l) {
  return 1 + kEnergyXChunk + 6 + 3 + static_cast<int>(ceil_div(energy_partials(l), 1024)) + 6 + 15;
}

void launch_energy(const Layout& l, const Coeffs& c, double tau, const double* a, const double* b, Partial* partials,
                   hipStream_t stream) {
  const EnergyGrid g = energy_grid(l);
  W3D_REQUIRE(g.bx > 0 && g.by > 0 && g.by <= 65535, "energy: empty box or too many planes for the kernel grid");
  W3D_REQUIRE(l.xg >= 1 && l.yg >= 1 && l.zg >= 1 && l.pitch % 2 == 0, "energy: the layout needs a ghost layer and an even pitch");
  EnergyParams p;
  p.a = a;
  p.b = b;
  p.partials = partials;
  p.plane = l.plane;
  p.pitch = l.pitch;
  p.zs = l.zs;
  p.xg = l.xg;
  p.yg = l.yg;
  p.zg = l.zg;
  p.N = l.N;
  p.nx = l.nx;
  p.ny = l.ny;
  p.nz = l.nz;
  p.gx0 = l.gx0;
  p.gy0 = l.gy0;
  p.gz0 = l.gz0;
  p.kp0 = g.kp0;
  p.npairs = g.npairs;
  p.inv_tau = 1.0 / tau;
  p.ihx2 = c.ihx2;
  p.ihy2 = c.ihy2;
  p.ihz2 = c.ihz2;
  hipLaunchKernelGGL(k_energy, dim3(static_cast<unsigned>(g.bx), static_cast<unsigned>(g.by)), dim3(kEnergyThreads), 0,
                     stream, p);
  W3D_HIP_CHECK(hipGetLastError());
}

void launch_energy_reduce(const Partial* partials, int n, Partial* out, hipStream_t stream) {
  hipLaunchKernelGGL(k_energy_reduce, dim3(1), dim3(1024), 0, stream, partials, n, out);
  W3D_HIP_CHECK(hipGetLastError());
}

}  // namespace wave3d
