// CPU solver kernels (sequential + OpenMP). See wave3d/cpu.hpp.
//
// Parallelisation is over x-planes. The error reduction keeps one partial per plane and combines the partials in plane
// order, so the result does not depend on the thread count (the reference's tables show identical δ for every thread
// and rank count, report.pdf p.7-11).
#include <omp.h>

#include <cmath>
#include <vector>

#include "wave3d/cpu.hpp"
#include "wave3d/stencil.hpp"

namespace wave3d {

int cpu_set_threads(int n) {
  if (n > 0) omp_set_num_threads(n);
  return omp_get_max_threads();
}
int cpu_max_threads() { return omp_get_max_threads(); }

void cpu_init_first(const Layout& l, const Coeffs& c, const double* s, double* u0, double* u1) {
  W3D_REQUIRE(c.order == 2, "order: the analytic start is the second-order one; order 4 starts through cpu_first_step_field");
  const i64 N = l.N;
#pragma omp parallel for schedule(static)
  for (i64 ix = -1; ix <= l.nx; ++ix) {
    const i64 gx = l.gx0 + ix;
    // zero the whole plane first: padding and out-of-domain ghosts stay 0
    double* p0 = u0 + (ix + 1) * l.plane;
    double* p1 = u1 + (ix + 1) * l.plane;
    for (i64 q = 0; q < l.plane; ++q) {
      p0[q] = 0.0;
      p1[q] = 0.0;
    }
    for (i64 iy = -1; iy <= l.ny; ++iy) {
      const i64 gy = l.gy0 + iy;
      for (i64 iz = -1; iz <= l.nz; ++iz) {
        const i64 gz = l.gz0 + iz;
        const i64 o = l.off(ix, iy, iz);
        const double v = phi(s, gx, gy, gz);
        u0[o] = v;
        const bool interior = gx > 0 && gx < N && gy > 0 && gy < N && gz > 0 && gz < N;
        if (interior) {
          const double xm = phi(s, gx - 1, gy, gz), xp = phi(s, gx + 1, gy, gz), ym = phi(s, gx, gy - 1, gz),
                       yp = phi(s, gx, gy + 1, gz), zm = phi(s, gx, gy, gz - 1), zp = phi(s, gx, gy, gz + 1);
          const double lap =
              c.box ? d2sum_box(v, xm, xp, ym, yp, zm, zp, c.ry, c.rz) : d2sum(v, xm, xp, ym, yp, zm, zp);
          u1[o] = first_step(v, lap, c.half_lam);
        } else {
          u1[o] = 0.0;
        }
      }
    }
  }
}

std::vector<double> eigenmode_local(const Problem& p, const Layout& l) {
  const std::vector<double> tab = sin_table_ext(p);
  const double* s = tab.data() + 1;
  std::vector<double> out(static_cast<size_t>(l.total), 0.0);
#pragma omp parallel for schedule(static)
  for (i64 x = -l.xg; x < l.nx + l.xg; ++x) {
    const i64 gx = l.gx0 + x;
    if (gx < 0 || gx > l.N) continue;
    for (i64 y = -l.yg; y < l.ny + l.yg; ++y) {
      const i64 gy = l.gy0 + y;
      if (gy < 0 || gy > l.N) continue;
      for (i64 z = -l.zg; z < l.nz + l.zg; ++z) {
        const i64 gz = l.gz0 + z;
        if (gz >= 0 && gz <= l.N) out[static_cast<size_t>(l.off(x, y, z))] = phi(s, gx, gy, gz);
      }
    }
  }
  return out;
}

void cpu_first_step_field(const Layout& l, const Layout& src, const Coeffs& c, double tau, const double* phi,
                          const double* psi, double* u0, double* u1, const double* lamf) {
  W3D_REQUIRE(src.xg == l.xg + 1 && src.yg == l.yg + 1 && src.zg == l.zg + 1 && src.nx == l.nx && src.ny == l.ny &&
                  src.nz == l.nz && src.gx0 == l.gx0 && src.gy0 == l.gy0 && src.gz0 == l.gz0,
              "first step: the source layout must be the solve layout's box with one ghost layer more");
  const i64 N = l.N, P = src.plane, R = src.pitch;
#pragma omp parallel for schedule(static)
  for (i64 ix = -l.xg; ix < l.nx + l.xg; ++ix) {
    const i64 gx = l.gx0 + ix;
    double* p0 = u0 + (ix + l.xg) * l.plane;
    double* p1 = u1 + (ix + l.xg) * l.plane;
    for (i64 q = 0; q < l.plane; ++q) {
      p0[q] = 0.0;
      p1[q] = 0.0;
    }
    if (gx < 0 || gx > N) continue;
    for (i64 iy = -l.yg; iy < l.ny + l.yg; ++iy) {
      const i64 gy = l.gy0 + iy;
      if (gy < 0 || gy > N) continue;
      for (i64 iz = -l.zg; iz < l.nz + l.zg; ++iz) {
        const i64 gz = l.gz0 + iz;
        if (gz < 0 || gz > N) continue;
        const i64 o = l.off(ix, iy, iz);
        const double* f = phi + src.off(ix, iy, iz);
        const double v = f[0];
        u0[o] = v;
        if (gx > 0 && gx < N && gy > 0 && gy < N && gz > 0 && gz < N) {
          double lap;
          if (c.order == 4) {  // (a neighbour at distance 2 outside the domain: the odd reflection −v, not a load)
            const double xmm = gx == 1 ? -v : f[-2 * P], xpp = gx == N - 1 ? -v : f[2 * P];
            const double ymm = gy == 1 ? -v : f[-2 * R], ypp = gy == N - 1 ? -v : f[2 * R];
            const double zmm = gz == 1 ? -v : f[-2], zpp = gz == N - 1 ? -v : f[2];
            lap = c.box ? d4sum_t<true>(v, xmm, f[-P], f[P], xpp, ymm, f[-R], f[R], ypp, zmm, f[-1], f[1], zpp, c.ry, c.rz)
                        : d4sum_t<false>(v, xmm, f[-P], f[P], xpp, ymm, f[-R], f[R], ypp, zmm, f[-1], f[1], zpp, c.ry, c.rz);
          } else {
            lap = c.box ? d2sum_box(v, f[-P], f[P], f[-R], f[R], f[-1], f[1], c.ry, c.rz)
                        : d2sum(v, f[-P], f[P], f[-R], f[R], f[-1], f[1]);
          }
          double w = first_step(v, lap, lamf ? 0.5 * lamf[o] : c.half_lam);
          if (psi) w = first_step_psi(w, psi[src.off(ix, iy, iz)], tau);
          u1[o] = w;
        }
      }
    }
  }
}

EnergySums cpu_energy(const Layout& l, const Coeffs& c, double tau, const double* a, const double* b, const double* c2) {
  EnergySums out;
  if (l.nx <= 0 || l.ny <= 0 || l.nz <= 0) return out;
  W3D_REQUIRE(l.xg >= 1 && l.yg >= 1 && l.zg >= 1, "energy: the layout needs a ghost layer");
  const i64 N = l.N, P = l.plane, R = l.pitch;
  const double inv_tau = 1.0 / tau;
  std::vector<EnergySums> part(static_cast<size_t>(l.nx));
#pragma omp parallel for schedule(static)
  for (i64 ix = 0; ix < l.nx; ++ix) {
    const bool ex = l.gx0 + ix + 1 <= N;
    EnergySums pl;
    for (i64 iy = 0; iy < l.ny; ++iy) {
      const bool ey = l.gy0 + iy + 1 <= N;
      const double* ra = a + l.off(ix, iy, 0);
      const double* rb = b + l.off(ix, iy, 0);
      const double* rc = c2 ? c2 + l.off(ix, iy, 0) : nullptr;  // (a speed field: the mass weight 1/c²)
      double kin = 0.0, pot = 0.0, ab = 0.0;
      for (i64 iz = 0; iz < l.nz; ++iz) {
        const bool ez = l.gz0 + iz + 1 <= N;
        const double av = ra[iz], bv = rb[iz];
        const double v = (bv - av) * inv_tau;
        const double tk = !rc ? v * v : (rc[iz] > 0.0 ? (v * v) / rc[iz] : 0.0);
        const double tx = ex ? ((rb[iz + P] - bv) * (ra[iz + P] - av)) * c.ihx2 : 0.0;
        const double ty = ey ? ((rb[iz + R] - bv) * (ra[iz + R] - av)) * c.ihy2 : 0.0;
        const double tz = ez ? ((rb[iz + 1] - bv) * (ra[iz + 1] - av)) * c.ihz2 : 0.0;
        kin += tk;
        pot += (tx + ty) + tz;
        ab += tk + ((std::fabs(tx) + std::fabs(ty)) + std::fabs(tz));
      }
      pl.kin += kin;
      pl.pot += pot;
      pl.abs += ab;
    }
    part[static_cast<size_t>(ix)] = pl;
  }
  for (const EnergySums& p : part) {
    out.kin += p.kin;
    out.pot += p.pot;
    out.abs += p.abs;
  }
  out.depth = l.nz + l.ny + l.nx;
  return out;
}

namespace {

template <bool CHECK, bool BOX, bool DAMP = false, bool VARC = false>
void leapfrog_impl(const Layout& l, const Coeffs& c, const double* cur, double* out, const LBox& b, const double* s,
                   double ct, ErrAcc* acc, const SpongeView* sp = nullptr, const double* lamf = nullptr) {
  const i64 nxp = b.x1 - b.x0;
  std::vector<ErrAcc> part(CHECK ? static_cast<size_t>(nxp) : 0);
  const i64 P = l.plane, R = l.pitch;
#pragma omp parallel for schedule(static)
  for (i64 ix = b.x0; ix < b.x1; ++ix) {
    double emax = 0.0, esum = 0.0;
    const double sx = s[l.gx0 + ix];
    const double gx = DAMP ? sp->gx[l.gx0 + ix] : 0.0, rx = DAMP ? sp->rx[l.gx0 + ix] : 1.0;
    for (i64 iy = b.y0; iy < b.y1; ++iy) {
      const double sxy = analytic_row(sx, s[l.gy0 + iy], ct);
      const double gxy = DAMP ? std::fmax(gx, sp->gy[l.gy0 + iy]) : 0.0, rxy = DAMP ? std::fmin(rx, sp->ry[l.gy0 + iy]) : 1.0;
      const i64 row = l.off(ix, iy, 0);
      const double* cr = cur + row;
      double* orow = out + row;
      const double* lrow = VARC ? lamf + row : nullptr;
      for (i64 iz = b.z0; iz < b.z1; ++iz) {
        const double u = cr[iz];
        const double lap = d2sum_t<BOX>(u, cr[iz - P], cr[iz + P], cr[iz - R], cr[iz + R], cr[iz - 1], cr[iz + 1],
                                        c.ry, c.rz);
        double v = leapfrog(u, orow[iz], lap, VARC ? lrow[iz] : c.lam);
        if (DAMP) v = leapfrog_damped(v, orow[iz], std::fmax(gxy, sp->gz[l.gz0 + iz]), std::fmin(rxy, sp->rz[l.gz0 + iz]));
        orow[iz] = v;
        if (CHECK) {
          const double e = std::fabs(v - sxy * s[l.gz0 + iz]);
          emax = e > emax ? e : emax;
          esum = err_sq_acc(e, esum);
        }
      }
    }
    if (CHECK) part[static_cast<size_t>(ix - b.x0)] = ErrAcc{emax, esum};
  }
  if (CHECK) {
    for (const auto& p : part) {
      acc->max = p.max > acc->max ? p.max : acc->max;
      acc->sum += p.sum;
    }
  }
}

// Order 4 (stencil.hpp d4sum_t): the same loops with the 13-point operator. The layout spans the whole domain (one
// ghost layer), so a neighbour at distance 2 is a stored node unless the centre is node 1 or N − 1 of that axis; there
// it is the odd reflection −u and nothing is read.
template <bool CHECK, bool BOX>
void leapfrog4_impl(const Layout& l, const Coeffs& c, const double* cur, double* out, const LBox& b, const double* s,
                    double ct, ErrAcc* acc) {
  const i64 nxp = b.x1 - b.x0;
  std::vector<ErrAcc> part(CHECK ? static_cast<size_t>(nxp) : 0);
  const i64 P = l.plane, R = l.pitch, N = l.N;
#pragma omp parallel for schedule(static)
  for (i64 ix = b.x0; ix < b.x1; ++ix) {
    double emax = 0.0, esum = 0.0;
    const double sx = s[l.gx0 + ix];
    const bool xlo = l.gx0 + ix == 1, xhi = l.gx0 + ix == N - 1;
    for (i64 iy = b.y0; iy < b.y1; ++iy) {
      const double sxy = analytic_row(sx, s[l.gy0 + iy], ct);
      const bool ylo = l.gy0 + iy == 1, yhi = l.gy0 + iy == N - 1;
      const i64 row = l.off(ix, iy, 0);
      const double* cr = cur + row;
      double* orow = out + row;
      for (i64 iz = b.z0; iz < b.z1; ++iz) {
        const double u = cr[iz];
        const bool zlo = l.gz0 + iz == 1, zhi = l.gz0 + iz == N - 1;
        const double lap = d4sum_t<BOX>(u, xlo ? -u : cr[iz - 2 * P], cr[iz - P], cr[iz + P], xhi ? -u : cr[iz + 2 * P],
                                        ylo ? -u : cr[iz - 2 * R], cr[iz - R], cr[iz + R], yhi ? -u : cr[iz + 2 * R],
                                        zlo ? -u : cr[iz - 2], cr[iz - 1], cr[iz + 1], zhi ? -u : cr[iz + 2], c.ry, c.rz);
        const double v = leapfrog(u, orow[iz], lap, c.lam);
        orow[iz] = v;
        if (CHECK) {
          const double e = std::fabs(v - sxy * s[l.gz0 + iz]);
          emax = e > emax ? e : emax;
          esum = err_sq_acc(e, esum);
        }
      }
    }
    if (CHECK) part[static_cast<size_t>(ix - b.x0)] = ErrAcc{emax, esum};
  }
  if (CHECK) {
    for (const auto& p : part) {
      acc->max = p.max > acc->max ? p.max : acc->max;
      acc->sum += p.sum;
    }
  }
}

}  // namespace

namespace {
// (a speed field: the same loops with the coefficient read per node)
template <bool CHECK, bool BOX>
void leapfrog_varc(const Layout& l, const Coeffs& c, const double* cur, double* out, const LBox& b, const double* s, double ct,
                   ErrAcc* acc, const SpongeView* sp, const double* lamf) {
  if (sp)
    leapfrog_impl<CHECK, BOX, true, true>(l, c, cur, out, b, s, ct, acc, sp, lamf);
  else
    leapfrog_impl<CHECK, BOX, false, true>(l, c, cur, out, b, s, ct, acc, nullptr, lamf);
}
}  // namespace

void cpu_leapfrog(const Layout& l, const Coeffs& c, const double* cur, double* old_out, const LBox& box,
                  const double* s, double ct, ErrAcc* acc, const SpongeView* sponge, const double* lamf) {
  if (box.empty()) return;
  if (c.order == 4) {
    W3D_REQUIRE(!sponge && !lamf, "order: no sponge and no speed field with order = 4");
    W3D_REQUIRE(c.time_order == 2, "time_order: a time_order = 4 step is cpu_lap4 + cpu_leapfrog44");
    W3D_REQUIRE(l.nx == l.N + 1 && l.ny == l.N + 1 && l.nz == l.N + 1, "order: order = 4 needs a layout that spans the domain");
    if (c.box) {
      if (acc)
        leapfrog4_impl<true, true>(l, c, cur, old_out, box, s, ct, acc);
      else
        leapfrog4_impl<false, true>(l, c, cur, old_out, box, s, ct, nullptr);
    } else if (acc) {
      leapfrog4_impl<true, false>(l, c, cur, old_out, box, s, ct, acc);
    } else {
      leapfrog4_impl<false, false>(l, c, cur, old_out, box, s, ct, nullptr);
    }
    return;
  }
  if (lamf) {
    if (c.box) {
      if (acc)
        leapfrog_varc<true, true>(l, c, cur, old_out, box, s, ct, acc, sponge, lamf);
      else
        leapfrog_varc<false, true>(l, c, cur, old_out, box, s, ct, nullptr, sponge, lamf);
    } else if (acc) {
      leapfrog_varc<true, false>(l, c, cur, old_out, box, s, ct, acc, sponge, lamf);
    } else {
      leapfrog_varc<false, false>(l, c, cur, old_out, box, s, ct, nullptr, sponge, lamf);
    }
  } else if (sponge) {  // (sponge layers: the same loop with the damped update)
    if (c.box) {
      if (acc)
        leapfrog_impl<true, true, true>(l, c, cur, old_out, box, s, ct, acc, sponge);
      else
        leapfrog_impl<false, true, true>(l, c, cur, old_out, box, s, ct, nullptr, sponge);
    } else if (acc) {
      leapfrog_impl<true, false, true>(l, c, cur, old_out, box, s, ct, acc, sponge);
    } else {
      leapfrog_impl<false, false, true>(l, c, cur, old_out, box, s, ct, nullptr, sponge);
    }
  } else if (c.box) {  // (a rectangular box: stencil.hpp::d2sum_box)
    if (acc)
      leapfrog_impl<true, true>(l, c, cur, old_out, box, s, ct, acc);
    else
      leapfrog_impl<false, true>(l, c, cur, old_out, box, s, ct, nullptr);
  } else if (acc) {
    leapfrog_impl<true, false>(l, c, cur, old_out, box, s, ct, acc);
  } else {
    leapfrog_impl<false, false>(l, c, cur, old_out, box, s, ct, nullptr);
  }
}

namespace {

// Time order 4. s4_row: d4sum_t at node iz of the row f (any field in a layout with plane P and pitch R), a distance-2
// neighbour outside the domain replaced by −centre.
template <bool BOX>
inline double s4_row(const double* f, i64 iz, i64 P, i64 R, bool xlo, bool xhi, bool ylo, bool yhi, bool zlo, bool zhi,
                     const Coeffs& c) {
  const double u = f[iz];
  return d4sum_t<BOX>(u, xlo ? -u : f[iz - 2 * P], f[iz - P], f[iz + P], xhi ? -u : f[iz + 2 * P],
                      ylo ? -u : f[iz - 2 * R], f[iz - R], f[iz + R], yhi ? -u : f[iz + 2 * R],
                      zlo ? -u : f[iz - 2], f[iz - 1], f[iz + 1], zhi ? -u : f[iz + 2], c.ry, c.rz);
}

template <bool BOX>
void lap4_impl(const Layout& l, const Coeffs& c, const double* u, double* v, const LBox& b) {
  const i64 P = l.plane, R = l.pitch, N = l.N;
#pragma omp parallel for schedule(static)
  for (i64 ix = b.x0; ix < b.x1; ++ix) {
    const bool xlo = l.gx0 + ix == 1, xhi = l.gx0 + ix == N - 1;
    for (i64 iy = b.y0; iy < b.y1; ++iy) {
      const bool ylo = l.gy0 + iy == 1, yhi = l.gy0 + iy == N - 1;
      const i64 row = l.off(ix, iy, 0);
      for (i64 iz = b.z0; iz < b.z1; ++iz)
        v[row + iz] = lap_t4(s4_row<BOX>(u + row, iz, P, R, xlo, xhi, ylo, yhi, l.gz0 + iz == 1, l.gz0 + iz == N - 1, c),
                             c.lam);
    }
  }
}

template <bool CHECK, bool BOX>
void leapfrog44_impl(const Layout& l, const Coeffs& c, const double* cur, const double* v, double* out, const LBox& b,
                     const double* s, double ct, ErrAcc* acc) {
  const i64 nxp = b.x1 - b.x0;
  std::vector<ErrAcc> part(CHECK ? static_cast<size_t>(nxp) : 0);
  const i64 P = l.plane, R = l.pitch, N = l.N;
#pragma omp parallel for schedule(static)
  for (i64 ix = b.x0; ix < b.x1; ++ix) {
    double emax = 0.0, esum = 0.0;
    const double sx = s[l.gx0 + ix];
    const bool xlo = l.gx0 + ix == 1, xhi = l.gx0 + ix == N - 1;
    for (i64 iy = b.y0; iy < b.y1; ++iy) {
      const double sxy = analytic_row(sx, s[l.gy0 + iy], ct);
      const bool ylo = l.gy0 + iy == 1, yhi = l.gy0 + iy == N - 1;
      const i64 row = l.off(ix, iy, 0);
      const double* cr = cur + row;
      const double* vr = v + row;
      double* orow = out + row;
      for (i64 iz = b.z0; iz < b.z1; ++iz) {
        const double sv = s4_row<BOX>(vr, iz, P, R, xlo, xhi, ylo, yhi, l.gz0 + iz == 1, l.gz0 + iz == N - 1, c);
        const double w = leapfrog_t4(cr[iz], orow[iz], vr[iz], sv, c.lam12);
        orow[iz] = w;
        if (CHECK) {
          const double e = std::fabs(w - sxy * s[l.gz0 + iz]);
          emax = e > emax ? e : emax;
          esum = err_sq_acc(e, esum);
        }
      }
    }
    if (CHECK) part[static_cast<size_t>(ix - b.x0)] = ErrAcc{emax, esum};
  }
  if (CHECK) {
    for (const auto& p : part) {
      acc->max = p.max > acc->max ? p.max : acc->max;
      acc->sum += p.sum;
    }
  }
}

template <bool BOX>
void first_step_t4_impl(const Layout& l, const Layout& src, const Coeffs& c, double tau, const double* psi,
                        const double* v, const double* u0, double* u1, const LBox& b) {
  const i64 P = l.plane, R = l.pitch, N = l.N;
#pragma omp parallel for schedule(static)
  for (i64 ix = b.x0; ix < b.x1; ++ix) {
    const bool xlo = l.gx0 + ix == 1, xhi = l.gx0 + ix == N - 1;
    for (i64 iy = b.y0; iy < b.y1; ++iy) {
      const bool ylo = l.gy0 + iy == 1, yhi = l.gy0 + iy == N - 1;
      const i64 row = l.off(ix, iy, 0);
      const double* prow = psi ? psi + src.off(ix, iy, 0) : nullptr;
      for (i64 iz = b.z0; iz < b.z1; ++iz) {
        const bool zlo = l.gz0 + iz == 1, zhi = l.gz0 + iz == N - 1;
        const double sv = s4_row<BOX>(v + row, iz, P, R, xlo, xhi, ylo, yhi, zlo, zhi, c);
        double w = first_step_t4(u0[row + iz], v[row + iz], sv, c.lam24);
        if (prow)
          w = first_step_t4_psi(w, prow[iz], s4_row<BOX>(prow, iz, src.plane, src.pitch, xlo, xhi, ylo, yhi, zlo, zhi, c),
                                c.lam6, tau);
        u1[row + iz] = w;
      }
    }
  }
}

void require_t4(const Layout& l, const Coeffs& c, const LBox& box) {
  W3D_REQUIRE(c.time_order == 4 && c.order == 4, "time_order: the coefficients of a time_order = 4 problem are needed");
  W3D_REQUIRE(l.nx == l.N + 1 && l.ny == l.N + 1 && l.nz == l.N + 1 && l.gx0 == 0 && l.gy0 == 0 && l.gz0 == 0,
              "time_order: time_order = 4 needs a layout that spans the domain");
  W3D_REQUIRE(box.x0 >= 1 && box.x1 <= l.N && box.y0 >= 1 && box.y1 <= l.N && box.z0 >= 1 && box.z1 <= l.N,
              "time_order: the box must lie inside the global interior");
}

}  // namespace

void cpu_lap4(const Layout& l, const Coeffs& c, const double* u, double* v, const LBox& box) {
  if (box.empty()) return;
  require_t4(l, c, box);
  if (c.box)
    lap4_impl<true>(l, c, u, v, box);
  else
    lap4_impl<false>(l, c, u, v, box);
}

void cpu_leapfrog44(const Layout& l, const Coeffs& c, const double* cur, const double* v, double* old_out, const LBox& box,
                    const double* s, double ct, ErrAcc* acc) {
  if (box.empty()) return;
  require_t4(l, c, box);
  if (c.box) {
    if (acc)
      leapfrog44_impl<true, true>(l, c, cur, v, old_out, box, s, ct, acc);
    else
      leapfrog44_impl<false, true>(l, c, cur, v, old_out, box, s, ct, nullptr);
  } else if (acc) {
    leapfrog44_impl<true, false>(l, c, cur, v, old_out, box, s, ct, acc);
  } else {
    leapfrog44_impl<false, false>(l, c, cur, v, old_out, box, s, ct, nullptr);
  }
}

void cpu_first_step_t4(const Layout& l, const Layout& src, const Coeffs& c, double tau, const double* phi,
                       const double* psi, double* v, double* u0, double* u1) {
  const LBox box = compute_box(l);
  require_t4(l, c, box);
  // u⁰ = φ over the whole allocation and zeros in u¹ outside the interior, exactly as the (4, 2) start stores them (its
  // u¹ on the interior is replaced below)
  cpu_first_step_field(l, src, c, tau, phi, nullptr, u0, u1, nullptr);
  cpu_lap4(l, c, u0, v, box);
  if (c.box)
    first_step_t4_impl<true>(l, src, c, tau, psi, v, u0, u1, box);
  else
    first_step_t4_impl<false>(l, src, c, tau, psi, v, u0, u1, box);
}

namespace {

template <bool BOX>
void source_response_impl(const Problem& p, const Coeffs& c, const i64 node[3], const double* a, bool start, int s,
                          double* lv0, double* lv1) {
  constexpr int S = kSourceSide, R = kSourceRadius;
  auto cell = [](int i, int j, int k) { return ((i + R) * S + (j + R)) * S + (k + R); };
  auto interior = [&](int i, int j, int k) {
    return node[0] + i > 0 && node[0] + i < p.N && node[1] + j > 0 && node[1] + j < p.N && node[2] + k > 0 &&
           node[2] + k < p.N;
  };
  double* lv[2] = {lv0, lv1};
  int io = 0, ic = 1;  // level k is written over level k − 2
  for (int k = 1; k <= s; ++k) {
    const double* cu = lv[ic];
    double* out = lv[io];
    const int r = k - 1;
    for (int i = -r; i <= r; ++i)
      for (int j = -r; j <= r; ++j)
        for (int m = -r; m <= r; ++m) {
          if (std::abs(i) + std::abs(j) + std::abs(m) > r || !interior(i, j, m)) continue;
          const int q = cell(i, j, m);
          const double u = cu[q];
          const double lap = d2sum_t<BOX>(u, cu[q - S * S], cu[q + S * S], cu[q - S], cu[q + S], cu[q - 1], cu[q + 1], c.ry, c.rz);
          out[q] = leapfrog(u, out[q], lap, c.lam);
        }
    out[cell(0, 0, 0)] += start ? 0.5 * a[0] : a[k - 1];
    const int t = io;
    io = ic;
    ic = t;
  }
  // lv[ic] = r^{n+s}, lv[io] = r^{n+s−1}: s odd leaves the last level in lv0
  if (ic != 0)
    for (int q = 0; q < kSourceCells; ++q) {
      const double t = lv0[q];
      lv0[q] = lv1[q];
      lv1[q] = t;
    }
}

}  // namespace

void cpu_source_response(const Problem& p, const Coeffs& c, const i64 node[3], const double* a, bool first_is_start, int s,
                         double* out_last, double* out_prev) {
  W3D_REQUIRE(s >= 1 && s <= kSourceMaxSteps, "source_response: 1..5 steps");
  W3D_REQUIRE(c.order == 2 || s == 1, "order: with order = 4 the source response is that of a single step");
  W3D_REQUIRE(!first_is_start || s == 1, "source_response: the start is one step");
  W3D_REQUIRE(node[0] > 0 && node[0] < p.N && node[1] > 0 && node[1] < p.N && node[2] > 0 && node[2] < p.N,
              "source_response: the node is not strictly inside the grid");
  for (int q = 0; q < kSourceCells; ++q) out_last[q] = out_prev[q] = 0.0;
  if (c.box)
    source_response_impl<true>(p, c, node, a, first_is_start, s, out_last, out_prev);
  else
    source_response_impl<false>(p, c, node, a, first_is_start, s, out_last, out_prev);
}

void cpu_error(const Layout& l, const double* u, const LBox& b, const double* s, double ct, ErrAcc* acc) {
  if (b.empty()) return;
  const i64 nxp = b.x1 - b.x0;
  std::vector<ErrAcc> part(static_cast<size_t>(nxp));
#pragma omp parallel for schedule(static)
  for (i64 ix = b.x0; ix < b.x1; ++ix) {
    double emax = 0.0, esum = 0.0;
    const double sx = s[l.gx0 + ix];
    for (i64 iy = b.y0; iy < b.y1; ++iy) {
      const double sxy = analytic_row(sx, s[l.gy0 + iy], ct);
      for (i64 iz = b.z0; iz < b.z1; ++iz) {
        const double e = std::fabs(u[l.off(ix, iy, iz)] - sxy * s[l.gz0 + iz]);
        emax = e > emax ? e : emax;
        esum = err_sq_acc(e, esum);
      }
    }
    part[static_cast<size_t>(ix - b.x0)] = ErrAcc{emax, esum};
  }
  for (const auto& p : part) {
    acc->max = p.max > acc->max ? p.max : acc->max;
    acc->sum += p.sum;
  }
}

void cpu_pack_face(const Layout& l, const Face& f, const double* u, double* buf) {
  if (f.axis == 1) {
#pragma omp parallel for schedule(static)
    for (i64 ix = 0; ix < l.nx; ++ix)
      for (i64 iz = 0; iz < l.nz; ++iz) buf[ix * l.nz + iz] = u[l.off(ix, f.send_layer, iz)];
  } else if (f.axis == 2) {
#pragma omp parallel for schedule(static)
    for (i64 ix = 0; ix < l.nx; ++ix)
      for (i64 iy = 0; iy < l.ny; ++iy) buf[ix * l.ny + iy] = u[l.off(ix, iy, f.send_layer)];
  } else {
    const double* src = u + f.send_off;
    for (i64 q = 0; q < f.count; ++q) buf[q] = src[q];
  }
}

void cpu_unpack_face(const Layout& l, const Face& f, const double* buf, double* u) {
  if (f.axis == 1) {
#pragma omp parallel for schedule(static)
    for (i64 ix = 0; ix < l.nx; ++ix)
      for (i64 iz = 0; iz < l.nz; ++iz) u[l.off(ix, f.recv_layer, iz)] = buf[ix * l.nz + iz];
  } else if (f.axis == 2) {
#pragma omp parallel for schedule(static)
    for (i64 ix = 0; ix < l.nx; ++ix)
      for (i64 iy = 0; iy < l.ny; ++iy) u[l.off(ix, iy, f.recv_layer)] = buf[ix * l.ny + iy];
  } else {
    double* dst = u + f.recv_off;
    for (i64 q = 0; q < f.count; ++q) dst[q] = buf[q];
  }
}

}  // namespace wave3d
