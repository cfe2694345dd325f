// Native unit tests of the user-supplied initial data path (no GPU): the global → local slicing into the layout with
// one ghost layer more (initial_layout / initial_to_local) on one rank and on rank layouts with deep ghosts,
// cpu_first_step_field against cpu_init_first and against a direct evaluation, cpu_energy against a brute-force sum
// over the global arrays and as a conserved quantity of CpuSolver::set_initial solves.
//
// Built and run by CMake/ctest (CMakeLists.txt) and, with host AddressSanitizer + UBSan, by tests/test_initial_native.py.
// Exit status 0 = all checks passed; every failure prints its location.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "wave3d/cpu.hpp"
#include "wave3d/decomp.hpp"
#include "wave3d/problem.hpp"
#include "wave3d/stencil.hpp"

using namespace wave3d;

namespace {

int g_fail = 0, g_checks = 0;

#define CHECK(cond)                                                          \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(cond)) {                                                           \
      ++g_fail;                                                              \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                        \
  } while (0)

Problem make(i64 N, int K, double Ly = 0.0, double Lz = 0.0) {
  Problem p;
  p.N = N;
  p.K = K;
  p.L = 1.0;
  p.Ly = Ly;
  p.Lz = Lz;
  p.tau = 0.5 * p.tau_max();
  p.validate();
  return p;
}

// a fixed pseudo-random global field (face values included: they must be ignored)
std::vector<double> field(i64 N, std::uint64_t seed) {
  std::vector<double> g(static_cast<size_t>((N + 1) * (N + 1) * (N + 1)));
  std::uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
  for (double& v : g) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    v = static_cast<double>(static_cast<std::int64_t>(s >> 11)) / 9007199254740992.0 - 0.5;
  }
  return g;
}

bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

// value of the global field with the Dirichlet faces and everything outside the grid 0
double at(const std::vector<double>& g, i64 N, i64 x, i64 y, i64 z) {
  if (x <= 0 || x >= N || y <= 0 || y >= N || z <= 0 || z >= N) return 0.0;
  return g[static_cast<size_t>((x * (N + 1) + y) * (N + 1) + z)];
}

void check_slicing_and_first_step(const Problem& p, const Dims& d, int rank, i64 xg, i64 yg, i64 zg, bool with_psi) {
  const i64 N = p.N;
  const Layout l = make_layout(p, rank_box(p, d, rank), 16, xg, yg, zg);
  const Layout src = initial_layout(p, l);
  CHECK(src.xg == xg + 1 && src.yg == yg + 1 && src.zg == zg + 1 && src.nx == l.nx && src.gz0 == l.gz0);
  CHECK((src.zg + src.zs - l.zg - l.zs) % 2 == 0);  // a 16-byte pair of the one layout is a pair of the other
  const std::vector<double> phi = field(N, 1), psi = field(N, 2);
  std::vector<double> f(static_cast<size_t>(src.total), -1.0), q(static_cast<size_t>(src.total), -1.0);
  initial_to_local(src, phi.data(), f.data());
  initial_to_local(src, psi.data(), q.data());
  i64 bad = 0, nonzero = 0;
  for (i64 x = -src.xg; x < src.nx + src.xg; ++x)
    for (i64 y = -src.yg; y < src.ny + src.yg; ++y)
      for (i64 z = -src.zg; z < src.nz + src.zg; ++z)
        bad += f[static_cast<size_t>(src.off(x, y, z))] != at(phi, N, src.gx0 + x, src.gy0 + y, src.gz0 + z);
  for (double v : f) nonzero += v != 0.0;
  CHECK(bad == 0);
  i64 want_nonzero = 0;
  for (i64 x = -src.xg; x < src.nx + src.xg; ++x)
    for (i64 y = -src.yg; y < src.ny + src.yg; ++y)
      for (i64 z = -src.zg; z < src.nz + src.zg; ++z)
        want_nonzero += at(phi, N, src.gx0 + x, src.gy0 + y, src.gz0 + z) != 0.0;
  CHECK(nonzero == want_nonzero);  // (padding and out-of-grid ghosts: zeros)

  const Coeffs c = Coeffs::from(p);
  std::vector<double> u0(static_cast<size_t>(l.total), 7.0), u1(static_cast<size_t>(l.total), 7.0);
  cpu_first_step_field(l, src, c, p.tau, f.data(), with_psi ? q.data() : nullptr, u0.data(), u1.data());
  bad = 0;
  for (i64 x = -l.xg; x < l.nx + l.xg; ++x)
    for (i64 y = -l.yg; y < l.ny + l.yg; ++y)
      for (i64 z = -l.zg; z < l.nz + l.zg; ++z) {
        const i64 gx = l.gx0 + x, gy = l.gy0 + y, gz = l.gz0 + z;
        const double v = at(phi, N, gx, gy, gz);
        double w = 0.0;
        if (gx > 0 && gx < N && gy > 0 && gy < N && gz > 0 && gz < N) {
          const double xm = at(phi, N, gx - 1, gy, gz), xp = at(phi, N, gx + 1, gy, gz), ym = at(phi, N, gx, gy - 1, gz),
                       yp = at(phi, N, gx, gy + 1, gz), zm = at(phi, N, gx, gy, gz - 1), zp = at(phi, N, gx, gy, gz + 1);
          const double lap = c.box ? d2sum_box(v, xm, xp, ym, yp, zm, zp, c.ry, c.rz) : d2sum(v, xm, xp, ym, yp, zm, zp);
          w = first_step(v, lap, c.half_lam);
          if (with_psi) w = first_step_psi(w, at(psi, N, gx, gy, gz), p.tau);
        }
        bad += u0[static_cast<size_t>(l.off(x, y, z))] != v || u1[static_cast<size_t>(l.off(x, y, z))] != w;
      }
  CHECK(bad == 0);
  for (i64 x = 0; x < l.nx + 2 * l.xg; ++x)  // the zero slot of every plane
    CHECK(u0[static_cast<size_t>(x * l.plane + l.zero_off())] == 0.0 && u1[static_cast<size_t>(x * l.plane + l.zero_off())] == 0.0);
}

void test_slicing_and_first_step() {
  for (i64 N : {16, 33}) {
    check_slicing_and_first_step(make(N, 4), Dims{1, 1, 1}, 0, 1, 1, 1, true);
    check_slicing_and_first_step(make(N, 4, 1.3, 0.7), Dims{1, 1, 1}, 0, 1, 1, 1, false);
  }
  check_slicing_and_first_step(make(33, 4, 1.3, 0.7), Dims{2, 2, 2}, 3, 5, 5, 5, true);
  check_slicing_and_first_step(make(33, 4), Dims{4, 1, 1}, 1, 5, 1, 1, true);
  check_slicing_and_first_step(make(33, 4), Dims{1, 2, 3}, 4, 1, 3, 2, false);
}

void test_eigenmode_reproduces_init_first() {
  for (const Problem& p : {make(16, 4), make(33, 4, 1.3, 0.7)}) {
    const i64 N = p.N;
    const Layout l = make_layout(p, Box{0, N + 1, 0, N + 1, 0, N + 1});
    const Layout src = initial_layout(p, l);
    const Coeffs c = Coeffs::from(p);
    const std::vector<double> s = sin_table_ext(p);
    std::vector<double> g(static_cast<size_t>((N + 1) * (N + 1) * (N + 1)));
    for (i64 x = 0; x <= N; ++x)
      for (i64 y = 0; y <= N; ++y)
        for (i64 z = 0; z <= N; ++z) g[static_cast<size_t>((x * (N + 1) + y) * (N + 1) + z)] = phi(s.data() + 1, x, y, z);
    std::vector<double> f(static_cast<size_t>(src.total));
    initial_to_local(src, g.data(), f.data());
    std::vector<double> r0(static_cast<size_t>(l.total), 1.0), r1 = r0, u0 = r0, u1 = r0;
    cpu_init_first(l, c, s.data() + 1, r0.data(), r1.data());
    cpu_first_step_field(l, src, c, p.tau, f.data(), nullptr, u0.data(), u1.data());
    CHECK(same_bits(u0, r0));
    CHECK(same_bits(u1, r1));
  }
}

void test_energy() {
  for (const Problem& p : {make(16, 12), make(33, 20, 1.3, 0.7)}) {
    const i64 N = p.N, n1 = N + 1;
    const std::vector<double> ph = field(N, 3), ps = field(N, 4);
    CpuSolver s(p, 2, 2);
    s.set_initial(ph.data(), ps.data());
    s.run();
    const EnergySums e1 = s.energy_sums(1), ek = s.energy_sums(0);
    const double E1 = s.energy(1), EK = s.energy(0);
    CHECK(E1 > 0.0 && EK == energy_value(p, ek.kin, ek.pot) && ek.depth == 3 * n1);
    // conserved within the summation bound of the two evaluations
    const double half_v = 0.5 * p.hx() * p.hy() * p.hz();
    const double tol = static_cast<double>(ek.depth + 8) * 0x1p-53 * half_v * ek.abs;
    CHECK(std::fabs(EK - E1) <= tol);
    // brute force over dense copies of the two levels, every edge by its lower endpoint (long double accumulators)
    const Layout& l = s.layout();
    std::vector<double> a(static_cast<size_t>(n1 * n1 * n1)), b(a.size());
    for (i64 x = 0; x <= N; ++x)
      for (i64 y = 0; y <= N; ++y)
        for (i64 z = 0; z <= N; ++z) {
          a[static_cast<size_t>((x * n1 + y) * n1 + z)] = s.field(1)[static_cast<size_t>(l.off(x, y, z))];
          b[static_cast<size_t>((x * n1 + y) * n1 + z)] = s.field(0)[static_cast<size_t>(l.off(x, y, z))];
        }
    const Coeffs c = Coeffs::from(p);
    long double kin = 0.0L, pot = 0.0L;
    auto id = [&](i64 x, i64 y, i64 z) { return static_cast<size_t>((x * n1 + y) * n1 + z); };
    for (i64 x = 0; x <= N; ++x)
      for (i64 y = 0; y <= N; ++y)
        for (i64 z = 0; z <= N; ++z) {
          const long double av = a[id(x, y, z)], bv = b[id(x, y, z)];
          kin += ((bv - av) / p.tau) * ((bv - av) / p.tau);
          if (x < N) pot += (b[id(x + 1, y, z)] - bv) * (a[id(x + 1, y, z)] - av) * c.ihx2;
          if (y < N) pot += (b[id(x, y + 1, z)] - bv) * (a[id(x, y + 1, z)] - av) * c.ihy2;
          if (z < N) pot += (b[id(x, y, z + 1)] - bv) * (a[id(x, y, z + 1)] - av) * c.ihz2;
        }
    const double brute = static_cast<double>(static_cast<long double>(half_v) * (kin + pot));
    CHECK(std::fabs(EK - brute) <= tol);
    // set_state takes the initial data's place again
    s.set_state(a.data(), b.data(), 1);
    s.run();
    bool threw = false;
    try {
      (void)s.energy(1);
    } catch (const std::exception&) {
      threw = true;
    }
    CHECK(threw);
  }
}

}  // namespace

int main() {
  test_slicing_and_first_step();
  test_eigenmode_reproduces_init_first();
  test_energy();
  std::printf("test_initial: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
