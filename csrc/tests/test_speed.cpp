// Native unit tests of the variable wave speed's host side (no GPU): speed_to_local (lamf = lam·c², c² with one rounding
// each, exact zeros on and outside the global boundary and in the padding, on a one-rank layout and on a block rank's
// layout with ghost layers; the refusals and the range), cpu_leapfrog with the field against a direct evaluation of the
// scheme node by node, the c ≡ 1 identity, cpu_first_step_field's halved coefficient, cpu_energy's mass weight,
// plan_units' speed plans and traffic()'s lamf reads.
//
// Built and run by CMake/ctest (CMakeLists.txt) and, with host AddressSanitizer + UBSan, by tests/test_speed_native.py.
// Exit status 0 = all checks passed; every failure prints its location.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "wave3d/cpu.hpp"
#include "wave3d/decomp.hpp"
#include "wave3d/problem.hpp"
#include "wave3d/schedule.hpp"
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

bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

double lcg(unsigned long long& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<double>(s >> 11) / 9007199254740992.0;
}

Problem make(i64 N, int K, bool box) {
  Problem p;
  p.N = N;
  p.K = K;
  p.L = 1.0;
  if (box) {
    p.Ly = 1.3;
    p.Lz = 0.7;
  }
  p.tau = 1.0;
  p.tau = 0.4 * p.tau_max() / 2.0;
  return p;
}

std::vector<double> medium(i64 N, unsigned long long seed) {
  std::vector<double> c(static_cast<size_t>((N + 1) * (N + 1) * (N + 1)));
  for (double& v : c) v = 0.5 + 1.5 * lcg(seed);
  return c;
}

template <class F>
bool refused(F&& f, const char* prefix) {
  try {
    f();
  } catch (const std::exception& e) {
    return std::strstr(e.what(), prefix) != nullptr;
  }
  return false;
}

void test_builder(i64 N, bool box, const Dims& d, int rank) {
  const Problem p = make(N, 9, box);
  const Layout l = make_layout(p, rank_box(p, d, rank), 16, d.px > 1 ? 2 : 1, 1, 1);
  std::vector<double> c = medium(N, 11);
  const i64 n1 = N + 1;
  // face values are ignored, whatever they hold
  c[0] = std::nan("");
  c[static_cast<size_t>(n1 * n1 * n1 - 1)] = -3.0;
  c[static_cast<size_t>((5 * n1 + 0) * n1 + 7)] = 0.0;
  std::vector<double> lamf(static_cast<size_t>(l.total), -7.0), c2(static_cast<size_t>(l.total), -7.0);
  const SpeedRange r = speed_to_local(p, l, c.data(), lamf.data(), c2.data());
  const double lam = Coeffs::from(p).lam;
  std::vector<char> seen(static_cast<size_t>(l.total), 0);
  double lo = 1e300, hi = 0.0;
  for (i64 x = 1; x < N; ++x)
    for (i64 y = 1; y < N; ++y)
      for (i64 z = 1; z < N; ++z) {
        const double v = c[static_cast<size_t>((x * n1 + y) * n1 + z)];
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
      }
  CHECK(same(r.cmin, lo) && same(r.cmax, hi));
  int bad = 0;
  for (i64 x = -l.xg; x < l.nx + l.xg; ++x)
    for (i64 y = -l.yg; y < l.ny + l.yg; ++y)
      for (i64 z = -l.zg; z < l.nz + l.zg; ++z) {
        const i64 gx = l.gx0 + x, gy = l.gy0 + y, gz = l.gz0 + z;
        const i64 o = l.off(x, y, z);
        seen[static_cast<size_t>(o)] = 1;
        const bool in = gx > 0 && gx < N && gy > 0 && gy < N && gz > 0 && gz < N;
        const double v = in ? c[static_cast<size_t>((gx * n1 + gy) * n1 + gz)] : 0.0;
        const double v2 = v * v;
        if (!same(c2[static_cast<size_t>(o)], in ? v2 : 0.0)) ++bad;
        if (!same(lamf[static_cast<size_t>(o)], in ? lam * v2 : 0.0)) ++bad;
      }
  CHECK(bad == 0);
  // the padding and everything else: exact +0
  for (i64 o = 0; o < l.total; ++o)
    if (!seen[static_cast<size_t>(o)] && !(same(lamf[static_cast<size_t>(o)], 0.0) && same(c2[static_cast<size_t>(o)], 0.0))) ++bad;
  CHECK(bad == 0);
  // either output may be left out
  speed_to_local(p, l, c.data(), nullptr, c2.data());
  speed_to_local(p, l, c.data(), lamf.data(), nullptr);
  // refusals: every interior value finite and > 0
  for (double v : {0.0, -1.0, std::nan(""), HUGE_VAL}) {
    std::vector<double> e = c;
    e[static_cast<size_t>((3 * n1 + 4) * n1 + 5)] = v;
    CHECK(refused([&] { speed_to_local(p, l, e.data(), lamf.data(), nullptr); }, "speed:"));
  }
  CHECK(refused([&] { speed_to_local(p, l, nullptr, lamf.data(), nullptr); }, "speed:"));
  // the CFL guard: courant · max c
  SpeedRange q;
  q.cmin = 1.0;
  q.cmax = 1.0 / p.courant();
  speed_cfl(p, q, false);
  q.cmax = 1.01 / p.courant();
  CHECK(refused([&] { speed_cfl(p, q, false); }, "speed: CFL"));
  speed_cfl(p, q, true);
}

void test_leapfrog(i64 N, bool box) {
  const Problem p = make(N, 9, box);
  const Layout l = make_layout(p, Box{0, N + 1, 0, N + 1, 0, N + 1});
  const Coeffs co = Coeffs::from(p);
  const std::vector<double> c = medium(N, 5);
  std::vector<double> lamf(static_cast<size_t>(l.total)), c2(static_cast<size_t>(l.total));
  speed_to_local(p, l, c.data(), lamf.data(), c2.data());
  unsigned long long seed = 3;
  std::vector<double> cur(static_cast<size_t>(l.total), 0.0), old(cur);
  for (i64 x = 1; x < N; ++x)
    for (i64 y = 1; y < N; ++y)
      for (i64 z = 1; z < N; ++z) {
        cur[static_cast<size_t>(l.off(x, y, z))] = lcg(seed) - 0.5;
        old[static_cast<size_t>(l.off(x, y, z))] = lcg(seed) - 0.5;
      }
  const std::vector<double> s = sin_table_ext(p);
  const LBox full = compute_box(l);
  std::vector<double> out = old;
  ErrAcc acc;
  cpu_leapfrog(l, co, cur.data(), out.data(), full, s.data() + 1, 0.7, &acc, nullptr, lamf.data());
  const i64 P = l.plane, R = l.pitch;
  int bad = 0;
  for (i64 x = 1; x < N; ++x)
    for (i64 y = 1; y < N; ++y)
      for (i64 z = 1; z < N; ++z) {
        const i64 o = l.off(x, y, z);
        const double* u = cur.data() + o;
        const double lap = co.box ? d2sum_box(u[0], u[-P], u[P], u[-R], u[R], u[-1], u[1], co.ry, co.rz)
                                  : d2sum(u[0], u[-P], u[P], u[-R], u[R], u[-1], u[1]);
        if (!same(out[static_cast<size_t>(o)], leapfrog(u[0], old[static_cast<size_t>(o)], lap, lamf[static_cast<size_t>(o)]))) ++bad;
      }
  CHECK(bad == 0);
  // nothing but the interior is written
  for (i64 o = 0; o < l.total; ++o)
    if (cur[static_cast<size_t>(o)] == 0.0 && old[static_cast<size_t>(o)] == 0.0 && !same(out[static_cast<size_t>(o)], 0.0)) ++bad;
  CHECK(bad == 0);
  // the check and the no-check path store the same bits
  std::vector<double> out2 = old;
  cpu_leapfrog(l, co, cur.data(), out2.data(), full, s.data() + 1, 0.0, nullptr, nullptr, lamf.data());
  CHECK(std::memcmp(out.data(), out2.data(), out.size() * sizeof(double)) == 0);
  // c ≡ 1: lamf == lam on the interior, and the constant-speed step's bits
  std::vector<double> one(c.size(), 1.0), lam1(static_cast<size_t>(l.total)), c21(static_cast<size_t>(l.total));
  speed_to_local(p, l, one.data(), lam1.data(), c21.data());
  CHECK(same(lam1[static_cast<size_t>(l.off(3, 4, 5))], co.lam));
  std::vector<double> a = old, b = old;
  cpu_leapfrog(l, co, cur.data(), a.data(), full, s.data() + 1, 0.0, nullptr);
  cpu_leapfrog(l, co, cur.data(), b.data(), full, s.data() + 1, 0.0, nullptr, nullptr, lam1.data());
  CHECK(std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
  // the first step: 0.5·lamf[p]
  const Layout il = initial_layout(p, l);
  std::vector<double> phi(static_cast<size_t>(il.total), 0.0);
  for (i64 x = 1; x < N; ++x)
    for (i64 y = 1; y < N; ++y)
      for (i64 z = 1; z < N; ++z) phi[static_cast<size_t>(il.off(x, y, z))] = lcg(seed) - 0.5;
  std::vector<double> u0(static_cast<size_t>(l.total), 9.0), u1(u0);
  cpu_first_step_field(l, il, co, p.tau, phi.data(), nullptr, u0.data(), u1.data(), lamf.data());
  for (i64 x = 0; x <= N; ++x)
    for (i64 y = 0; y <= N; ++y)
      for (i64 z = 0; z <= N; ++z) {
        const bool in = x > 0 && x < N && y > 0 && y < N && z > 0 && z < N;
        const double* f = phi.data() + il.off(x, y, z);
        const i64 IP = il.plane, IR = il.pitch;
        double want = 0.0;
        if (in) {
          const double lap = co.box ? d2sum_box(f[0], f[-IP], f[IP], f[-IR], f[IR], f[-1], f[1], co.ry, co.rz)
                                    : d2sum(f[0], f[-IP], f[IP], f[-IR], f[IR], f[-1], f[1]);
          want = first_step(f[0], lap, 0.5 * lamf[static_cast<size_t>(l.off(x, y, z))]);
        }
        if (!same(u1[static_cast<size_t>(l.off(x, y, z))], want)) ++bad;
      }
  CHECK(bad == 0);
  // the energy's mass weight: against a plain long double sum
  const EnergySums e = cpu_energy(l, co, p.tau, u0.data(), u1.data(), c2.data());
  const EnergySums e0 = cpu_energy(l, co, p.tau, u0.data(), u1.data());
  long double kin = 0.0L;
  for (i64 x = 1; x < N; ++x)
    for (i64 y = 1; y < N; ++y)
      for (i64 z = 1; z < N; ++z) {
        const i64 o = l.off(x, y, z);
        const double v = (u1[static_cast<size_t>(o)] - u0[static_cast<size_t>(o)]) * (1.0 / p.tau);
        kin += static_cast<long double>(v * v) / c2[static_cast<size_t>(o)];
      }
  CHECK(std::fabs(static_cast<double>(kin - e.kin)) <= 1e-12 * static_cast<double>(kin));
  CHECK(same(e.pot, e0.pot) && std::isfinite(e.kin) && e.kin != e0.kin);
}

void test_solver_and_plan() {
  const i64 N = 16;
  Problem p = make(N, 12, false);
  const std::vector<double> c = medium(N, 9);
  CpuSolver a(p, 2, 2), b(p, 2, 2);
  std::vector<double> one(c.size(), 1.0);
  b.set_speed(one.data());
  a.run();
  b.run();
  CHECK(std::memcmp(a.field(0).data(), b.field(0).data(), a.field(0).size() * sizeof(double)) == 0);
  CHECK(std::memcmp(a.field(1).data(), b.field(1).data(), a.field(1).size() * sizeof(double)) == 0);
  b.set_speed(c.data());
  b.run();
  CHECK(std::memcmp(a.field(0).data(), b.field(0).data(), a.field(0).size() * sizeof(double)) != 0);
  CHECK(std::isfinite(b.energy(0)) && std::fabs(b.energy(0) - b.energy(1)) <= 1e-12 * b.energy(1));
  b.set_speed(nullptr);
  CHECK(!b.speed());
  b.run();
  CHECK(std::memcmp(a.field(0).data(), b.field(0).data(), a.field(0).size() * sizeof(double)) == 0);
  std::vector<double> big(c.size(), 10.0);
  CHECK(refused([&] { b.set_speed(big.data()); }, "speed: CFL"));
  b.set_speed(big.data(), true);
  // the unit plans: pairs where no check falls between, single steps otherwise; no drop_prev; one lamf read per unit
  SolverOptions o;
  for (int every : {1, 2, 3}) {
    o.check_every = every;
    const RankSchedule s = make_rank_schedule(p, o, 0, 1, 64e9);
    for (SpeedPlan sp : {SpeedPlan::kPairs, SpeedPlan::kSingles}) {
      const std::vector<UnitPlan> u = plan_units(s, 1, false, false, sp);
      int n = 1;
      for (const UnitPlan& q : u) {
        CHECK(q.n == n && !q.drop_prev && !q.analytic && q.steps <= (sp == SpeedPlan::kPairs ? 2 : 1));
        CHECK(q.steps == 1 || !s.is_check(q.n + 1));
        n += q.steps;
      }
      CHECK(n == p.K);
      const Traffic t0 = traffic(s, u, true), t1 = traffic(s, u, true, true);
      const double node = static_cast<double>((N - 1) * (N - 1) * (N - 1)) * sizeof(double);
      CHECK(t1.field_bytes - t0.field_bytes == node * static_cast<double>(u.size() + 1));
    }
    CHECK(refused([&] { plan_units(s, 1, true, false, SpeedPlan::kPairs); }, "speed:"));
  }
}

}  // namespace

int main() {
  try {
    test_builder(12, false, Dims{1, 1, 1}, 0);
    test_builder(13, true, Dims{1, 1, 1}, 0);
    test_builder(14, false, Dims{2, 2, 1}, 3);
    test_leapfrog(12, false);
    test_leapfrog(11, true);
    test_solver_and_plan();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("test_speed: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
