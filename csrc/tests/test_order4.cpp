// Native unit tests of the fourth-order operator's host side (no GPU): cpu_leapfrog with Coeffs::order = 4 against a
// direct triple loop over a zero-extended, odd-reflected copy of the field (cube and box, with and without the error
// accumulator); the reflection at all six walls on a 6³ and a 9³ grid (the smallest in which nodes 1 and N − 1 are
// distinct, and adjacent to the nodes that read them) with NaN in the stored ghost layer; cpu_first_step_field's
// fourth-order form; Problem::order's validation and the order-aware CFL guard; CpuSolver's refusals; plan_units' single
// steps for K = 1..12.
//
// Built and run by CMake/ctest (CMakeLists.txt) and, with host AddressSanitizer + UBSan, by tests/test_order4_native.py.
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
  return static_cast<double>(s >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

Problem make(i64 N, int K, bool box, int order = 4) {
  Problem p;
  p.N = N;
  p.K = K;
  p.L = 1.0;
  if (box) {
    p.Ly = 1.3;
    p.Lz = 0.7;
  }
  p.order = order;
  p.tau = 1.0;
  p.tau = 0.4 * p.tau_max();
  return p;
}

template <class F>
bool refused(F&& f, const char* prefix) {
  try {
    f();
  } catch (const std::exception& e) {
    return std::string(e.what()).find(prefix) != std::string::npos;
  }
  return false;
}

// the field on nodes −2..N+2 per axis (index + 2): stored values on 0..N, the odd reflection u_{−k} = −u_k, u_{N+k} = −u_{N−k}
struct Ext {
  i64 N, M;
  std::vector<double> v;
  explicit Ext(i64 n) : N(n), M(n + 5), v(static_cast<size_t>((n + 5) * (n + 5) * (n + 5)), 0.0) {}
  double& at(i64 x, i64 y, i64 z) { return v[static_cast<size_t>(((x + 2) * M + (y + 2)) * M + (z + 2))]; }
};
i64 fold(i64 i, i64 N, double& sign) {
  if (i < 0) {
    sign = -sign;
    return -i;
  }
  if (i > N) {
    sign = -sign;
    return 2 * N - i;
  }
  return i;
}

// one order-4 step over the whole interior of an LCG field, ghost layer NaN: cpu_leapfrog against the triple loop
void step_against_loop(i64 N, bool box, bool check) {
  const Problem p = make(N, 5, box);
  const Coeffs c = Coeffs::from(p);
  CHECK(c.order == 4 && same(c.lam, ((p.tau * p.tau) * (1.0 / (p.h() * p.h()))) / 12.0));
  const Layout l = make_layout(p, Box{0, N + 1, 0, N + 1, 0, N + 1});
  const std::vector<double> tab = sin_table_ext(p);
  std::vector<double> cur(static_cast<size_t>(l.total), std::nan("")), old = cur;
  unsigned long long seed = 42 + static_cast<unsigned long long>(N);
  for (i64 x = 0; x <= N; ++x)
    for (i64 y = 0; y <= N; ++y)
      for (i64 z = 0; z <= N; ++z) {
        const bool in = x > 0 && x < N && y > 0 && y < N && z > 0 && z < N;
        cur[static_cast<size_t>(l.off(x, y, z))] = in ? lcg(seed) : 0.0;
        old[static_cast<size_t>(l.off(x, y, z))] = in ? lcg(seed) : 0.0;
      }
  Ext e(N);
  for (i64 x = -2; x <= N + 2; ++x)
    for (i64 y = -2; y <= N + 2; ++y)
      for (i64 z = -2; z <= N + 2; ++z) {
        double sg = 1.0;
        const i64 fx = fold(x, N, sg), fy = fold(y, N, sg), fz = fold(z, N, sg);
        e.at(x, y, z) = sg * cur[static_cast<size_t>(l.off(fx, fy, fz))];
      }
  std::vector<double> got = old;
  ErrAcc acc;
  cpu_leapfrog(l, c, cur.data(), got.data(), compute_box(l), tab.data() + 1, 0.83, check ? &acc : nullptr);
  double emax = 0.0;
  for (i64 x = 1; x < N; ++x)
    for (i64 y = 1; y < N; ++y)
      for (i64 z = 1; z < N; ++z) {
        auto ax = [&](double m2, double m1, double p1, double p2) {
          return std::fma(16.0, m1 + p1, std::fma(-30.0, e.at(x, y, z), -(m2 + p2)));
        };
        const double dx = ax(e.at(x - 2, y, z), e.at(x - 1, y, z), e.at(x + 1, y, z), e.at(x + 2, y, z));
        const double dy = ax(e.at(x, y - 2, z), e.at(x, y - 1, z), e.at(x, y + 1, z), e.at(x, y + 2, z));
        const double dz = ax(e.at(x, y, z - 2), e.at(x, y, z - 1), e.at(x, y, z + 1), e.at(x, y, z + 2));
        const double s = box ? std::fma(c.rz, dz, std::fma(c.ry, dy, dx)) : (dx + dy) + dz;
        const double u = e.at(x, y, z);
        const double want = std::fma(c.lam, s, 2.0 * u - old[static_cast<size_t>(l.off(x, y, z))]);
        CHECK(same(got[static_cast<size_t>(l.off(x, y, z))], want));
        const double err = std::fabs(want - ((tab[static_cast<size_t>(x + 1)] * tab[static_cast<size_t>(y + 1)]) * 0.83) *
                                                tab[static_cast<size_t>(z + 1)]);
        emax = err > emax ? err : emax;
      }
  if (check) CHECK(same(acc.max, emax));
  // nothing but the interior is written: the faces stay 0, the ghost layer and the padding NaN
  i64 other = 0;
  for (i64 q = 0; q < l.total; ++q) {
    const double a = got[static_cast<size_t>(q)], b = old[static_cast<size_t>(q)];
    if (!same(a, b)) ++other;
  }
  CHECK(other <= (N - 1) * (N - 1) * (N - 1));
  for (i64 y = 0; y <= N; ++y)
    for (i64 z = 0; z <= N; ++z) {
      CHECK(same(got[static_cast<size_t>(l.off(0, y, z))], 0.0) && same(got[static_cast<size_t>(l.off(N, y, z))], 0.0));
      CHECK(same(got[static_cast<size_t>(l.off(y, 0, z))], 0.0) && same(got[static_cast<size_t>(l.off(y, z, N))], 0.0));
    }
}

// the first step's fourth-order form against the same direct evaluation
void first_step_against_loop(i64 N, bool box, bool with_psi) {
  const Problem p = make(N, 5, box);
  const Coeffs c = Coeffs::from(p);
  const Layout l = make_layout(p, Box{0, N + 1, 0, N + 1, 0, N + 1});
  const Layout src = initial_layout(p, l);
  std::vector<double> g(static_cast<size_t>((N + 1) * (N + 1) * (N + 1))), h = g;
  unsigned long long seed = 7;
  for (double& v : g) v = lcg(seed);
  for (double& v : h) v = lcg(seed);
  std::vector<double> phi(static_cast<size_t>(src.total)), psi = phi;
  initial_to_local(src, g.data(), phi.data());
  initial_to_local(src, h.data(), psi.data());
  std::vector<double> u0(static_cast<size_t>(l.total), 7.0), u1 = u0;
  cpu_first_step_field(l, src, c, p.tau, phi.data(), with_psi ? psi.data() : nullptr, u0.data(), u1.data());
  auto f = [&](i64 x, i64 y, i64 z) {
    double sg = 1.0;
    const i64 fx = fold(x, N, sg), fy = fold(y, N, sg), fz = fold(z, N, sg);
    return sg * phi[static_cast<size_t>(src.off(fx, fy, fz))];
  };
  for (i64 x = 1; x < N; ++x)
    for (i64 y = 1; y < N; ++y)
      for (i64 z = 1; z < N; ++z) {
        const double u = f(x, y, z);
        auto ax = [&](double m2, double m1, double p1, double p2) {
          return std::fma(16.0, m1 + p1, std::fma(-30.0, u, -(m2 + p2)));
        };
        const double dx = ax(f(x - 2, y, z), f(x - 1, y, z), f(x + 1, y, z), f(x + 2, y, z));
        const double dy = ax(f(x, y - 2, z), f(x, y - 1, z), f(x, y + 1, z), f(x, y + 2, z));
        const double dz = ax(f(x, y, z - 2), f(x, y, z - 1), f(x, y, z + 1), f(x, y, z + 2));
        const double s = box ? std::fma(c.rz, dz, std::fma(c.ry, dy, dx)) : (dx + dy) + dz;
        double want = std::fma(c.half_lam, s, u);
        if (with_psi) want = std::fma(p.tau, psi[static_cast<size_t>(src.off(x, y, z))], want);
        CHECK(same(u1[static_cast<size_t>(l.off(x, y, z))], want));
        CHECK(same(u0[static_cast<size_t>(l.off(x, y, z))], u));
      }
  CHECK(same(u1[static_cast<size_t>(l.off(0, 3, 3))], 0.0) && same(u1[static_cast<size_t>(l.off(-1, 3, 3))], 0.0));
}

void problem_and_guard() {
  Problem p = make(16, 5, false);
  p.order = 3;
  CHECK(refused([&] { p.validate(); }, "order:"));
  p.order = 4;
  p.sponge.width = 3;
  CHECK(refused([&] { p.validate(); }, "order:"));
  p.sponge.width = 0;
  p.validate();
  for (bool box : {false, true}) {
    Problem q = make(16, 5, box);
    const double lim = q.tau_max() * (std::sqrt(3.0) / 2.0);
    q.tau = 0.999 * lim;
    CHECK(q.cfl_ok_eff() && q.cfl_ok());
    q.tau = 1.001 * lim;
    CHECK(!q.cfl_ok_eff() && q.cfl_ok());  // (courant() and tau_max() are the second-order ones, as before)
    Problem q2 = q;
    q2.order = 2;
    CHECK(q2.cfl_ok_eff() && same(q2.courant_eff(), q2.courant()));
    const Coeffs a = Coeffs::from(q), b = Coeffs::from(q2);
    CHECK(same(a.lam, b.lam / 12.0) && same(a.half_lam, b.half_lam / 12.0) && b.order == 2 && same(a.ry, b.ry));
  }
}

void solver_refusals_and_plan() {
  const i64 N = 12;
  const Problem p = make(N, 9, false);
  CpuSolver s(p, 1);
  const std::vector<double> ones(static_cast<size_t>((N + 1) * (N + 1) * (N + 1)), 1.0);
  CHECK(refused([&] { s.set_speed(ones.data()); }, "order:"));
  CHECK(refused([&] { s.set_state(ones.data(), ones.data(), 3); }, "order:"));
  const CpuResult r = s.run();
  CHECK(r.finite && r.steps.size() == 9);
  CHECK(refused([&] { (void)s.energy(0); }, "order:"));
  CHECK(refused([&] { (void)s.energy_sums(0); }, "order:"));
  // receivers and sources follow single steps and do not depend on the stencil
  const i64 node[3] = {5, 6, 7};
  std::vector<double> w(9, 1.0);
  s.set_sources(node, 1, w.data());
  s.set_receivers(node, 1);
  const CpuResult r2 = s.run();
  CHECK(r2.finite && s.traces().size() == 10 && s.traces()[9] != 0.0);
  // a forced solve beyond the new limit (classic Courant number 0.95) blows up and says so
  Problem bad = make(16, 400, false);
  bad.tau = 0.95 * bad.tau_max();
  CpuSolver sb(bad, 50);
  std::vector<double> phi(static_cast<size_t>(17 * 17 * 17));
  unsigned long long seed = 3;
  for (double& v : phi) v = lcg(seed);
  sb.set_initial(phi.data(), nullptr);
  Problem ok2 = bad;
  ok2.order = 2;
  CpuSolver s2(ok2, 50);
  s2.set_initial(phi.data(), nullptr);
  CHECK(!sb.run().finite || !(std::fabs(sb.field(0)[static_cast<size_t>(sb.layout().off(8, 8, 8))]) < 1e30));
  CHECK(std::fabs(s2.field(0)[static_cast<size_t>(s2.layout().off(8, 8, 8))]) < 1e3 || true);
  (void)s2.run();
  CHECK(std::fabs(s2.field(0)[static_cast<size_t>(s2.layout().off(8, 8, 8))]) < 1e3);

  for (int K = 1; K <= 12; ++K)
    for (int temporal : {1, 2, 5})
      for (bool tb : {false, true})
        for (int every : {0, 1, 3}) {
          Problem q = make(24, K, false);
          SolverOptions o;
          o.temporal = temporal;
          o.tb = tb;
          o.check_every = every;
          const RankSchedule sch = make_rank_schedule(q, o, 0, 1, 64e9);
          const std::vector<UnitPlan> u = plan_units(sch, 1, false);
          CHECK(static_cast<int>(u.size()) == K - 1);
          int n = 1;
          for (const UnitPlan& v : u) {
            CHECK(v.n == n && v.steps == 1 && !v.analytic && !v.drop_prev && !v.exchange && v.interior.count() == sch.full.count());
            ++n;
          }
          CHECK(refused([&] { (void)plan_units(sch, 1, true); }, "order:"));
          // traffic(): an order-4 step counts like any single step (two levels read, one written)
          const Traffic t = traffic(sch, u, true);
          const double node_b = 23.0 * 23.0 * 23.0 * sizeof(double);
          CHECK(t.field_bytes == node_b * (2.0 + 3.0 * static_cast<double>(K - 1)) && t.halo_bytes == 0.0);
        }
  Problem q2 = make(24, 9, false, 2);  // order 2: the plan is what it was
  const RankSchedule s2r = make_rank_schedule(q2, SolverOptions{}, 0, 1, 64e9);
  bool fused = false;
  for (const UnitPlan& v : plan_units(s2r, 1, true)) fused = fused || v.fused();
  CHECK(fused);
}

}  // namespace

int main() {
  try {
    for (i64 N : {6, 9, 13})
      for (bool box : {false, true})
        for (bool check : {false, true}) step_against_loop(N, box, check);
    for (i64 N : {6, 9})
      for (bool box : {false, true})
        for (bool psi : {false, true}) first_step_against_loop(N, box, psi);
    problem_and_guard();
    solver_refusals_and_plan();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "unexpected exception: %s\n", e.what());
    return 2;
  }
  std::printf("test_order4: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
