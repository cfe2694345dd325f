// Native unit tests of the fourth-order time integrator's host side (no GPU), Problem::time_order = 4: Problem's validation,
// Coeffs::lam12 / lam24 / lam6 and the CFL guard at courant() = 3/2; cpu_lap4, cpu_leapfrog44 and cpu_first_step_t4 against a
// direct triple loop over odd-reflected copies of u and of v (N = 6: every node within 2 of a wall; N = 24; cube and box;
// NaN in the stored ghost layer and the row padding of u, u^{n−1} and v); the eigenmode's first-step factor and recurrence;
// CpuSolver's refusals and the identity of time_order = 2.
//
// Built and run by CMake/ctest (CMakeLists.txt) and, with host AddressSanitizer + UBSan, by tests/test_time_order_native.py.
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

Problem make(i64 N, int K, bool box, int time_order = 4, double frac = 0.9) {
  Problem p;
  p.N = N;
  p.K = K;
  p.L = 1.0;
  if (box) {
    p.Ly = 1.3;
    p.Lz = 0.7;
  }
  p.order = 4;
  p.time_order = time_order;
  p.tau = 1.0;
  p.tau = frac * p.courant_limit() * p.tau_max();
  return p;
}

template <class F>
bool refused(F&& f, const char* prefix) {
  try {
    f();
  } catch (const std::exception& e) {
    return std::string(e.what()).find(prefix) == 8;  // after "wave3d: "
  }
  return false;
}

// a grid function on nodes −2..N+2 per axis, odd about every wall: value(−k) = −value(k), value(N+k) = −value(N−k)
struct Odd {
  i64 N;
  const Layout& l;
  const double* f;
  double operator()(i64 x, i64 y, i64 z) const {
    double sg = 1.0;
    auto fold = [&](i64 i) {
      if (i < 0) {
        sg = -sg;
        return -i;
      }
      if (i > N) {
        sg = -sg;
        return 2 * N - i;
      }
      return i;
    };
    const i64 fx = fold(x), fy = fold(y), fz = fold(z);
    return sg * f[static_cast<size_t>(l.off(fx, fy, fz))];
  }
};

double s4(const Odd& e, i64 x, i64 y, i64 z, const Coeffs& c, bool box) {
  const double u = e(x, y, z);
  auto ax = [&](double m2, double m1, double p1, double p2) {
    return std::fma(16.0, m1 + p1, std::fma(-30.0, u, -(m2 + p2)));
  };
  const double dx = ax(e(x - 2, y, z), e(x - 1, y, z), e(x + 1, y, z), e(x + 2, y, z));
  const double dy = ax(e(x, y - 2, z), e(x, y - 1, z), e(x, y + 1, z), e(x, y + 2, z));
  const double dz = ax(e(x, y, z - 2), e(x, y, z - 1), e(x, y, z + 1), e(x, y, z + 2));
  return box ? std::fma(c.rz, dz, std::fma(c.ry, dy, dx)) : (dx + dy) + dz;
}

// LCG values on the interior, exact zeros on the faces, NaN in the ghost layer and the padding
std::vector<double> field(const Layout& l, i64 N, unsigned long long& seed) {
  std::vector<double> f(static_cast<size_t>(l.total), std::nan(""));
  for (i64 x = 0; x <= N; ++x)
    for (i64 y = 0; y <= N; ++y)
      for (i64 z = 0; z <= N; ++z) {
        const bool in = x > 0 && x < N && y > 0 && y < N && z > 0 && z < N;
        f[static_cast<size_t>(l.off(x, y, z))] = in ? lcg(seed) : 0.0;
      }
  return f;
}

void coeffs_and_guard() {
  Problem p = make(16, 5, false);
  const Coeffs c = Coeffs::from(p);
  Problem p2 = p;
  p2.time_order = 2;
  const Coeffs c2 = Coeffs::from(p2);
  CHECK(c.time_order == 4 && c.order == 4 && c2.time_order == 2);
  CHECK(same(c.lam, c2.lam) && same(c.half_lam, c2.half_lam) && same(c.lam, ((p.tau * p.tau) * (1.0 / (p.h() * p.h()))) / 12.0));
  CHECK(same(c.lam12, c.lam / 12.0) && same(c.lam24, c.lam / 24.0) && same(c.lam6, c.lam / 6.0));
  CHECK(same(c2.lam12, 0.0) && same(c2.lam24, 0.0) && same(c2.lam6, 0.0));
  // the guard: courant_eff = courant · 2/3, the limit courant = 3/2; (4, 2) and (2, 2) keep their expressions
  CHECK(same(p.courant_eff(), p.courant() * (2.0 / 3.0)) && p.courant_limit() == 1.5);
  CHECK(same(p2.courant_eff(), p2.courant() * (2.0 / std::sqrt(3.0))) && same(p2.courant_limit(), std::sqrt(3.0) / 2.0));
  Problem q = p;
  q.tau = 0.999 * 1.5 * q.tau_max();
  CHECK(q.cfl_ok_eff());
  q.tau = 1.001 * 1.5 * q.tau_max();
  CHECK(!q.cfl_ok_eff());
  q.time_order = 2;
  q.tau = 0.999 * (std::sqrt(3.0) / 2.0) * q.tau_max();
  CHECK(q.cfl_ok_eff());
  q.tau = 1.001 * (std::sqrt(3.0) / 2.0) * q.tau_max();
  CHECK(!q.cfl_ok_eff());
  Problem o2;
  o2.N = 16;
  CHECK(same(o2.courant_eff(), o2.courant()) && o2.courant_limit() == 1.0 && o2.time_order == 2);
  // validation
  Problem bad = p;
  bad.time_order = 3;
  CHECK(refused([&] { bad.validate(); }, "time_order: the time order must be 2 or 4"));
  bad.time_order = 4;
  bad.order = 2;
  CHECK(refused([&] { bad.validate(); }, "time_order: 4 needs order = 4"));
  bad.order = 4;
  bad.sponge.width = 3;
  CHECK(refused([&] { bad.validate(); }, "order: no sponge"));
  p.validate();
  // the eigenmode's symbol: first-step factor 1 − z/2 + z²/24, recurrence 2 − z + z²/12, |.| ≤ 1 iff 0 ≤ z ≤ 12
  for (double z : {0.0, 1.0, 6.0, 9.72, 12.0}) CHECK(std::fabs(1.0 - z / 2.0 + z * z / 24.0) <= 1.0);
  CHECK(1.0 - 12.1 / 2.0 + 12.1 * 12.1 / 24.0 > 1.0);
}

void step_against_loop(i64 N, bool box, bool check) {
  const Problem p = make(N, 5, box);
  const Coeffs c = Coeffs::from(p);
  const Layout l = make_layout(p, Box{0, N + 1, 0, N + 1, 0, N + 1});
  const LBox full = compute_box(l);
  const std::vector<double> tab = sin_table_ext(p);
  unsigned long long seed = 99 + static_cast<unsigned long long>(N);
  const std::vector<double> cur = field(l, N, seed), old = field(l, N, seed);
  // v: zeros on the grid (the solver's zeroed buffer), NaN outside it
  std::vector<double> v(static_cast<size_t>(l.total), std::nan(""));
  for (i64 x = 0; x <= N; ++x)
    for (i64 y = 0; y <= N; ++y)
      for (i64 z = 0; z <= N; ++z) v[static_cast<size_t>(l.off(x, y, z))] = 0.0;
  const std::vector<double> v0 = v;
  cpu_lap4(l, c, cur.data(), v.data(), full);
  const Odd eu{N, l, cur.data()};
  i64 touched = 0;
  for (i64 q = 0; q < l.total; ++q)
    if (!same(v[static_cast<size_t>(q)], v0[static_cast<size_t>(q)])) ++touched;
  CHECK(touched <= (N - 1) * (N - 1) * (N - 1));
  for (i64 x = 1; x < N; ++x)
    for (i64 y = 1; y < N; ++y)
      for (i64 z = 1; z < N; ++z) CHECK(same(v[static_cast<size_t>(l.off(x, y, z))], c.lam * s4(eu, x, y, z, c, box)));
  for (i64 a = 0; a <= N; ++a)
    for (i64 b = 0; b <= N; ++b) {
      CHECK(same(v[static_cast<size_t>(l.off(0, a, b))], 0.0) && same(v[static_cast<size_t>(l.off(N, a, b))], 0.0));
      CHECK(same(v[static_cast<size_t>(l.off(a, 0, b))], 0.0) && same(v[static_cast<size_t>(l.off(a, N, b))], 0.0));
      CHECK(same(v[static_cast<size_t>(l.off(a, b, 0))], 0.0) && same(v[static_cast<size_t>(l.off(a, b, N))], 0.0));
    }
  std::vector<double> got = old;
  ErrAcc acc;
  cpu_leapfrog44(l, c, cur.data(), v.data(), got.data(), full, tab.data() + 1, 0.83, check ? &acc : nullptr);
  const Odd ev{N, l, v.data()};
  double emax = 0.0;
  for (i64 x = 1; x < N; ++x)
    for (i64 y = 1; y < N; ++y)
      for (i64 z = 1; z < N; ++z) {
        const size_t o = static_cast<size_t>(l.off(x, y, z));
        const double want = std::fma(c.lam12, s4(ev, x, y, z, c, box), (2.0 * cur[o] - old[o]) + v[o]);
        CHECK(same(got[o], want));
        const double err = std::fabs(want - ((tab[static_cast<size_t>(x + 1)] * tab[static_cast<size_t>(y + 1)]) * 0.83) *
                                                tab[static_cast<size_t>(z + 1)]);
        emax = err > emax ? err : emax;
      }
  if (check) CHECK(same(acc.max, emax));
  touched = 0;
  for (i64 q = 0; q < l.total; ++q)
    if (!same(got[static_cast<size_t>(q)], old[static_cast<size_t>(q)])) ++touched;
  CHECK(touched <= (N - 1) * (N - 1) * (N - 1));
  // a (4, 2) coefficient set is refused, and so is a time_order = 4 set in cpu_leapfrog
  Problem p2 = p;
  p2.time_order = 2;
  p2.tau = 0.5 * p2.tau;
  const Coeffs c2 = Coeffs::from(p2);
  CHECK(refused([&] { cpu_lap4(l, c2, cur.data(), v.data(), full); }, "time_order:"));
  CHECK(refused([&] { cpu_leapfrog(l, c, cur.data(), got.data(), full, tab.data() + 1, 0.0, nullptr); }, "time_order:"));
}

void first_step_against_loop(i64 N, bool box, bool with_psi) {
  const Problem p = make(N, 5, box);
  const Coeffs c = Coeffs::from(p);
  const Layout l = make_layout(p, Box{0, N + 1, 0, N + 1, 0, N + 1});
  const Layout src = initial_layout(p, l);
  std::vector<double> g(static_cast<size_t>((N + 1) * (N + 1) * (N + 1))), h = g;
  unsigned long long seed = 7;
  for (double& x : g) x = lcg(seed);
  for (double& x : h) x = lcg(seed);
  std::vector<double> phi(static_cast<size_t>(src.total)), psi = phi;
  initial_to_local(src, g.data(), phi.data());
  initial_to_local(src, h.data(), psi.data());
  std::vector<double> u0(static_cast<size_t>(l.total), 7.0), u1 = u0, v(static_cast<size_t>(l.total), 0.0);
  cpu_first_step_t4(l, src, c, p.tau, phi.data(), with_psi ? psi.data() : nullptr, v.data(), u0.data(), u1.data());
  const Odd ef{N, src, phi.data()}, es{N, src, psi.data()}, ev{N, l, v.data()};
  for (i64 x = 0; x <= N; ++x)
    for (i64 y = 0; y <= N; ++y)
      for (i64 z = 0; z <= N; ++z) {
        const size_t o = static_cast<size_t>(l.off(x, y, z));
        CHECK(same(u0[o], phi[static_cast<size_t>(src.off(x, y, z))]));
        if (!(x > 0 && x < N && y > 0 && y < N && z > 0 && z < N)) {
          CHECK(same(u1[o], 0.0) && same(v[o], 0.0));
          continue;
        }
        CHECK(same(v[o], c.lam * s4(ef, x, y, z, c, box)));
        double w = std::fma(c.lam24, s4(ev, x, y, z, c, box), std::fma(0.5, v[o], u0[o]));
        if (with_psi) w = std::fma(p.tau, std::fma(c.lam6, s4(es, x, y, z, c, box), es(x, y, z)), w);
        CHECK(same(u1[o], w));
      }
}

void solver_checks() {
  // the eigenmode: u^n = cos(n ω_h τ)·φ with cos(ω_h τ) = 1 − z/2 + z²/24, at 0.9 of the limit (courant 1.35)
  const i64 N = 12;
  Problem p = make(N, 40, false);
  CHECK(p.cfl_ok_eff() && p.courant() > 1.0);
  CpuSolver s(p, 1);
  const CpuResult r = s.run();
  CHECK(r.finite && r.steps.size() == 40u);
  const double th = M_PI / static_cast<double>(N);
  const double z = p.tau * p.tau * 3.0 * (30.0 - 32.0 * std::cos(th) + 2.0 * std::cos(2.0 * th)) / (12.0 * p.h() * p.h());
  const double om = std::acos(1.0 - z / 2.0 + z * z / 24.0);
  for (size_t k = 0; k < r.steps.size(); ++k) {
    const int n = r.steps[k];
    const double want = std::fabs(std::cos(n * om) - std::cos(p.a_t() * (n * p.tau)));  // (max |φ| = 1: N even)
    CHECK(std::fabs(r.max_err[k] - want) <= 16.0 * n * n * 2.3e-16);
  }
  // time_order = 2 given explicitly: the (4, 2) solve's bits
  Problem a = make(N, 9, false, 2), b = a;
  CpuSolver sa(a, 1), sb(b, 1);
  const CpuResult ra = sa.run(), rb = sb.run();
  CHECK(ra.max_err == rb.max_err && sa.field(0) == sb.field(0));
  // refusals
  const i64 node[3] = {3, 4, 5};
  std::vector<double> w(static_cast<size_t>(p.K), 1.0), one(static_cast<size_t>((N + 1) * (N + 1) * (N + 1)), 1.0);
  CHECK(refused([&] { s.set_sources(node, 1, w.data()); }, "time_order: no point sources"));
  s.set_sources(node, 0, nullptr);  // (removing sources is no refusal)
  CHECK(refused([&] { s.set_speed(one.data(), false); }, "order: no speed field"));
  CHECK(refused([&] { s.set_state(one.data(), one.data(), 3); }, "order: not together with set_state"));
  CHECK(refused([&] { (void)s.energy(0); }, "order: the second-order discrete energy"));
  // receivers read the stored nodes after every step
  s.set_receivers(node, 1);
  (void)s.run();
  CHECK(s.traces().size() == 41u && same(s.traces()[40], s.field(0)[static_cast<size_t>(s.layout().off(3, 4, 5))]));
}

}  // namespace

int main() {
  try {
    coeffs_and_guard();
    for (i64 N : {6, 24})
      for (bool box : {false, true}) {
        step_against_loop(N, box, false);
        step_against_loop(N, box, true);
        first_step_against_loop(N, box, false);
        first_step_against_loop(N, box, true);
      }
    solver_checks();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "unexpected exception: %s\n", e.what());
    return 1;
  }
  std::printf("test_time_order: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
