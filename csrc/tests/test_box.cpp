// Native unit tests of the rectangular-box problem (no GPU): Problem / Coeffs box values, the cube's values unchanged
// (against a table of the numbers the cube expressions gave before boxes existed), the solve schedule's independence of
// the edges, and the box form of the CPU leapfrog fed ratios of 1 against the cube form.
//
// Built and run by CMake/ctest (CMakeLists.txt) and, with host AddressSanitizer + UBSan, by tests/test_box_native.py.
// Exit status 0 = all checks passed; every failure prints its location.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

Problem make(i64 N, double tau, int K, double L, double Ly = 0.0, double Lz = 0.0) {
  Problem p;
  p.N = N;
  p.tau = tau;
  p.K = K;
  p.L = L;
  p.Ly = Ly;
  p.Lz = Lz;
  p.validate();
  return p;
}

// The cube's numbers as the expressions of problem.hpp gave them before the box: a_t = π·sqrt(3/L²),
// courant = τ·sqrt(3)/h, tau_max = h/sqrt(3), 1/h², τ²/h², (τ²/2)/h² (hex floats: every bit).
struct CubeRow {
  i64 N;
  double tau, L, a_t, courant, tau_max, ih2, lam, half_lam;
};
const CubeRow kCube[] = {
    {512, 0x1.0624dd2f1a9fcp-10, 0x1.0000000000000p+0, 0x1.5c3fddc92b2ddp+2, 0x1.c60bf64b487d9p-1,
     0x1.279a74590331dp-10, 0x1.0000000000000p+18, 0x1.0c6f7a0b5ed8dp-2, 0x1.0c6f7a0b5ed8dp-3},
    {128, 0x1.0624dd2f1a9fcp-10, 0x1.921fb54442d18p+1, 0x1.bb67ae8584cabp+0, 0x1.210e1c99f615cp-4,
     0x1.d05527b6e43d2p-7, 0x1.9f02f6222c720p+10, 0x1.b32bd1ce57881p-10, 0x1.b32bd1ce57881p-11},
    {24, 0x1.0624dd2f1a9fcp-10, 0x1.0000000000000p+1, 0x1.5c3fddc92b2ddp+1, 0x1.5488f8b8765e3p-6,
     0x1.8a2345cc04426p-5, 0x1.2000000000000p+7, 0x1.2dfd694ccab3fp-13, 0x1.2dfd694ccab3fp-14},
    {64, 0x1.0624dd2f1a9fcp-12, 0x1.8000000000000p-1, 0x1.d05527b6e43d1p+2, 0x1.2eb2a4323053bp-5,
     0x1.bb67ae8584cabp-8, 0x1.c71c71c71c71cp+12, 0x1.dd37f5698c2c1p-12, 0x1.dd37f5698c2c1p-13},
};

void test_cube_unchanged() {
  for (const CubeRow& r : kCube) {
    // a plain cube, and the same cube spelled with its three edges: both are cubes
    for (int spelled = 0; spelled < 2; ++spelled) {
      const Problem p = make(r.N, r.tau, 10, r.L, spelled ? r.L : 0.0, spelled ? r.L : 0.0);
      CHECK(!p.is_box());
      CHECK(p.a_t() == r.a_t);
      CHECK(p.courant() == r.courant);
      CHECK(p.tau_max() == r.tau_max);
      CHECK(p.hx() == p.h() && p.hy() == p.h() && p.hz() == p.h());
      const Coeffs c = Coeffs::from(p);
      CHECK(!c.box && c.ry == 1.0 && c.rz == 1.0);
      CHECK(c.ihx2 == r.ih2 && c.ihy2 == r.ih2 && c.ihz2 == r.ih2);
      CHECK(c.tau2 == r.tau * r.tau && c.half_tau2 == 0.5 * (r.tau * r.tau));
      CHECK(c.lam == r.lam && c.half_lam == r.half_lam);
      const Coeffs f = Coeffs::from(p, true);  // the forced box form of a cube: ratios of 1, everything else equal
      CHECK(f.box && f.ry == 1.0 && f.rz == 1.0 && f.lam == r.lam && f.half_lam == r.half_lam);
    }
  }
}

void test_box_values() {
  const double Lx = 1.0, Ly = 1.3, Lz = 0.7, tau = 1e-3;
  const i64 N = 32;
  const Problem p = make(N, tau, 11, Lx, Ly, Lz);
  CHECK(p.is_box());
  CHECK(p.Lx() == Lx && p.edge_y() == Ly && p.edge_z() == Lz);
  CHECK(p.hx() == Lx / 32.0 && p.hy() == Ly / 32.0 && p.hz() == Lz / 32.0);
  // the fixed operation orders
  CHECK(p.a_t() == M_PI * std::sqrt((1.0 / (Lx * Lx) + 1.0 / (Ly * Ly)) + 1.0 / (Lz * Lz)));
  const double hx = p.hx(), hy = p.hy(), hz = p.hz();
  const double q = (1.0 / (hx * hx) + 1.0 / (hy * hy)) + 1.0 / (hz * hz);
  CHECK(p.courant() == tau * std::sqrt(q));
  CHECK(p.tau_max() == 1.0 / std::sqrt(q));
  CHECK(p.cfl_ok());
  // tau_max ≈ 4.0e-3 at N = 130 (the largest N of the GPU tests), below the cube's h/√3 ≈ 4.4e-3: hz < hx
  const Problem p130 = make(130, tau, 11, Lx, Ly, Lz);
  CHECK(p130.tau_max() > 3.9e-3 && p130.tau_max() < 4.1e-3 && p130.tau_max() < make(130, tau, 11, Lx).tau_max());
  // mathematically: a_t² = π²·Σ 1/L_d², courant² = τ²·N²·Σ 1/L_d²
  const double sl = 1.0 / (Lx * Lx) + 1.0 / (Ly * Ly) + 1.0 / (Lz * Lz);
  CHECK(std::fabs(p.a_t() * p.a_t() - M_PI * M_PI * sl) < 1e-12 * M_PI * M_PI * sl);
  CHECK(std::fabs(p.courant() - tau * 32.0 * std::sqrt(sl)) < 1e-15);
  const Coeffs c = Coeffs::from(p);
  CHECK(c.box);
  CHECK(c.ihx2 == 1.0 / (hx * hx) && c.ihy2 == 1.0 / (hy * hy) && c.ihz2 == 1.0 / (hz * hz));
  CHECK(c.ry == (hx * hx) / (hy * hy) && c.rz == (hx * hx) / (hz * hz));
  CHECK(std::fabs(c.ry - 1.0 / 1.69) < 1e-15 && std::fabs(c.rz - 1.0 / 0.49) < 1e-14);
  CHECK(c.lam == (tau * tau) * c.ihx2 && c.half_lam == (0.5 * (tau * tau)) * c.ihx2);
  // a CFL case: τ between the box's and the unit cube's tau_max
  const Problem bad = make(N, 0.5 * (p.tau_max() + make(N, tau, 11, 1.0).tau_max()), 11, Lx, Ly, Lz);
  CHECK(!bad.cfl_ok());
  CHECK(make(N, bad.tau, 11, 1.0).cfl_ok());
  // the sine table does not know the edges beyond Lx: sin(π·i·h_x/L_x)
  const std::vector<double> sb = sin_table_ext(p), sc = sin_table_ext(make(N, tau, 11, Lx));
  CHECK(sb == sc);
  // d2sum_box: the fixed form, and with ratios of 1 the cube's bits
  const double v[7] = {0.3, -0.7, 0.11, 1.9, -2.3, 0.05, 0.77};
  const double c2 = 2.0 * v[0];
  CHECK(d2sum_box(v[0], v[1], v[2], v[3], v[4], v[5], v[6], c.ry, c.rz) ==
        std::fma(c.rz, v[6] - c2 + v[5], std::fma(c.ry, v[4] - c2 + v[3], v[2] - c2 + v[1])));
  CHECK(d2sum_box(v[0], v[1], v[2], v[3], v[4], v[5], v[6], 1.0, 1.0) == d2sum(v[0], v[1], v[2], v[3], v[4], v[5], v[6]));
}

// ---- the schedule does not depend on the edges
bool same_box(const LBox& a, const LBox& b) {
  return a.x0 == b.x0 && a.x1 == b.x1 && a.y0 == b.y0 && a.y1 == b.y1 && a.z0 == b.z0 && a.z1 == b.z1;
}
bool same_boxes(const std::vector<LBox>& a, const std::vector<LBox>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (!same_box(a[i], b[i])) return false;
  return true;
}
bool same_units(const std::vector<UnitPlan>& a, const std::vector<UnitPlan>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) {
    const UnitPlan &x = a[i], &y = b[i];
    if (x.n != y.n || x.steps != y.steps || x.analytic != y.analytic || x.exchange != y.exchange ||
        x.depth != y.depth || x.ghost_bits != y.ghost_bits || x.msgs.size() != y.msgs.size() ||
        !same_boxes(x.shells, y.shells) || !same_box(x.interior, y.interior))
      return false;
    for (size_t m = 0; m < x.msgs.size(); ++m) {
      const MsgPlan &p = x.msgs[m], &q = y.msgs[m];
      if (p.peer != q.peer || p.tag != q.tag || p.field != q.field || p.send_off != q.send_off ||
          p.recv_off != q.recv_off || p.count != q.count)
        return false;
    }
  }
  return true;
}

void test_schedule_independent_of_edges() {
  const int K = 21;
  for (int world : {1, 4, 8}) {
    for (const char* decomp : {"slab", "block"}) {
      for (int overlap = 0; overlap < 2; ++overlap) {
        SolverOptions o;
        o.decomp = decomp;
        o.overlap = overlap != 0;
        o.tb_min_planes = 8;
        for (i64 N : {64, 100}) {
          for (int r = 0; r < world; ++r) {
            const RankSchedule sc = make_rank_schedule(make(N, 1e-3, K, 1.0), o, r, world, 1e13);
            const RankSchedule sb = make_rank_schedule(make(N, 1e-3, K, 1.0, 1.3, 0.7), o, r, world, 1e13);
            CHECK(sb.prob.is_box() && !sc.prob.is_box());
            CHECK(sc.mode == sb.mode && sc.mode_name() == sb.mode_name() && sc.nbuf == sb.nbuf);
            CHECK(sc.opt.temporal == sb.opt.temporal && sc.block_tb == sb.block_tb);
            CHECK(sc.dims.px == sb.dims.px && sc.dims.py == sb.dims.py && sc.dims.pz == sb.dims.pz);
            CHECK(sc.lay.total == sb.lay.total && sc.lay.plane == sb.lay.plane && sc.lay.pitch == sb.lay.pitch);
            CHECK(same_box(sc.full, sb.full) && same_box(sc.interior, sb.interior) && same_box(sc.dint, sb.dint));
            CHECK(same_boxes(sc.shell, sb.shell) && same_boxes(sc.dshell, sb.dshell));
            CHECK(sc.analytic_ok() == sb.analytic_ok() && sc.send_total == sb.send_total && sc.deep_max == sb.deep_max);
            const bool analytic = (sc.mode == Mode::kFusedSingle || sc.mode == Mode::kDeepTb) && sc.analytic_ok();
            const int start = analytic ? 1 : sc.opt.init2 && K >= 2 ? 2 : 1;
            const std::vector<UnitPlan> uc = plan_units(sc, start, analytic), ub = plan_units(sb, start, analytic);
            CHECK(!uc.empty());
            CHECK(same_units(uc, ub));
          }
        }
      }
    }
  }
}

// ---- cpu_leapfrog / cpu_init_first: the box form with ratios of 1 is the cube form, bit for bit
void test_cpu_box_form_with_unit_ratios() {
  const Problem p = make(20, 1e-3, 5, 2.0);
  const Layout l = make_layout(p, rank_box(p, Dims{1, 1, 1}, 0));
  const Coeffs cube = Coeffs::from(p), forced = Coeffs::from(p, true);
  CHECK(!cube.box && forced.box);
  const std::vector<double> s = sin_table_ext(p);
  std::uint64_t st = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() {  // xorshift64*: values in (−1, 1)
    st ^= st >> 12;
    st ^= st << 25;
    st ^= st >> 27;
    return static_cast<double>((st * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 * 2.0 - 1.0;
  };
  std::vector<double> cur(static_cast<size_t>(l.total)), old(static_cast<size_t>(l.total));
  for (double& v : cur) v = rnd();
  for (double& v : old) v = rnd();
  std::vector<double> oa = old, ob = old;
  ErrAcc ea, eb;
  const LBox full = compute_box(l);
  cpu_leapfrog(l, cube, cur.data(), oa.data(), full, s.data() + 1, 0.83, &ea);
  cpu_leapfrog(l, forced, cur.data(), ob.data(), full, s.data() + 1, 0.83, &eb);
  CHECK(std::memcmp(oa.data(), ob.data(), oa.size() * sizeof(double)) == 0);
  CHECK(std::memcmp(oa.data(), old.data(), oa.size() * sizeof(double)) != 0);
  CHECK(ea.max == eb.max && ea.sum == eb.sum);
  std::vector<double> a0(cur.size()), a1(cur.size()), b0(cur.size()), b1(cur.size());
  cpu_init_first(l, cube, s.data() + 1, a0.data(), a1.data());
  cpu_init_first(l, forced, s.data() + 1, b0.data(), b1.data());
  CHECK(a0 == b0 && a1 == b1);
  // ... and real ratios change the result (the flag is not ignored)
  const Coeffs real = Coeffs::from(make(20, 1e-3, 5, 2.0, 2.6, 1.4));
  std::vector<double> oc = old;
  cpu_leapfrog(l, real, cur.data(), oc.data(), full, s.data() + 1, 0.83, nullptr);
  CHECK(std::memcmp(oa.data(), oc.data(), oa.size() * sizeof(double)) != 0);
  // one node by hand: the fixed form
  const i64 o = l.off(3, 4, 5);
  const double u = cur[static_cast<size_t>(o)], c2 = 2.0 * u;
  auto at = [&](i64 d) { return cur[static_cast<size_t>(o + d)]; };
  const double lap = std::fma(real.rz, at(1) - c2 + at(-1),
                              std::fma(real.ry, at(l.pitch) - c2 + at(-l.pitch), at(l.plane) - c2 + at(-l.plane)));
  CHECK(oc[static_cast<size_t>(o)] == std::fma(real.lam, lap, c2 - old[static_cast<size_t>(o)]));
}

// ---- the CPU solver on a box against the discrete solution's closed form (SURVEY.md §1.6 with the box eigenvalue
// λ_h = 4·sin²(π/(2N))·Σ 1/h_d²): L∞ error = |cos nθ − cos(a_t nτ)|·max φ, cos θ = 1 − τ²λ_h/2. In double here: the two
// cosines differ by ~1e-7 at this shape and each side carries ~1e-15 of rounding, so they agree to ~1e-8 relative; the
// bound is 1e-5 (the comparison to 1e-6 against the 50-digit oracle is tests/test_box_cpu.py). A swapped ry / rz
// changes λ_h by O(1). All three cyclic permutations of the edges.
void test_cpu_solver_box() {
  const double e[3] = {1.0, 1.3, 0.7};
  for (int s = 0; s < 3; ++s) {
    const i64 N = 16;
    const Problem p = make(N, 1e-3, 6, e[s % 3], e[(s + 1) % 3], e[(s + 2) % 3]);
    CpuSolver cs(p, 2, 2);
    const CpuResult r = cs.run();
    CHECK(r.finite && r.steps.size() == 3 && r.steps.back() == 6);
    const double sn = std::sin(M_PI / (2.0 * N));
    const double lam = 4.0 * sn * sn * p.inv_h2_sum();
    const double theta = std::acos(1.0 - p.tau * p.tau * lam / 2.0);
    double smax = 0.0;
    for (i64 i = 0; i <= N; ++i) smax = std::fmax(smax, std::fabs(std::sin(M_PI * i / N)));
    for (size_t k = 0; k < r.steps.size(); ++k) {
      const int n = r.steps[k];
      const double want = std::fabs(std::cos(n * theta) - std::cos(p.a_t() * n * p.tau)) * smax * smax * smax;
      CHECK(want > 1e-9);
      CHECK(std::fabs(r.max_err[k] - want) <= 1e-5 * want);
    }
  }
}

}  // namespace

int main() {
  test_cube_unchanged();
  test_box_values();
  test_schedule_independent_of_edges();
  test_cpu_box_form_with_unit_ratios();
  test_cpu_solver_box();
  std::printf("test_box: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
