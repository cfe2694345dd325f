// Native unit tests of the point sources' host side (no GPU):
//   * plan_sources at N = 77 over one rank, 4 slabs and 2x2x2 blocks: a source is on exactly the ranks whose allocation
//     its L1 ball meets (brute force over the ball's nodes), the table is ordered by colour class and list order, the
//     classes are the same on every rank, two sources of a class have disjoint balls, face / outside nodes are refused;
//   * cpu_source_response against brute force: a full CpuSolver run from a zero field with one source (N = 16, s =
//     1..5) — bit-equal on the cube, +0.0 off the ball, a corner source at (1, 1, 1) clipped by three faces;
//   * the split identity and its rounding: CpuSolver with sources against unforced cpu_leapfrog passes plus the
//     responses (superposition), from seeded initial data. Prints d_split = max |difference| and umax = max |u| for
//     every configuration: N = 24 with one source and a 5 + 5 split, and the N = 40, K = 12 cube and box configurations
//     of tests/sources_common.py (5 + 5 + 1), whose figures set the tolerance of the fused GPU solves; and the K = 203
//     shot of tests/long_reference.py (two Ricker sources into a field at rest, 40 x 5 + 2), cube and box.
//
// Built and run by CMake/ctest (CMakeLists.txt) and, with host AddressSanitizer + UBSan, by
// tests/test_sources_native.py. Exit status 0 = all checks passed; every failure prints its location.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <vector>

#include "wave3d/cpu.hpp"
#include "wave3d/decomp.hpp"
#include "wave3d/problem.hpp"
#include "wave3d/schedule.hpp"

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

Problem make(i64 N, int K, bool box = false) {
  Problem p;
  p.N = N;
  p.K = K;
  p.L = 1.0;
  if (box) {
    p.Ly = 1.3;
    p.Lz = 0.7;
  }
  p.tau = 0.5 * p.tau_max();
  p.validate();
  return p;
}

using Node = std::array<i64, 3>;

std::vector<i64> flat(const std::vector<Node>& nodes) {
  std::vector<i64> v;
  for (const Node& n : nodes) v.insert(v.end(), n.begin(), n.end());
  return v;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

i64 l1(const Node& a, const Node& b) {
  return std::llabs(a[0] - b[0]) + std::llabs(a[1] - b[1]) + std::llabs(a[2] - b[2]);
}

// seeded values in [−1, 1), the same sequence as tests/sources_common.py lcg_field
struct Lcg {
  std::uint64_t s;
  double next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<double>(s >> 11) / 9007199254740992.0 * 2.0 - 1.0;
  }
};

// the test wavelet: exact small dyadic samples, the same formula as tests/sources_common.py wavelet
double wavelet(int m, int q) { return static_cast<double>((m * 7 + q * 3) % 11 - 5) / 4.0; }

std::vector<Node> source_set(const Problem& p, const Dims& d) {
  const i64 N = p.N;
  std::vector<Node> v = {{N / 2, N / 2, N / 2}, {1, 1, 1},         {N - 1, N / 3, N / 2}, {N / 2, N / 2 + 1, N / 2 + 1},
                         {N / 2, N / 2, N / 2}, {N - 1, N - 1, 1}, {5, 60, 33}};
  // next to and on every rank face and corner
  for (int r = 0; r < d.size(); ++r) {
    const Box b = rank_box(p, d, r);
    for (i64 x : {b.x0, b.x1 - 1, b.x0 + 1})
      for (i64 y : {b.y0, b.y1 - 2})
        for (i64 z : {b.z0 + 3, b.z1 - 1}) {
          const Node n{x, y, z};
          if (x > 0 && x < N && y > 0 && y < N && z > 0 && z < N) v.push_back(n);
        }
  }
  return v;
}

void check_plan(const Problem& p, const Dims& d, int radius) {
  const std::vector<Node> nodes = source_set(p, d);
  std::vector<int> colour(nodes.size(), -1);
  for (int r = 0; r < d.size(); ++r) {
    const Layout l = make_layout(p, rank_box(p, d, r), 16, d.px > 1 ? 5 : 1, d.py > 1 ? 5 : 1, d.pz > 1 ? 5 : 1);
    const SourcePlan plan = plan_sources(p, d, r, l, nodes, radius);
    CHECK(plan.class_begin.size() >= 2 && plan.class_begin.front() == 0 &&
          plan.class_begin.back() == static_cast<int>(plan.table.size()));
    std::vector<char> present(nodes.size(), 0);
    for (int c = 0; c < plan.classes(); ++c) {
      i64 last = -1;
      CHECK(plan.class_begin[static_cast<size_t>(c)] <= plan.class_begin[static_cast<size_t>(c) + 1]);
      for (int k = plan.class_begin[static_cast<size_t>(c)]; k < plan.class_begin[static_cast<size_t>(c) + 1]; ++k) {
        const Source& q = plan.table[static_cast<size_t>(k)];
        CHECK(q.slot > last);  // list order inside a class
        last = q.slot;
        CHECK(q.slot >= 0 && q.slot < static_cast<i64>(nodes.size()));
        if (q.slot < 0 || q.slot >= static_cast<i64>(nodes.size())) continue;
        const size_t slot = static_cast<size_t>(q.slot);
        CHECK(!present[slot]);
        present[slot] = 1;
        CHECK(colour[slot] == -1 || colour[slot] == c);  // the same class on every rank
        colour[slot] = c;
        CHECK(q.x + l.gx0 == nodes[slot][0] && q.y + l.gy0 == nodes[slot][1] && q.z + l.gz0 == nodes[slot][2]);
        CHECK(q.off == (q.x + l.xg) * l.plane + (q.y + l.yg) * l.pitch + (q.z + l.zg + l.zs));
      }
    }
    // on this rank exactly when a node of the ball lies inside the allocation
    for (size_t q = 0; q < nodes.size(); ++q) {
      bool meets = false;
      for (i64 a = -radius; a <= radius && !meets; ++a)
        for (i64 b = -radius; b <= radius && !meets; ++b)
          for (i64 c = -radius; c <= radius && !meets; ++c) {
            if (std::llabs(a) + std::llabs(b) + std::llabs(c) > radius) continue;
            const i64 x = nodes[q][0] + a - l.gx0, y = nodes[q][1] + b - l.gy0, z = nodes[q][2] + c - l.gz0;
            meets = x >= -l.xg && x < l.nx + l.xg && y >= -l.yg && y < l.ny + l.yg && z >= -l.zg && z < l.nz + l.zg;
          }
      CHECK(meets == (present[q] != 0));
    }
  }
  // every source has a class (some rank keeps it), and two of one class are farther apart than 2·radius
  for (size_t a = 0; a < nodes.size(); ++a) {
    CHECK(colour[a] >= 0);
    for (size_t b = a + 1; b < nodes.size(); ++b)
      if (colour[a] == colour[b]) CHECK(l1(nodes[a], nodes[b]) > 2 * radius);
  }
  // greedy in list order: the first source opens class 0, the node listed twice (slots 0 and 4) takes a later class, and
  // so does slot 3 at distance 2 from slot 0
  CHECK(colour[0] == 0 && colour[4] > colour[0] && (radius < 1 || (colour[3] != colour[0] && colour[3] != colour[4])));
  CHECK(colour[1] == 0);  // far from slot 0
  // a node on a global face or outside the grid is refused, with a message that starts with "sources:"
  const Layout l0 = make_layout(p, rank_box(p, d, 0));
  for (const Node& bad : {Node{0, 3, 3}, Node{3, p.N, 3}, Node{3, 3, p.N + 7}, Node{-1, 3, 3}}) {
    bool thrown = false;
    try {
      std::vector<Node> n2 = nodes;
      n2.push_back(bad);
      (void)plan_sources(p, d, 0, l0, n2, radius);
    } catch (const std::exception& e) {
      thrown = std::strncmp(e.what(), "sources:", 8) == 0 || std::strstr(e.what(), "sources:") != nullptr;
    }
    CHECK(thrown);
  }
}

// cpu_source_response against a CpuSolver run from a zero field with one source whose first s samples follow `wavelet`
void check_response(i64 N, const Node& node, bool box) {
  for (int s = 1; s <= kSourceMaxSteps; ++s) {
    // the brute force: K = s + 1 steps from u⁰ = u¹ = 0; sample 0 is zero, so the forcing is a[1 .. s] after steps 1 → 2 …
    // s → s + 1: a pass n = 1 → 1 + s with addends a[1 .. s]
    const int K = s + 1;
    const Problem p = make(N, K, box);
    const Coeffs c = Coeffs::from(p);
    std::vector<double> w(static_cast<size_t>(K), 0.0), a(static_cast<size_t>(K), 0.0);
    for (int m = 1; m < K; ++m) w[static_cast<size_t>(m)] = wavelet(m, 2);
    for (int m = 0; m < K; ++m) a[static_cast<size_t>(m)] = source_addend(p, w[static_cast<size_t>(m)]);
    CpuSolver sol(p, 0, 0);
    const std::vector<double> zero(static_cast<size_t>((N + 1) * (N + 1) * (N + 1)), 0.0);
    sol.set_initial(zero.data(), zero.data());
    sol.set_sources(node.data(), 1, w.data());
    CHECK(sol.sources() == 1);
    sol.run();
    std::vector<double> last(kSourceCells), prev(kSourceCells);
    cpu_source_response(p, c, node.data(), a.data() + 1, false, s, last.data(), prev.data());
    const Layout& l = sol.layout();
    i64 nonzero = 0;
    for (i64 gx = 0; gx <= N; ++gx)
      for (i64 gy = 0; gy <= N; ++gy)
        for (i64 gz = 0; gz <= N; ++gz) {
          const i64 i = gx - node[0], j = gy - node[1], k = gz - node[2];
          const double f0 = sol.field(0)[static_cast<size_t>(l.off(gx, gy, gz))];
          const double f1 = sol.field(1)[static_cast<size_t>(l.off(gx, gy, gz))];
          const bool in = std::llabs(i) <= kSourceRadius && std::llabs(j) <= kSourceRadius && std::llabs(k) <= kSourceRadius;
          if (!in) {
            CHECK(same_bits(f0, 0.0) && same_bits(f1, 0.0));
            continue;
          }
          const size_t q = static_cast<size_t>(((i + kSourceRadius) * kSourceSide + (j + kSourceRadius)) * kSourceSide + (k + kSourceRadius));
          CHECK(same_bits(last[q], f0));
          CHECK(same_bits(prev[q], f1));
          const i64 dist = std::llabs(i) + std::llabs(j) + std::llabs(k);
          if (dist > s - 1) CHECK(same_bits(last[q], 0.0));
          if (dist > s - 2) CHECK(same_bits(prev[q], 0.0));
          if (last[q] != 0.0) ++nonzero;
        }
    CHECK(nonzero > 0);
    // cells of the cube outside the grid stay +0.0
    for (int i = -kSourceRadius; i <= kSourceRadius; ++i)
      for (int j = -kSourceRadius; j <= kSourceRadius; ++j)
        for (int k = -kSourceRadius; k <= kSourceRadius; ++k) {
          const i64 gx = node[0] + i, gy = node[1] + j, gz = node[2] + k;
          if (gx > 0 && gx < N && gy > 0 && gy < N && gz > 0 && gz < N) continue;
          const size_t q = static_cast<size_t>(((i + kSourceRadius) * kSourceSide + (j + kSourceRadius)) * kSourceSide + (k + kSourceRadius));
          CHECK(same_bits(last[q], 0.0) && same_bits(prev[q], 0.0));
        }
  }
  // the start level: ½·a[0] at the node, nothing else
  const Problem p = make(N, 3, box);
  const double a0 = source_addend(p, 1.25);
  std::vector<double> last(kSourceCells), prev(kSourceCells);
  cpu_source_response(p, Coeffs::from(p), node.data(), &a0, true, 1, last.data(), prev.data());
  for (int q = 0; q < kSourceCells; ++q) {
    CHECK(same_bits(last[static_cast<size_t>(q)], q == kSourceCells / 2 ? 0.5 * a0 : 0.0));
    CHECK(same_bits(prev[static_cast<size_t>(q)], 0.0));
  }
}

// the long shot's wavelets: Ricker samples rounded to multiples of 2^-16, the same formula as tests/long_reference.py
// ricker16 (the rounding keeps the last bits of exp out of the samples; their sum is exact in any order)
double ricker16(double f0, double t0, double tau, int m, double amp) {
  const double t = static_cast<double>(m) * tau - t0;
  const double a = (3.141592653589793 * f0) * t;
  return std::nearbyint(amp * ((1.0 - 2.0 * (a * a)) * std::exp(-(a * a))) * 65536.0) / 65536.0;
}

// The split identity: CpuSolver with sources against passes of `split` steps without forcing plus the responses.
// long_shot: zero initial data and the two Ricker wavelets of tests/long_reference.py long_shot instead of the seeded
// data and the dyadic test wavelet.
void check_split(const char* name, i64 N, int K, bool box, double tau, const std::vector<Node>& nodes,
                 const std::vector<int>& split, bool long_shot = false) {
  Problem p = make(N, K, box);
  p.tau = tau;
  p.validate();
  const Coeffs c = Coeffs::from(p);
  const int Q = static_cast<int>(nodes.size());
  const size_t n3 = static_cast<size_t>((N + 1) * (N + 1) * (N + 1));
  std::vector<double> phi(n3), psi(n3), w(static_cast<size_t>(K) * static_cast<size_t>(Q));
  Lcg g{0x9E3779B97F4A7C15ull};
  for (double& v : phi) v = g.next();
  for (double& v : psi) v = g.next();
  for (int m = 0; m < K; ++m)
    for (int q = 0; q < Q; ++q) w[static_cast<size_t>(m) * Q + q] = wavelet(m, q);
  if (long_shot) {
    CHECK(Q == 2);
    std::fill(phi.begin(), phi.end(), 0.0);
    std::fill(psi.begin(), psi.end(), 0.0);
    const double f0[2] = {static_cast<double>(N) / 10.0, static_cast<double>(N) / 8.0}, amp[2] = {1.0, -0.75};
    double wsum = 0.0;
    for (int m = 0; m < K; ++m)
      for (int q = 0; q < 2; ++q) wsum += std::fabs(w[static_cast<size_t>(m) * 2 + q] = ricker16(f0[q], 1.5 / f0[q], tau, m, amp[q]));
    std::printf("long-shot %s: tau = %.17g sum |w| = %.17g\n", name, tau, wsum);
  }
  const std::vector<i64> ijk = flat(nodes);
  CpuSolver ref(p, 0, 0);
  ref.set_initial(phi.data(), psi.data());
  ref.set_sources(ijk.data(), Q, w.data());
  ref.run();
  const std::vector<double> a = source_addends(p, ijk.data(), Q, w.data());
  // the same start, then unforced passes + responses
  const Layout& l = ref.layout();
  const Layout il = initial_layout(p, l);
  std::vector<double> lphi(static_cast<size_t>(il.total)), lpsi(static_cast<size_t>(il.total));
  initial_to_local(il, phi.data(), lphi.data());
  initial_to_local(il, psi.data(), lpsi.data());
  std::vector<double> u[2] = {std::vector<double>(static_cast<size_t>(l.total)), std::vector<double>(static_cast<size_t>(l.total))};
  cpu_first_step_field(l, il, c, p.tau, lphi.data(), lpsi.data(), u[0].data(), u[1].data());
  std::vector<double> last(kSourceCells), prev(kSourceCells), col(static_cast<size_t>(kSourceMaxSteps));
  auto add = [&](const Node& nd, int q, int n, int s, bool start, std::vector<double>& ulast, std::vector<double>& uprev) {
    for (int k = 0; k < s; ++k) col[static_cast<size_t>(k)] = a[static_cast<size_t>(n + k) * Q + q];
    cpu_source_response(p, c, nd.data(), col.data(), start, s, last.data(), prev.data());
    for (int i = -kSourceRadius; i <= kSourceRadius; ++i)
      for (int j = -kSourceRadius; j <= kSourceRadius; ++j)
        for (int k = -kSourceRadius; k <= kSourceRadius; ++k) {
          const i64 gx = nd[0] + i, gy = nd[1] + j, gz = nd[2] + k;
          if (gx <= 0 || gx >= N || gy <= 0 || gy >= N || gz <= 0 || gz >= N) continue;
          const size_t cq = static_cast<size_t>(((i + kSourceRadius) * kSourceSide + (j + kSourceRadius)) * kSourceSide + (k + kSourceRadius));
          ulast[static_cast<size_t>(l.off(gx, gy, gz))] += last[cq];
          uprev[static_cast<size_t>(l.off(gx, gy, gz))] += prev[cq];
        }
  };
  for (int q = 0; q < Q; ++q) add(nodes[static_cast<size_t>(q)], q, 0, 1, true, u[1], u[0]);
  const std::vector<double> table = sin_table_ext(p);
  int cur = 1, old = 0, n = 1, total = 0;
  double umax_run = 0.0;
  for (int s : split) total += s;
  CHECK(1 + total == K);
  for (int s : split) {
    for (int k = 0; k < s; ++k) {
      cpu_leapfrog(l, c, u[cur].data(), u[old].data(), compute_box(l), table.data() + 1, 0.0, nullptr);
      std::swap(cur, old);
    }
    for (int q = 0; q < Q; ++q) add(nodes[static_cast<size_t>(q)], q, n, s, false, u[cur], u[old]);
    n += s;
    // (the long shot: its largest values occur while the wavelets fire, long before K, and the traces hold them — umax is
    // taken over the levels at every pass boundary, not over the two last levels alone)
    if (long_shot)
      for (const std::vector<double>* f : {&u[cur], &u[old]})
        for (double v : *f) umax_run = std::fmax(umax_run, std::fabs(v));
  }
  double d_split = 0.0, umax = umax_run;
  for (int which = 0; which < 2; ++which) {
    const std::vector<double>& f = ref.field(which);
    const std::vector<double>& h = u[which == 0 ? cur : old];
    for (size_t k = 0; k < f.size(); ++k) {
      d_split = std::fmax(d_split, std::fabs(f[k] - h[k]));
      umax = std::fmax(umax, std::fabs(f[k]));
    }
  }
  std::printf("split %s N=%lld K=%d: d_split = %.17g umax = %.17g\n", name, static_cast<long long>(N), K, d_split, umax);
  CHECK(std::isfinite(d_split) && std::isfinite(umax) && umax > 0.0);
  // the identity holds to rounding: far below the field's size (a wrong response or addend index shows at order umax)
  CHECK(d_split <= 1e-9 * umax);
}

}  // namespace

int main() {
  try {
    const Problem p = make(77, 12);
    for (int radius : {4, 0}) {
      check_plan(p, Dims{1, 1, 1}, radius);
      check_plan(p, Dims{4, 1, 1}, radius);
      check_plan(p, Dims{2, 2, 2}, radius);
    }
    for (bool box : {false, true}) {
      check_response(16, Node{8, 7, 9}, box);
      check_response(16, Node{1, 1, 1}, box);
      check_response(16, Node{15, 8, 14}, box);
    }
    check_split("one-source", 24, 11, false, 0.008, {Node{12, 11, 13}}, {5, 5});
    // tests/sources_common.py SOURCES_40 (the fused GPU solves' configurations)
    const std::vector<Node> s40 = {{20, 20, 20}, {1, 1, 1},    {39, 17, 22}, {31, 32, 9}, {32, 10, 31},
                                   {20, 21, 21}, {20, 20, 20}, {10, 20, 20}, {11, 5, 5}};
    check_split("cube", 40, 12, false, 0.005, s40, {5, 5, 1});
    check_split("box", 40, 12, true, 0.005, s40, {5, 5, 1});
    // tests/long_reference.py long_shot(40, box): K = 203 at 0.9 tau_max, 40 passes of 5 steps and one of 2 (the long
    // fused GPU solves' configurations, tests/test_gpu_long_solves.py)
    std::vector<int> split203(40, 5);
    split203.push_back(2);
    for (bool box : {false, true}) {
      const double tau = 0.9 * make(40, 203, box).tau_max();
      check_split(box ? "long-box" : "long-cube", 40, 203, box, tau, {Node{19, 20, 21}, Node{21, 19, 20}}, split203, true);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "unexpected exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
