// Native unit tests of the sponge layers' host side (no GPU): sponge_tables (the quadratic ramp, symmetric and one-sided
// faces, a rectangular box's per-axis default sigma, r = 1/(1 + g) entry by entry), sponge_boxes (disjoint boxes whose
// union is exactly the slabs d < W + steps − 1, for N = 24 and 40, W = 1, 4, 8, steps = 2..5, every single face, the opposite
// pairs and all six — N = 24, W = 8, steps = 5 included, where opposite slabs leave one node between them; at W = 11 they
// overlap and merge, as opposite pairs alone and on all six faces), Problem::validate's refusals, and
// CpuSolver with a sponge: nodes outside the layers' reach keep the undamped solve's bits over a few steps.
//
// Built and run by CMake/ctest (CMakeLists.txt) and, with host AddressSanitizer + UBSan, by tests/test_sponge_native.py.
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

Problem make(i64 N, int K, int W, double sigma, int faces, bool box = false) {
  Problem p;
  p.N = N;
  p.K = K;
  p.L = 1.0;
  if (box) {
    p.Ly = 1.3;
    p.Lz = 0.7;
  }
  p.tau = 0.9 * p.tau_max();
  p.sponge = Sponge{W, sigma, faces};
  p.validate();
  return p;
}

bool refused(const Problem& p, const char* needle) {
  try {
    p.validate();
  } catch (const std::exception& e) {
    return std::strstr(e.what(), "sponge:") != nullptr && std::strstr(e.what(), needle) != nullptr;
  }
  return false;
}

void check_tables() {
  {  // all six faces, a cube: symmetric, zero outside the layers, the ramp's values
    const Problem p = make(24, 4, 6, 0.0, 63);
    const SpongeTables t = sponge_tables(p);
    const double sig = 3.0 * std::log(1000.0) / (2.0 * 6.0 * p.hx());
    for (int a = 0; a < 3; ++a) {
      CHECK(t.g[a].size() == 27 && t.r[a].size() == 27);
      CHECK(t.g[a][0] == 0.0 && t.g[a][1] == 0.0 && t.g[a][25] == 0.0 && t.g[a][26] == 0.0);  // nodes −1, 0, N, N + 1
      for (i64 i = 1; i < 24; ++i) {
        const size_t e = static_cast<size_t>(i + 1);
        const i64 d = i < 24 - i ? i : 24 - i;
        CHECK(t.g[a][e] == t.g[a][static_cast<size_t>(24 - i + 1)]);
        CHECK((t.g[a][e] > 0.0) == (d < 6));
        if (d < 6) {
          const double q = static_cast<double>(6 - d) / 6.0;
          CHECK(std::fabs(t.g[a][e] - p.tau * sig * q * q) <= 4e-16 * t.g[a][e]);
        }
        CHECK(t.r[a][e] == 1.0 / (1.0 + t.g[a][e]));
      }
      CHECK(t.g[a][2] > t.g[a][3] && t.g[a][6] > 0.0 && t.g[a][7] == 0.0);  // decreasing inwards; d = 5 damped, d = 6 not
    }
  }
  {  // one-sided faces on a box: x−, y+, both z; per-axis default sigma; an explicit sigma is the same on every axis
    const Problem p = make(40, 4, 8, 0.0, 1 | 8 | 16 | 32, true);
    const SpongeTables t = sponge_tables(p);
    CHECK(t.g[0][2] > 0.0 && t.g[0][40] == 0.0);   // x: node 1 damped, node 39 not
    CHECK(t.g[1][2] == 0.0 && t.g[1][40] > 0.0);   // y: the other way round
    CHECK(t.g[2][2] > 0.0 && t.g[2][40] == t.g[2][2]);
    CHECK(sponge_sigma(p, 1) < sponge_sigma(p, 0) && sponge_sigma(p, 0) < sponge_sigma(p, 2));  // ∝ 1/h_a
    const Problem q = make(40, 4, 8, 2.5, 63, true);
    const SpongeTables u = sponge_tables(q);
    CHECK(u.g[0][2] == u.g[1][2] && u.g[1][2] == u.g[2][2] && u.g[0][2] == q.tau * 2.5 * (49.0 / 64.0));
  }
  {  // width 0 / faces 0: no entry is set; the widest layers that fit (2 W = N − 2)
    CHECK(!make(24, 4, 0, 0.0, 63).sponge.on() && !make(24, 4, 5, 0.0, 0).sponge.on());
    const SpongeTables z = sponge_tables(make(24, 4, 5, 0.0, 0));
    for (double g : z.g[1]) CHECK(g == 0.0);
    const SpongeTables t = sponge_tables(make(24, 4, 11, 0.0, 63));
    // nodes 10 | 11, 12, 13 | 14: d = 10 from a face is damped, d = 11 = W and beyond is not
    CHECK(t.g[0][11] > 0.0 && t.g[0][12] == 0.0 && t.g[0][13] == 0.0 && t.g[0][14] == 0.0 && t.g[0][15] > 0.0);
  }
}

void check_boxes(i64 N, int W, int steps, int faces) {
  const Problem p = make(N, 4, W, 0.0, faces);
  const Layout l = make_layout(p, Box{0, N + 1, 0, N + 1, 0, N + 1});
  const std::vector<LBox> boxes = sponge_boxes(p, l, steps);
  CHECK(boxes.size() <= 6);
  std::vector<int> cover(static_cast<size_t>((N + 1) * (N + 1) * (N + 1)), 0);
  for (const LBox& b : boxes) {
    CHECK(!b.empty() && b.x0 >= 1 && b.x1 <= N && b.y0 >= 1 && b.y1 <= N && b.z0 >= 1 && b.z1 <= N);
    for (i64 x = b.x0; x < b.x1; ++x)
      for (i64 y = b.y0; y < b.y1; ++y)
        for (i64 z = b.z0; z < b.z1; ++z) ++cover[static_cast<size_t>((x * (N + 1) + y) * (N + 1) + z)];
  }
  const i64 reach = W + steps - 1;
  bool ok = true;
  for (i64 x = 0; x <= N && ok; ++x)
    for (i64 y = 0; y <= N && ok; ++y)
      for (i64 z = 0; z <= N; ++z) {
        const i64 c[3] = {x, y, z};
        bool in = false, interior = true;
        for (int a = 0; a < 3; ++a) {
          interior = interior && c[a] > 0 && c[a] < N;
          if (((faces >> (2 * a)) & 1) && c[a] < reach) in = true;
          if (((faces >> (2 * a + 1)) & 1) && N - c[a] < reach) in = true;
        }
        if (cover[static_cast<size_t>((x * (N + 1) + y) * (N + 1) + z)] != ((in && interior) ? 1 : 0)) {
          ok = false;
          std::fprintf(stderr, "sponge_boxes N=%lld W=%d steps=%d faces=%d: node %lld %lld %lld covered %d times\n",
                       static_cast<long long>(N), W, steps, faces, static_cast<long long>(x), static_cast<long long>(y),
                       static_cast<long long>(z), cover[static_cast<size_t>((x * (N + 1) + y) * (N + 1) + z)]);
          break;
        }
      }
  CHECK(ok);
}

void check_validate() {
  Problem p = make(24, 4, 0, 0.0, 63);
  p.sponge = Sponge{-1, 0.0, 63};
  CHECK(refused(p, "width"));
  p.sponge = Sponge{12, 0.0, 63};
  CHECK(refused(p, "2 * width"));
  p.sponge = Sponge{11, 0.0, 63};
  p.validate();
  p.sponge = Sponge{4, -1.0, 1};
  CHECK(refused(p, "sigma"));
  p.sponge = Sponge{4, std::nan(""), 1};
  CHECK(refused(p, "sigma"));
  p.sponge = Sponge{4, INFINITY, 1};
  CHECK(refused(p, "sigma"));
  p.sponge = Sponge{4, 0.0, 64};
  CHECK(refused(p, "faces"));
  p.sponge = Sponge{12, -1.0, 0};  // (faces = 0: no sponge, nothing to refuse)
  p.validate();
}

// CpuSolver from the eigenmode with a layer at x−: after K steps a node farther than W + K − 1 from the face holds the
// undamped solve's bits, and the nodes of the layer do not
void check_solver() {
  const int K = 5, W = 4;
  Problem plain = make(24, K, 0, 0.0, 63);
  Problem damped = make(24, K, W, 0.0, 1);
  CpuSolver a(plain, 2, 2), b(damped, 2, 2);
  a.run();
  b.run();
  const Layout& l = a.layout();
  bool far_equal = true, near_differs = false;
  for (i64 x = 1; x < 24; ++x)
    for (i64 y = 1; y < 24; ++y)
      for (i64 z = 1; z < 24; ++z) {
        const double u = a.field(0)[static_cast<size_t>(l.off(x, y, z))], v = b.field(0)[static_cast<size_t>(l.off(x, y, z))];
        const bool same = std::memcmp(&u, &v, sizeof u) == 0;
        // (K − 1 leapfrog steps follow the start: the difference reaches d < W + K − 2)
        if (x >= W + K - 2) far_equal = far_equal && same;
        if (x < W && !same) near_differs = true;
      }
  CHECK(far_equal);
  CHECK(near_differs);
}

}  // namespace

int main() {
  try {
    check_tables();
    const int face_sets[] = {1, 2, 4, 8, 16, 32, 3, 12, 48, 63};
    for (i64 N : {i64{24}, i64{40}})
      for (int W : {1, 4, 8})
        for (int steps = 2; steps <= 5; ++steps)
          for (int faces : face_sets) check_boxes(N, W, steps, faces);
    // overlapping opposite slabs merge into one interval: a pair alone (the other axes undamped), and all six (one box)
    for (int steps = 2; steps <= 5; ++steps)
      for (int faces : {3, 12, 48, 63}) check_boxes(24, 11, steps, faces);
    check_validate();
    check_solver();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 1;
  }
  std::printf("test_sponge: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
