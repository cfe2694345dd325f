// Native unit tests of the receivers' host side (no GPU): plan_receivers over one rank, slab and block decompositions
// (every slot owned exactly once, offsets equal Layout::off, out-of-range nodes refused) and CpuSolver's traces
// (row n equals the field of a K = n solve at the nodes; receivers on a global face record +0.0).
//
// Built and run by CMake/ctest (CMakeLists.txt) and, with host AddressSanitizer + UBSan, by
// tests/test_receivers_native.py. Exit status 0 = all checks passed; every failure prints its location.
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
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

Problem make(i64 N, int K) {
  Problem p;
  p.N = N;
  p.K = K;
  p.L = 1.0;
  p.tau = 0.5 * p.tau_max();
  p.validate();
  return p;
}

using Node = std::array<i64, 3>;

// The common receiver set for N and a decomposition: per axis the nodes 0, 1, N − 1, N with mid-range values on the
// other axes; the first and last owned node of every rank along every split axis; the eight corners of every rank box
// of a block decomposition; one node listed twice; 48 seeded random nodes.
std::vector<Node> receiver_set(const Problem& p, const Dims& d) {
  const i64 N = p.N;
  std::vector<Node> v;
  const i64 mid[3] = {N / 2, N / 3, (2 * N) / 3};
  for (int a = 0; a < 3; ++a)
    for (i64 e : {i64{0}, i64{1}, N - 1, N}) {
      Node n = {mid[0], mid[1], mid[2]};
      n[static_cast<size_t>(a)] = e;
      v.push_back(n);
    }
  const int parts[3] = {d.px, d.py, d.pz};
  for (int a = 0; a < 3; ++a)
    for (int c = 0; c < parts[a] && parts[a] > 1; ++c) {
      i64 b = 0, e = 0;
      split_axis(N, parts[a], c, &b, &e);
      for (i64 x : {b, e - 1}) {
        Node n = {mid[0], mid[1], mid[2]};
        n[static_cast<size_t>(a)] = x;
        v.push_back(n);
      }
    }
  if (d.py > 1 || d.pz > 1)
    for (int r = 0; r < d.size(); ++r) {
      const Box b = rank_box(p, d, r);
      for (i64 x : {b.x0, b.x1 - 1})
        for (i64 y : {b.y0, b.y1 - 1})
          for (i64 z : {b.z0, b.z1 - 1}) v.push_back(Node{x, y, z});
    }
  v.push_back(v[5]);
  std::uint64_t s = 0x9E3779B97F4A7C15ull * static_cast<std::uint64_t>(N + 7);
  auto next = [&] {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<i64>((s >> 33) % static_cast<std::uint64_t>(N + 1));
  };
  for (int k = 0; k < 48; ++k) {
    const i64 x = next(), y = next(), z = next();
    v.push_back(Node{x, y, z});
  }
  return v;
}

void check_plan(const Problem& p, const Dims& d) {
  const std::vector<Node> nodes = receiver_set(p, d);
  std::vector<int> owners(nodes.size(), 0);
  for (int r = 0; r < d.size(); ++r) {
    // (ghost depths as a deep-tb rank has them: the offsets must follow the layout, whatever its depths)
    const Layout l = make_layout(p, rank_box(p, d, r), 16, d.px > 1 ? 5 : 1, d.py > 1 ? 3 : 1, d.pz > 1 ? 2 : 1);
    const std::vector<Receiver> mine = plan_receivers(p, d, r, l, nodes);
    i64 last = -1;
    for (const Receiver& q : mine) {
      CHECK(q.slot > last);  // list order
      last = q.slot;
      CHECK(q.slot >= 0 && q.slot < static_cast<i64>(nodes.size()));
      if (q.slot < 0 || q.slot >= static_cast<i64>(nodes.size())) continue;
      ++owners[static_cast<size_t>(q.slot)];
      const Node& n = nodes[static_cast<size_t>(q.slot)];
      CHECK(q.x >= 0 && q.x < l.nx && q.y >= 0 && q.y < l.ny && q.z >= 0 && q.z < l.nz);
      CHECK(q.x + l.gx0 == n[0] && q.y + l.gy0 == n[1] && q.z + l.gz0 == n[2]);
      CHECK(q.off == l.off(q.x, q.y, q.z));
      CHECK(q.off >= 0 && q.off < l.total);
    }
  }
  for (int c : owners) CHECK(c == 1);
  // an index outside 0..N is refused, on every rank, with a message that names it
  const Layout l0 = make_layout(p, rank_box(p, d, 0));
  for (const Node& bad : {Node{-1, 3, 3}, Node{3, p.N + 1, 3}, Node{3, 3, p.N + 7}}) {
    bool thrown = false;
    try {
      std::vector<Node> n2 = nodes;
      n2.push_back(bad);
      (void)plan_receivers(p, d, 0, l0, n2);
    } catch (const std::exception& e) {
      thrown = std::strstr(e.what(), "outside the grid") != nullptr;
    }
    CHECK(thrown);
  }
}

std::vector<i64> flat(const std::vector<Node>& nodes) {
  std::vector<i64> v;
  for (const Node& n : nodes) v.insert(v.end(), n.begin(), n.end());
  return v;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

void check_cpu_traces(i64 N) {
  const int K = 12;
  const Problem p = make(N, K);
  const std::vector<Node> nodes = receiver_set(p, Dims{2, 2, 2});
  const std::vector<i64> ijk = flat(nodes);
  const int R = static_cast<int>(nodes.size());
  CpuSolver s(p, 2, 0);
  s.set_receivers(ijk.data(), R);
  CHECK(s.receivers() == R);
  s.run();
  const std::vector<double> tr = s.traces();
  CHECK(tr.size() == static_cast<size_t>(K + 1) * static_cast<size_t>(R));
  if (tr.size() != static_cast<size_t>(K + 1) * static_cast<size_t>(R)) return;
  for (double v : tr) CHECK(!std::isnan(v));
  // face receivers: +0.0 at every level
  for (int r = 0; r < R; ++r) {
    const Node& n = nodes[static_cast<size_t>(r)];
    const bool face = n[0] == 0 || n[0] == N || n[1] == 0 || n[1] == N || n[2] == 0 || n[2] == N;
    for (int m = 0; m <= K && face; ++m) CHECK(same_bits(tr[static_cast<size_t>(m) * R + r], 0.0));
  }
  // the node listed twice: two equal columns
  for (int m = 0; m <= K; ++m) {
    int twin = -1;
    for (int r = 0; r < R && twin < 0; ++r)
      for (int q = r + 1; q < R; ++q)
        if (nodes[static_cast<size_t>(r)] == nodes[static_cast<size_t>(q)]) {
          CHECK(same_bits(tr[static_cast<size_t>(m) * R + r], tr[static_cast<size_t>(m) * R + q]));
          twin = q;
        }
    CHECK(twin >= 0);
  }
  // row n = the field of a K = n solve without receivers (rows 0 and 1: its u^{K−1} of the K = 1 solve, and u^1)
  for (int n : {0, 1, 2, 7, 12}) {
    Problem q = p;
    q.K = n == 0 ? 1 : n;
    CpuSolver ref(q, 2, 0);
    ref.run();
    const std::vector<double>& f = ref.field(n == 0 ? 1 : 0);
    const Layout& l = ref.layout();
    for (int r = 0; r < R; ++r) {
      const Node& nd = nodes[static_cast<size_t>(r)];
      CHECK(same_bits(tr[static_cast<size_t>(n) * R + r], f[static_cast<size_t>(l.off(nd[0], nd[1], nd[2]))]));
    }
  }
  // out-of-range nodes are refused; R = 0 removes the list
  bool thrown = false;
  try {
    const i64 bad[3] = {0, N + 1, 0};
    s.set_receivers(bad, 1);
  } catch (const std::exception&) {
    thrown = true;
  }
  CHECK(thrown);
  s.set_receivers(nullptr, 0);
  CHECK(s.receivers() == 0);
}

}  // namespace

int main() {
  try {
    const Problem p = make(77, 12);
    check_plan(p, Dims{1, 1, 1});
    check_plan(p, Dims{4, 1, 1});
    check_plan(p, Dims{2, 2, 2});
    check_plan(p, Dims{3, 2, 1});
    check_cpu_traces(77);
    check_cpu_traces(40);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "unexpected exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
