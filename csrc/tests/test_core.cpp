// Native unit tests of the host-side core (no GPU): decomposition, layout, halo plans, scheme, CPU solver, and the
// solve schedule (schedule.hpp: modes, unit lists, messages, shell boxes, traffic, the error-log combine).
//
// SURVEY.md §4.2 "unit (C++/ctest)": exact-arithmetic checks of the pieces every backend shares. Built and run by
// CMake/ctest (CMakeLists.txt) and, with host AddressSanitizer + UBSan, by tests/test_native_unit.py.
// Exit status 0 = all checks passed; every failure prints its location.
#include <cmath>
#include <cstdio>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "wave3d/cpu.hpp"
#include "wave3d/decomp.hpp"
#include "wave3d/pass_grid.hpp"
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

template <class F>
bool throws(F&& f) {
  try {
    f();
  } catch (const std::exception&) {
    return true;
  }
  return false;
}

// f throws an error whose message contains `what`
template <class F>
bool throws_with(F&& f, const std::string& what) {
  try {
    f();
  } catch (const std::exception& e) {
    return std::string(e.what()).find(what) != std::string::npos;
  }
  return false;
}

// split_axis: the parts tile 0..N exactly once, interior work differs by at most one node between parts
void test_split_axis() {
  for (i64 N : {2, 3, 7, 64, 127, 512, 2048}) {
    for (int p = 1; p <= 32; ++p) {
      if (p > N - 1) continue;
      i64 expect = 0, mn = 1 << 30, mx = 0;
      for (int c = 0; c < p; ++c) {
        i64 b = 0, e = 0;
        split_axis(N, p, c, &b, &e);
        CHECK(b == expect);
        CHECK(e > b);
        expect = e;
        const i64 work = std::min(e, N) - std::max<i64>(b, 1);
        mn = std::min(mn, work);
        mx = std::max(mx, work);
      }
      CHECK(expect == N + 1);
      CHECK(mx - mn <= 1);
    }
  }
}

// every decomposition: boxes partition the grid, neighbours are adjacent, x faces contiguous, y/z faces packed
void test_decompositions() {
  const std::vector<std::pair<std::string, int>> cases = {
      {"slab", 1}, {"slab", 2}, {"slab", 3}, {"slab", 8}, {"slab", 16}, {"block", 4}, {"block", 7},
      {"block", 8}, {"block", 10}, {"block", 20}, {"block", 32}, {"2x2x2", 8}, {"1x2x3", 6}, {"4x1x2", 8}};
  for (const auto& [spec, P] : cases) {
    for (i64 N : {40, 65}) {
      Problem pr;
      pr.N = N;
      const Dims d = parse_dims(spec, P, N);
      CHECK(d.size() == P);
      i64 total = 0;
      for (int r = 0; r < P; ++r) {
        const Box b = rank_box(pr, d, r);
        total += b.count();
        for (int axis = 0; axis < 3; ++axis)
          for (int side = 0; side < 2; ++side) {
            const int q = neighbor_rank(d, r, axis, side);
            if (q < 0) continue;
            CHECK(neighbor_rank(d, q, axis, 1 - side) == r);
            const Box c = rank_box(pr, d, q);
            const i64 lo[3] = {b.x0, b.y0, b.z0}, hi[3] = {b.x1, b.y1, b.z1};
            const i64 clo[3] = {c.x0, c.y0, c.z0}, chi[3] = {c.x1, c.y1, c.z1};
            CHECK(side ? chi[axis] > hi[axis] && clo[axis] == hi[axis] : chi[axis] == lo[axis]);
          }
        // halo plan: message sizes agree with the peer's matching face
        const Layout l = make_layout(pr, b);
        const HaloPlan h = make_halo_plan(l, d, r);
        for (const Face& f : h.faces) {
          const Layout lq = make_layout(pr, rank_box(pr, d, f.peer));
          const HaloPlan hq = make_halo_plan(lq, d, f.peer);
          int matches = 0;
          for (const Face& g : hq.faces)
            if (g.peer == r && g.axis == f.axis && g.side == 1 - f.side) {
              ++matches;
              CHECK(g.count == f.count);
            }
          CHECK(matches == 1);
          CHECK(f.contiguous == (f.axis == 0));
        }
      }
      CHECK(total == (N + 1) * (N + 1) * (N + 1));
    }
  }
  CHECK(throws([] { parse_dims("2x2x3", 8, 64); }));
  CHECK(throws([] { parse_dims("pencil", 8, 64); }));
  const Dims b8 = block_dims(8, 512);
  CHECK(b8.px == 2 && b8.py == 2 && b8.pz == 2);
}

// layout: 64-bit offsets at 2049³, 128-byte aligned rows, first updated node of a row on a line boundary
void test_layout() {
  Problem pr;
  pr.N = 2048;
  const Layout l = make_layout(pr, rank_box(pr, Dims{1, 1, 1}, 0));
  CHECK(l.total > (i64{1} << 33));  // > 8.6e9 doubles: needs 64-bit indexing
  CHECK(l.off(l.nx, l.ny, l.nz) < l.total);
  CHECK(l.off(-1, -1, -1) >= 0);
  CHECK(l.pitch % 16 == 0);
  CHECK((l.cz0 + 1 + l.zs) % 16 == 0);
  for (i64 xg : {1, 2, 4}) {
    pr.N = 70;
    const Layout m = make_layout(pr, rank_box(pr, Dims{3, 1, 1}, 1), 16, xg);
    CHECK(m.plane_off(-xg) == 0);
    CHECK(m.plane_off(m.nx + xg) == m.total);
    CHECK(m.off(0, 0, 0) == m.plane_off(0) + m.pitch + 1 + m.zs);
    for (i64 x = -xg; x <= m.nx + xg - 1; ++x) CHECK(m.kbase() + (x + 1) * m.plane == m.plane_off(x));  // kernel base
  }
}

// Δ_h is exact on quadratics when h is a power of two: u = x² + 2y² + 3z² → Δu = 12
void test_lap7_quadratic() {  // d2sum · 1/h²
  const double h = 1.0 / 64.0, ih2 = 1.0 / (h * h);
  auto u = [&](int i, int j, int k) {
    const double x = i * h, y = j * h, z = k * h;
    return x * x + 2.0 * y * y + 3.0 * z * z;
  };
  for (int i = 1; i < 10; ++i)
    for (int j = 1; j < 10; ++j)
      for (int k = 1; k < 10; ++k) {
        const double v = d2sum(u(i, j, k), u(i - 1, j, k), u(i + 1, j, k), u(i, j - 1, k), u(i, j + 1, k),
                              u(i, j, k - 1), u(i, j, k + 1));
        CHECK(v * ih2 == 12.0);
      }
  // the leapfrog and first-step formulas
  CHECK(leapfrog(1.5, 0.5, 2.0, 0.25) == 3.0);
  CHECK(first_step(1.0, 4.0, 0.125) == 1.5);
}

void test_problem() {
  Problem p;
  p.N = 512;
  p.tau = 1e-3;
  CHECK(p.cfl_ok());
  CHECK(std::fabs(p.courant() - 0.001 * std::sqrt(3.0) * 512) < 1e-12);
  p.N = 1024;
  CHECK(!p.cfl_ok());  // τ = 1e-3 diverges from N ≈ 578 up
  p.N = 2048;
  p.tau = 2.5e-4;
  CHECK(p.cfl_ok());
  CHECK(p.cell_updates() == 2048.0 * 2048.0 * 2048.0 * 20.0);
  const std::vector<double> s = sin_table_ext(p);
  CHECK(s.size() == static_cast<size_t>(p.N + 3));
  CHECK(s[0] == 0.0 && s[1] == 0.0 && s[static_cast<size_t>(p.N + 1)] == 0.0 && s[static_cast<size_t>(p.N + 2)] == 0.0);
  CHECK(std::fabs(s[static_cast<size_t>(p.N / 2 + 1)] - 1.0) < 1e-15);
  Problem bad;
  bad.N = 1;
  CHECK(throws([&] { bad.validate(); }));
  bad.N = 8;
  bad.tau = -1.0;
  CHECK(throws([&] { bad.validate(); }));
}

// pack → unpack moves a y/z face into the peer's ghost layer and nothing else
void test_pack_unpack() {
  Problem pr;
  pr.N = 20;
  const Dims d{1, 2, 2};
  const Box b = rank_box(pr, d, 0);
  const Layout l = make_layout(pr, b);
  const HaloPlan h = make_halo_plan(l, d, 0);
  std::vector<double> u(static_cast<size_t>(l.total));
  for (size_t i = 0; i < u.size(); ++i) u[i] = static_cast<double>(i);
  for (const Face& f : h.faces) {
    std::vector<double> buf(static_cast<size_t>(f.count));
    cpu_pack_face(l, f, u.data(), buf.data());
    std::vector<double> v(static_cast<size_t>(l.total), -1.0);
    cpu_unpack_face(l, f, buf.data(), v.data());
    i64 written = 0;
    for (size_t i = 0; i < v.size(); ++i) written += v[i] != -1.0;
    CHECK(written == f.count);
    // the value at ghost (x, recv_layer, z) came from (x, send_layer, z)
    if (f.axis == 1) CHECK(v[static_cast<size_t>(l.off(3, f.recv_layer, 4))] == u[static_cast<size_t>(l.off(3, f.send_layer, 4))]);
    if (f.axis == 2) CHECK(v[static_cast<size_t>(l.off(3, 4, f.recv_layer))] == u[static_cast<size_t>(l.off(3, 4, f.send_layer))]);
  }
}

// CPU solver at the reference's sequential config (128³, τ = 1e-3, K = 20): the closed-form oracle values that the
// golden tests pin, all printed digits
void test_cpu_solver_golden() {
  Problem p;
  p.N = 128;
  p.tau = 1e-3;
  p.K = 20;
  CpuSolver s(p, 2, 0);
  const CpuResult r = s.run();
  CHECK(r.steps.size() == 10 && r.steps.back() == 20);
  char buf[64];
  std::snprintf(buf, sizeof buf, "%.6e %.6e", r.max_err.back(), r.rms_err.back());
  CHECK(std::string(buf) == "2.820954e-07 1.009161e-07");
  CHECK(r.finite);
  // boundary nodes are never written: the Dirichlet faces stay exact zeros
  const Layout& l = s.layout();
  const std::vector<double>& u = s.field(0);
  for (i64 j = 0; j <= p.N; j += 7)
    for (i64 k = 0; k <= p.N; k += 5) {
      CHECK(u[static_cast<size_t>(l.off(0, j, k))] == 0.0);
      CHECK(u[static_cast<size_t>(l.off(p.N, j, k))] == 0.0);
    }
}


// ------------------------------------------------------------------------------------------------------------------
// The solve schedule (schedule.hpp). Layouts and plans only: no field is allocated.
// ------------------------------------------------------------------------------------------------------------------
RankSchedule sched(i64 N, int K, const SolverOptions& o, int rank = 0, int world = 1, double free_bytes = 1e13) {
  Problem p;
  p.N = N;
  p.K = K;
  return make_rank_schedule(p, o, rank, world, free_bytes);
}

// the units of a fresh solve, started as GpuSolver::phase_init starts it
std::vector<UnitPlan> fresh_units(const RankSchedule& s) {
  const bool analytic = (s.mode == Mode::kFusedSingle || s.mode == Mode::kDeepTb) && s.analytic_ok();
  return plan_units(s, analytic ? 1 : s.opt.init2 && s.prob.K >= 2 ? 2 : 1, analytic);
}

using Steps = std::vector<std::pair<int, int>>;  // (n, steps) per unit
Steps steps_of(const std::vector<UnitPlan>& u) {
  Steps v;
  for (const UnitPlan& x : u) v.push_back({x.n, x.steps});
  return v;
}

void test_unit_lists() {
  SolverOptions o;
  std::vector<UnitPlan> u = fresh_units(sched(64, 20, o));
  CHECK((steps_of(u) == Steps{{1, 4}, {5, 5}, {10, 5}, {15, 5}}));
  CHECK(u[0].analytic && !u[1].analytic);
  o.tiling_tb.p2 = false;
  u = fresh_units(sched(64, 20, o));
  CHECK((steps_of(u) == Steps{{1, 3}, {4, 4}, {8, 4}, {12, 4}, {16, 4}}));
  CHECK(u[0].analytic);
  o = SolverOptions{};
  o.check_every = 1;  // u¹ carries a check: no analytic start
  CHECK(!sched(64, 20, o).analytic_ok());
  u = fresh_units(sched(64, 20, o));
  CHECK(u[0].n == 2 && !u[0].analytic);
  o = SolverOptions{};
  o.tb = false;  // pairs wherever the intermediate step carries no check
  u = fresh_units(sched(64, 20, o));
  CHECK((steps_of(u) == Steps{{2, 2}, {4, 2}, {6, 2}, {8, 2}, {10, 2}, {12, 2}, {14, 2}, {16, 2}, {18, 2}}));
  o.check_every = 3;  // checks at 3, 6, ..., 18, 20
  u = fresh_units(sched(64, 20, o));
  CHECK((steps_of(u) == Steps{{2, 1}, {3, 2}, {5, 1}, {6, 2}, {8, 1}, {9, 2}, {11, 1}, {12, 2}, {14, 1}, {15, 2},
                              {17, 1}, {18, 2}}));
  o = SolverOptions{};
  o.temporal = 1;
  const RankSchedule s1 = sched(64, 20, o);
  CHECK(s1.mode == Mode::kSingleStep && s1.nbuf == 2);
  u = plan_units(s1, 1, false);
  CHECK(u.size() == 19);
  for (const UnitPlan& x : u) CHECK(x.steps == 1);
  // every unit list covers start_n..K exactly once
  std::vector<SolverOptions> opts(6);
  opts[1].tiling_tb.p2 = false;
  opts[2].tb = false;
  opts[3].temporal = 1;
  opts[4].check_every = 1;
  opts[5].check_every = 3;
  for (const SolverOptions& q : opts)
    for (int K = 3; K <= 25; ++K)
      for (int world : {1, 2}) {
        const RankSchedule s = sched(64, K, q, 0, world);
        u = fresh_units(s);
        CHECK(!u.empty());
        int n = u.empty() ? 0 : u[0].n;
        CHECK(n == 1 || n == 2);
        for (const UnitPlan& x : u) {
          CHECK(x.n == n && x.steps >= 1 && x.steps <= s.opt.temporal);
          n += x.steps;
        }
        CHECK(n == K);
      }
}

void test_mode_table() {
  SolverOptions o;
  for (int world : {2, 4, 8}) {
    const RankSchedule s = sched(512, 20, o, 1, world);
    CHECK(s.mode == Mode::kDeepTb && !s.block_tb && s.mode_name() == "deep-tb" && s.opt.temporal == 5 && s.nbuf == 4);
    CHECK(s.lay.xg == 5 && !s.push);
    SolverOptions p = o;
    p.push = true;
    const RankSchedule t = sched(512, 20, p, 1, world);
    CHECK(t.mode == Mode::kDeepTb && t.push && t.opt.temporal == 4 && t.lay.xg == 4);
  }
  // slab ranks: deep-tb exactly when the smallest rank owns max(tb_min_planes, 2·temporal) = 16 planes
  for (i64 N = 24; N <= 40; ++N) {
    Problem p;
    p.N = N;
    const i64 mn = imin(rank_box(p, Dims{2, 1, 1}, 0).nx(), rank_box(p, Dims{2, 1, 1}, 1).nx());
    CHECK((sched(N, 20, o, 0, 2).mode == Mode::kDeepTb) == (mn >= 16));
  }
  CHECK(sched(64, 20, o, 0, 8).mode != Mode::kDeepTb);  // 7-8 planes per rank
  SolverOptions b = o;
  for (const char* dec : {"2x2x2", "3x3x3"}) {
    b.decomp = dec;
    const int world = dec[0] == '2' ? 8 : 27;
    const RankSchedule s = sched(40, 20, b, 0, world);  // extents 20-21 / 13-14
    CHECK(s.mode == Mode::kDeepTb && s.block_tb && s.mode_name() == "deep-tb-block" && s.opt.temporal == 5);
    CHECK(!s.opt.fused_pack && s.lay.xg == 5 && s.lay.yg == 5 && s.lay.zg == 5 && s.send_total >= s.deep_max);
  }
  // Smallest block extent 9 (N = 17) or 8 (N = 16): block_fits asks for 2·5 nodes, so the ranks fall to single steps
  // and temporal is lowered to 4 all the same. ADVICE.md (round 6, low) calls this a silent regression of the S = 4
  // block passes; the fix (keep deep-tb at temporal 4) changes the next line to Mode::kDeepTb.
  b.decomp = "2x2x2";
  for (i64 N : {16, 17}) {
    const RankSchedule s = sched(N, 20, b, 0, 8);
    CHECK(s.mode == Mode::kSingleStep);
    CHECK(s.opt.temporal == 4 && !s.block_tb && s.nbuf == 2);
  }
  // memory plan at 2049³: four buffers + 2 GB of headroom must fit, else the two-buffer single-step scheme
  const double four = 4.0 * static_cast<double>(sched(2049, 20, o).lay.bytes()) + 2.0e9;
  const RankSchedule lo = sched(2049, 20, o, 0, 1, four - 1e6), hi = sched(2049, 20, o, 0, 1, four + 1e6);
  CHECK(lo.mode == Mode::kSingleStep && lo.nbuf == 2 && lo.mode_name() == "single-step");
  CHECK(hi.mode == Mode::kFusedSingle && hi.nbuf == 4);
  CHECK(throws([&] { sched(2049, 20, o, 0, 1, 1e9); }));
  // every rank of a world gets the same mode and pass depth
  const std::vector<std::pair<std::string, int>> worlds = {{"slab", 3}, {"slab", 8}, {"2x2x2", 8}, {"2x2x1", 4}, {"3x3x3", 27}};
  for (const auto& [dec, world] : worlds)
    for (i64 N : {17, 40, 100, 130}) {
      SolverOptions q;
      q.decomp = dec;
      const RankSchedule r0 = sched(N, 20, q, 0, world);
      for (int r = 1; r < world; ++r) {
        const RankSchedule s = sched(N, 20, q, r, world);
        CHECK(s.mode == r0.mode && s.opt.temporal == r0.opt.temporal && s.block_tb == r0.block_tb && s.nbuf == r0.nbuf);
      }
    }
}

bool boxes_meet(const LBox& a, const LBox& b) {
  return imax(a.x0, b.x0) < imin(a.x1, b.x1) && imax(a.y0, b.y0) < imin(a.y1, b.y1) && imax(a.z0, b.z0) < imin(a.z1, b.z1);
}

// --poison-ghosts of a slab unit whose exchange a pass of w steps follows (plan_poison): the message receive ranges and
// the self-stored plane together are exactly ghost planes [−w, 0) / [nx, nx + w) of u^{n+S} and [−(w − 1), 0) /
// [nx, nx + w − 1) of u^{n+S−1} on the sides that have a neighbour, each plane once, none of them owned; the
// self-stored plane is poisoned before the pass, over the compute box's y / z range, and keeps its zero slot.
void check_poison(const RankSchedule& s, const UnitPlan& u, int w) {
  const std::vector<PoisonRange> pr = plan_poison(s, u);
  if (s.block_tb) {  // (k_box_copy fills the receive regions of the DeepPlan)
    CHECK(pr.empty());
    return;
  }
  const Layout& l = s.lay;
  std::set<i64> got[2], want[2];  // ghost planes of out1 (u^{n+S−1}) / out2 (u^{n+S})
  int self = 0;
  for (const PoisonRange& p : pr) {
    CHECK(p.field == MsgField::kOut1 || p.field == MsgField::kOut2);
    const int f = p.field == MsgField::kOut2 ? 1 : 0;
    CHECK(p.off >= 0 && p.count > 0 && p.rows >= 1);
    const i64 x = p.off / l.plane - l.xg;
    if (p.before_pass) {
      const int side = x < 0 ? 0 : 1;
      CHECK(f == 0 && x == (side == 0 ? -1 : l.nx) && ((u.ghost_bits >> side) & 1));
      CHECK(p.off == l.off(x, s.full.y0, s.full.z0) && p.count == s.full.z1 - s.full.z0 &&
            p.rows == s.full.y1 - s.full.y0 && p.pitch == l.pitch && p.count <= p.pitch);
      CHECK(p.off + (p.rows - 1) * p.pitch + p.count <= l.plane_off(x) + l.zero_off());
      CHECK(got[0].insert(x).second);
      ++self;
    } else {
      CHECK(p.rows == 1 && p.off % l.plane == 0 && p.count % l.plane == 0);
      for (i64 k = 0; k < p.count / l.plane; ++k) CHECK(got[f].insert(x + k).second);
    }
  }
  CHECK(self == (u.ghost_bits & 1) + (u.ghost_bits >> 1));
  for (int side = 0; side < 2; ++side) {
    if (!s.nb[0][side]) continue;
    for (i64 d = 1; d <= w; ++d) want[1].insert(side == 0 ? -d : l.nx - 1 + d);
    for (i64 d = 1; d <= w - 1; ++d) want[0].insert(side == 0 ? -d : l.nx - 1 + d);
  }
  CHECK(got[0] == want[0] && got[1] == want[1]);
  for (int f = 0; f < 2; ++f)
    for (i64 x : got[f]) CHECK((x < 0 || x >= l.nx) && x >= -l.xg && x < l.nx + l.xg);
}

// Every deep-tb world of the matrix: both ends of every message agree, message sizes are the region sizes, and the
// overlapped units' shell boxes and interior tile the compute box on boxes the pair-tiled pass accepts.
void test_deep_tb_worlds() {
  const std::vector<std::pair<std::string, int>> worlds = {{"slab", 2}, {"slab", 3}, {"slab", 4}, {"slab", 5}, {"slab", 6},
                                                           {"slab", 7}, {"slab", 8}, {"2x2x2", 8}, {"2x2x1", 4},
                                                           {"1x2x2", 4}, {"3x3x3", 27}};
  for (const auto& [dec, world] : worlds)
    for (int temporal = 2; temporal <= 5; ++temporal)
      for (int variant = 0; variant < 4; ++variant) {
        SolverOptions o;
        o.decomp = dec;
        o.temporal = temporal;
        o.overlap = (variant & 1) != 0;
        o.ghost_store = (variant & 2) != 0;
        // (slab worlds 7 and 8 own 12-14 planes per rank at N = 100: below the default 16 no N of the set would do)
        o.tb_min_planes = 8;
        // (K = 21: 2-step passes after a 2-step analytic start cannot cover the 19 steps of K = 20 — plan_units
        // refuses that schedule, as build_units always did)
        const int K = 21;
        i64 N = 0;
        for (i64 n : {40, 64, 100})
          if (N == 0 && sched(n, K, o, 0, world).mode == Mode::kDeepTb) N = n;
        CHECK(N != 0);
        if (N == 0) continue;
        std::vector<RankSchedule> rs;
        std::vector<std::vector<UnitPlan>> us;
        for (int r = 0; r < world; ++r) {
          rs.push_back(sched(N, K, o, r, world));
          us.push_back(fresh_units(rs.back()));
          CHECK(rs.back().opt.temporal == temporal && us.back().size() == us[0].size());
        }
        for (int r = 0; r < world; ++r) {
          const RankSchedule& s = rs[static_cast<size_t>(r)];
          CHECK(s.side_stream() == o.overlap && s.late_exchange() == !o.overlap && s.overlapped() == o.overlap);
          for (size_t i = 0; i < us[static_cast<size_t>(r)].size(); ++i) {
            const UnitPlan& u = us[static_cast<size_t>(r)][i];
            CHECK(u.exchange == (i + 1 < us[0].size()));
            if (!u.exchange || !o.overlap) {
              CHECK(u.shells.empty() && u.interior.count() == s.full.count() && u.interior.x0 == s.full.x0);
            } else {
              // shells + interior tile the compute box: inside it, pairwise disjoint, volumes add up
              std::vector<LBox> all = u.shells;
              if (!u.interior.empty()) all.push_back(u.interior);
              i64 vol = 0;
              for (size_t a = 0; a < all.size(); ++a) {
                const LBox& b = all[a];
                vol += b.count();
                CHECK(!b.empty() && b.x0 >= s.full.x0 && b.x1 <= s.full.x1 && b.y0 >= s.full.y0 && b.y1 <= s.full.y1 &&
                      b.z0 >= s.full.z0 && b.z1 <= s.full.z1);
                CHECK(leapfrog_p2_supported(s.lay, b, u.steps));
                for (size_t c = a + 1; c < all.size(); ++c) CHECK(!boxes_meet(b, all[c]));
              }
              CHECK(vol == s.full.count());
              CHECK(!u.shells.empty() && static_cast<int>(u.shells.size()) < kTbSlots);
            }
            if (!u.exchange) {
              CHECK(u.msgs.empty() && u.ghost_bits == 0);
              continue;
            }
            const int w = us[static_cast<size_t>(r)][i + 1].steps;
            CHECK(u.depth == w);
            CHECK(s.block_tb || !o.ghost_store ? u.ghost_bits == 0 : u.ghost_bits == (s.nb[0][0] ? 1 : 0) + (s.nb[0][1] ? 2 : 0));
            const DeepPlan dp = s.block_tb ? make_deep_plan(s.lay, s.dims, r, w) : DeepPlan{};
            CHECK(!u.msgs.empty());
            for (const MsgPlan& m : u.msgs) {
              const UnitPlan& v = us[static_cast<size_t>(m.peer)][i];
              int matches = 0;
              for (const MsgPlan& h : v.msgs)
                if (h.peer == r && h.tag == m.tag) {
                  ++matches;
                  CHECK(h.count == m.count && h.field == m.field);
                }
              CHECK(matches == 1);
              if (s.block_tb) {
                i64 want = -1;
                for (const DeepPeer& q : dp.peers)
                  if (q.peer == m.peer) want = q.count;
                CHECK(m.count == want && m.field == MsgField::kStaging && m.send_off + m.count <= s.send_total &&
                      m.recv_off + m.count <= s.deep_max);
              } else {
                // slab: S' planes of u^{n+S}, S' − 1 − g of u^{n+S−1}; both ends store the same ghost plane or neither
                const int side = m.peer < r ? 0 : 1, g = (u.ghost_bits >> side) & 1;
                CHECK(((v.ghost_bits >> (1 - side)) & 1) == g);
                CHECK(m.count == (m.tag == 0 ? w : w - 1 - g) * s.lay.plane);
                CHECK(m.field == (m.tag == 0 ? MsgField::kOut2 : MsgField::kOut1));
                CHECK(m.send_off >= s.lay.plane_off(0) && m.send_off + m.count <= s.lay.plane_off(s.lay.nx));
                CHECK(m.recv_off >= 0 && m.recv_off + m.count <= s.lay.total &&
                      (m.recv_off + m.count <= s.lay.plane_off(0) || m.recv_off >= s.lay.plane_off(s.lay.nx)));
              }
            }
            check_poison(s, u, w);
          }
        }
      }
  // two-step deep halos: 2 ghost planes of u^{n+2}, 1 of u^{n+1}, all by message
  SolverOptions o;
  o.tb = false;
  o.deep_min_planes = 3;
  for (int r = 0; r < 3; ++r) {
    const RankSchedule s = sched(66, 20, o, r, 3);
    CHECK(s.mode == Mode::kDeep);
    int nx = 0;
    for (const UnitPlan& u : fresh_units(s))
      if (u.exchange) {
        CHECK(u.ghost_bits == 0);
        check_poison(s, u, 2);
        ++nx;
      }
    CHECK(nx == 8);
  }
}

void test_traffic() {
  // slab S = 5, K = 20, N = 512, world 8, an inner rank: three exchanges of 5 planes of u^{n+S} and 4 (ghost_store: 3)
  // of u^{n+S−1} per face (docs/ARCHITECTURE.md: 60.5 → 53.8 MB is the same 27 : 24)
  for (bool gs : {true, false}) {
    SolverOptions o;
    o.ghost_store = gs;
    const RankSchedule s = sched(512, 20, o, 3, 8);
    const std::vector<UnitPlan> u = fresh_units(s);
    CHECK((steps_of(u) == Steps{{1, 4}, {5, 5}, {10, 5}, {15, 5}}));
    const Traffic t = traffic(s, u, false);
    CHECK(t.halo_bytes == 2.0 * (gs ? 24.0 : 27.0) * static_cast<double>(s.lay.plane) * 8.0);
  }
  // one rank: an analytic-start pass writes two levels, a fused pass moves four, a single step three, the init two
  for (bool tb : {true, false}) {
    SolverOptions o;
    o.tb = tb;
    o.check_every = 3;
    const RankSchedule s = sched(64, 20, o);
    const std::vector<UnitPlan> u = fresh_units(s);
    const double nb = 63.0 * 63.0 * 63.0 * 8.0;
    double want = u[0].analytic ? 0.0 : 2.0 * nb;
    for (const UnitPlan& x : u) want += nb * (x.analytic ? 2.0 : x.steps >= 2 ? 4.0 : 3.0);
    const Traffic t = traffic(s, u, !u[0].analytic);
    CHECK(u[0].analytic == tb);
    CHECK(t.field_bytes == want && t.halo_bytes == 0.0);
  }
}

// combine_error_log: three ranks' logs of a K = 4 solve checked at steps 2 and 4 into the global one. Fixed rank order,
// a NaN maximum sticks, the finite flag, unchecked steps left out.
void test_combine_error_log() {
  const int K = 4, N = 5, P = 3;  // (N − 1)³ = 64
  const double nan = std::nan(""), big = 1e16;
  const std::vector<int> checked = {2, 4};
  std::vector<double> xy;
  auto at = [&](int q, int n) { return &xy[static_cast<size_t>((q * (K + 1) + n) * 2)]; };
  // every entry of the unchecked steps 0, 1, 3 holds what must never show: NaN maxima, infinite sums
  auto reset = [&] {
    xy.assign(static_cast<size_t>(P * (K + 1) * 2), 0.0);
    for (int q = 0; q < P; ++q)
      for (int n : {0, 1, 3}) at(q, n)[0] = nan, at(q, n)[1] = INFINITY;
  };
  auto set = [&](int n, const double (&mx)[3], const double (&sum)[3]) {
    for (int q = 0; q < P; ++q) at(q, n)[0] = mx[q], at(q, n)[1] = sum[q];
  };
  // Σe² in rank order: three values whose sum depends on the order, in two arrangements that tell left-to-right from
  // every other order; the maximum held by the last rank (step 2) and by the first (step 4)
  {
    reset();
    set(2, {0.25, 0.5, 0.75}, {big, 1.0, -big});
    set(4, {3.0, 1.0, 2.0}, {big, -big, 1.0});
    const ErrorLog r = combine_error_log(xy.data(), P, K, N, checked);
    CHECK(r.steps == checked && r.max_err.size() == 2 && r.rms_err.size() == 2);
    CHECK(r.max_err[0] == 0.75 && r.max_err[1] == 3.0);
    double s2 = 0.0, s4 = 0.0;
    for (double v : {big, 1.0, -big}) s2 += v;
    for (double v : {big, -big, 1.0}) s4 += v;
    CHECK(s2 == 0.0 && (big + -big) + 1.0 == 1.0);   // (step 2: left to right loses the 1 that first + last keeps)
    CHECK(s4 == 1.0 && big + (-big + 1.0) == 0.0);   // (step 4: left to right keeps the 1 that right to left loses)
    CHECK(r.rms_err[0] == std::sqrt(s2 / 64.0) && r.rms_err[1] == std::sqrt(s4 / 64.0) && r.rms_err[1] == 0.125);
    CHECK(r.finite);
  }
  // a NaN maximum in the middle rank sticks for that step (a larger finite maximum follows it) and clears `finite`;
  // the other step stays finite
  {
    reset();
    set(2, {0.25, nan, 0.75}, {1.0, 2.0, 3.0});
    set(4, {0.5, 0.125, 0.25}, {16.0, 16.0, 32.0});
    const ErrorLog r = combine_error_log(xy.data(), P, K, N, checked);
    CHECK(std::isnan(r.max_err[0]) && !r.finite);
    CHECK(r.rms_err[0] == std::sqrt(6.0 / 64.0));
    CHECK(r.max_err[1] == 0.5 && r.rms_err[1] == 1.0);
    // ... the same log without the NaN is finite; an infinite sum alone is not
    at(1, 2)[0] = 0.5;
    CHECK(combine_error_log(xy.data(), P, K, N, checked).finite);
    at(2, 4)[1] = INFINITY;
    CHECK(!combine_error_log(xy.data(), P, K, N, checked).finite);
  }
  // one source (a one-rank solve, or a rank's own log): the first rank's entries alone; no checked step, an empty log
  {
    reset();
    set(2, {0.25, 9.0, 9.0}, {64.0, 9.0, 9.0});
    const ErrorLog r = combine_error_log(xy.data(), 1, K, N, {2});
    CHECK(r.steps == std::vector<int>{2} && r.max_err[0] == 0.25 && r.rms_err[0] == 1.0 && r.finite);
    const ErrorLog e = combine_error_log(xy.data(), P, K, N, {});
    CHECK(e.steps.empty() && e.max_err.empty() && e.rms_err.empty() && e.finite);
  }
}

// Workgroup counts of every LDS pass launch (pass_grid.hpp) against the partial slot the solver sizes once: an
// over-wide grid — a launch asked for more workgroups than its slot holds — aborts the solve inside the graph capture
// ("bad grid_blocks"). `over` counts the units whose combined shell launch, with only the parent's guard (Σ tiles ≤
// target_blocks), would have exceeded the slot.
void check_box_grid(const PassBoxGrid& g, const LBox& b, int maxlen) {
  if (b.empty()) {
    CHECK(g.blocks() == 0);
    return;
  }
  const i64 nxb = b.x1 - b.x0;
  CHECK(g.nty == ceil_div(b.y1 - b.y0, kTbTile) && g.ntz == ceil_div(b.z1 - b.z0, kTbTile));
  CHECK(g.nxc >= 1 && g.xlen >= 1 && g.xlen <= maxlen);
  CHECK(static_cast<i64>(g.xlen) * g.nxc >= nxb);        // the chunks cover the x range ...
  CHECK(static_cast<i64>(g.xlen) * (g.nxc - 1) < nxb);   // ... and the last one is not empty
}

int check_unit_grids(const RankSchedule& s, const UnitPlan& u, int target) {
  LeapfrogTbTiling t = s.opt.tiling_tb;
  t.target_blocks = target;
  LeapfrogTbTiling tmax = t;
  tmax.stages = s.opt.temporal;
  const int slot = tb_slot_blocks(s.lay, s.full, tmax, s.mode == Mode::kDeepTb);
  CHECK(slot > 0 && (!t.xcd_remap || slot % 8 == 0));
  t.stages = u.steps;
  // one launch per box (GpuSolver::tb_pass): the pair-tiled kernel where it applies, else k_leapfrog_tb (S ≤ 4).
  // (These schedules have no push transport, and no fused pack where tiling.p2 is set.) Either kernel's box checks
  // accept the box with the schedule's stage-real ranges.
  const LBox real = s.mode == Mode::kDeepTb ? s.sreal : tb_default_real();
  auto kernel = [&](const LBox& b) { return pass_kernel(s.lay, b, u.steps, t.p2, u.analytic, false, false); };
  auto one = [&](const LBox& b) {
    if (b.empty()) return;
    CHECK(!throws([&] { pass_box_check(s.lay, b, u.steps, real, "leapfrog_tb", true); }));
    CHECK(!throws([&] { pass_box_check(s.lay, b, u.steps, real, "leapfrog_p2", false); }));
    if (kernel(b) == PassKernel::kP2) {
      const P2LaunchGrid g = p2_launch_grid(&b, 1, t);
      check_box_grid(g.box[0], b, p2_max_xlen(u.steps));
      CHECK(g.box[0].blk0 == 0 && g.nactive == g.box[0].blocks() && g.nblocks >= g.nactive);
      CHECK(g.nblocks <= slot);
    } else {
      CHECK(u.steps <= 4);
      const PassBoxGrid g = tb_box_grid(b, t);
      check_box_grid(g, b, 1 << 30);
      CHECK(pass_round(g.blocks(), t) <= slot);
    }
  };
  one(u.interior);
  for (const LBox& b : u.shells) one(b);
  if (u.shells.size() < 2) return 0;
  // all shells in one launch (GpuSolver::tb_pass_boxes): only where the combined grid fits the slot
  const int n = static_cast<int>(u.shells.size());
  const int used = tb_shells_launch_blocks(s.lay, u.shells.data(), n, t, slot, u.analytic);
  CHECK(used <= slot);
  if (n > kP2MaxBoxes) {
    CHECK(used == 0);
    return 0;
  }
  LeapfrogTbTiling tc = t;
  tc.xcd_remap = false;
  const P2LaunchGrid g = p2_launch_grid(u.shells.data(), n, tc);
  int blk = 0;
  i64 tiles = 0;
  bool p2 = true;
  for (int k = 0; k < n; ++k) {
    const LBox& b = u.shells[static_cast<size_t>(k)];
    p2 = p2 && kernel(b) == PassKernel::kP2;
    check_box_grid(g.box[k], b, p2_max_xlen(u.steps));
    CHECK(g.box[k].blk0 == blk);  // prefix sums
    blk += g.box[k].blocks();
    tiles += g.box[k].tiles();
  }
  CHECK(g.nactive == blk && g.nblocks == blk);
  const bool parent_takes = p2 && tiles <= target;  // the guard before the slot check existed
  CHECK(used == (parent_takes && g.nblocks <= slot ? g.nblocks : 0));
  return parent_takes && g.nblocks > slot ? 1 : 0;
}

int sweep_pass_grids(i64 N, const char* decomp, int world, const std::vector<int>& ranks) {
  int over = 0;
  for (int temporal = 2; temporal <= 5; ++temporal)
    for (int target : {12, 248, 256})
      for (int r : ranks) {
        SolverOptions o;
        o.decomp = decomp;
        o.temporal = temporal;
        const RankSchedule s = sched(N, 20, o, r, world);
        CHECK(world == 1 ? s.mode == Mode::kFusedSingle : s.mode == Mode::kDeepTb);
        // a fresh solve, and one resumed at every level the pass splitter can be entered at: passes of every depth
        // 2..temporal as units and as the depth of the exchange that follows
        // (2-step passes cannot cover an odd number of remaining steps: plan_units refuses those starts)
        std::vector<std::vector<UnitPlan>> plans;
        for (int n0 = 1; n0 <= 7; ++n0) try {
            plans.push_back(n0 == 1 ? fresh_units(s) : plan_units(s, n0, false));
          } catch (const std::exception&) {
          }
        CHECK(plans.size() >= 3);
        for (const std::vector<UnitPlan>& us : plans)
          for (const UnitPlan& u : us)
            if (u.fused()) over += check_unit_grids(s, u, target);
      }
  if (over > 0) std::printf("test_pass_grids: N = %lld %s: %d combined shell launches wider than their slot\n",
                            static_cast<long long>(N), decomp, over);
  return over;
}

void test_pass_grids() {
  CHECK(p2_max_xlen(2) >= 512 && p2_max_xlen(5) >= 512 && p2_max_xlen(5) < p2_max_xlen(2));
  // the hand calculation of an interior rank with 11 × 11 tiles (352² faces, 3×3×3 at N = 1056), S = 5, target 256:
  // x slabs 81 + 81, y rows 66 + 66, z columns 54 + 54 = 402 workgroups against a slot of 384
  {
    SolverOptions o;
    o.decomp = "3x3x3";
    const RankSchedule s = sched(1056, 20, o, 13, 27);
    CHECK(s.mode == Mode::kDeepTb && s.opt.temporal == 5 && s.lay.ny == 352 && s.lay.nz == 352);
    std::vector<LBox> shells;
    LBox interior;
    deep_split(s.full, s.nb, 5, kTbTile, shells, interior);
    CHECK(shells.size() == 6);
    LeapfrogTbTiling t = s.opt.tiling_tb;
    t.stages = 5;
    t.target_blocks = 256;
    const int slot = tb_slot_blocks(s.lay, s.full, t, true);
    CHECK(slot == 384);
    t.xcd_remap = false;
    const P2LaunchGrid g = p2_launch_grid(shells.data(), 6, t);
    int tiles = 0;
    for (int k = 0; k < 6; ++k) tiles += g.box[k].tiles();
    CHECK(tiles == 202 && tiles <= 256);  // the parent's only guard lets the launch through ...
    CHECK(g.nblocks == 402);              // ... which needs more workgroups than the slot holds
    CHECK(tb_shells_launch_blocks(s.lay, shells.data(), 6, t, slot) == 0);  // now: one launch per box
  }
  int over = 0;
  CHECK(sweep_pass_grids(512, "slab", 1, {0}) == 0);
  over += sweep_pass_grids(1056, "3x3x3", 27, {13, 0, 26, 4});
  over += sweep_pass_grids(1152, "3x3x3", 27, {13, 0, 26});
  over += sweep_pass_grids(1536, "4x4x4", 64, {21, 0, 63});
  over += sweep_pass_grids(2048, "2x2x2", 8, {0, 7});
  CHECK(sweep_pass_grids(512, "slab", 2, {0, 1}) == 0);
  CHECK(sweep_pass_grids(512, "slab", 8, {0, 3, 7}) == 0);
  // the small shapes of the GPU tests (tests/test_gpu_rank_pass.py)
  over += sweep_pass_grids(100, "3x3x3", 27, {13});
  over += sweep_pass_grids(67, "2x2x2", 8, {0, 7});
  over += sweep_pass_grids(70, "1x2x3", 6, {4});
  over += sweep_pass_grids(66, "slab", 3, {1});
  CHECK(over > 0);  // (the sweep reaches the regime the slot check exists for)
}

i64& edge(LBox& b, int axis, int side) {
  i64* const e[3][2] = {{&b.x0, &b.x1}, {&b.y0, &b.y1}, {&b.z0, &b.z1}};
  return *e[axis][side];
}
Layout block_layout(i64 N, const Dims& d, int rank, i64 g) {
  Problem pr;
  pr.N = N;
  return make_layout(pr, rank_box(pr, d, rank), 16, g, g, g);
}

// The rule that says which kernel family takes a launch (pass_grid.hpp pass_kernel): every condition flips the answer
// on its own.
void test_pass_kernel() {
  const PassKernel kP2 = PassKernel::kP2, kTb = PassKernel::kTb;
  int odd_ends = 0;
  for (const Layout& l : {block_layout(40, Dims{1, 1, 1}, 0, 1), block_layout(40, Dims{2, 2, 2}, 0, 3),
                          block_layout(40, Dims{2, 2, 2}, 7, 3)}) {
    const LBox full = compute_box(l);
    CHECK(!full.empty() && full.z1 - full.z0 >= 8);
    for (int S = 2; S <= 5; ++S) CHECK(pass_kernel(l, full, S, true, false, false, false) == kP2);
    CHECK(pass_kernel(l, full, 4, false, false, false, false) == kTb);  // tiling.p2 off
    CHECK(pass_kernel(l, full, 4, true, false, true, false) == kTb);    // push transport on
    CHECK(pass_kernel(l, full, 4, true, false, false, true) == kTb);    // fused pack present
    // 16-byte pairs: a box starts on a pair ...
    LBox b = full;
    b.z0 = full.z0 + 1;
    CHECK(pass_kernel(l, b, 4, true, false, false, false) == kTb);
    b.z0 = full.z0 + 2;
    CHECK(pass_kernel(l, b, 4, true, false, false, false) == kP2);
    // ... and ends on a whole one, unless it ends at the rank's last node
    b = full;
    b.z1 = full.z0 + 3;
    CHECK(pass_kernel(l, b, 4, true, false, false, false) == kTb);
    b.z1 = full.z0 + 4;
    CHECK(pass_kernel(l, b, 4, true, false, false, false) == kP2);
    b.z0 = full.z0 + 2 * ((full.z1 - full.z0 - 3) / 2);  // the last 3 (or 4) nodes: half a pair at the end, or none
    b.z1 = full.z1;
    odd_ends += (b.z1 - b.z0) % 2;
    CHECK(pass_kernel(l, b, 4, true, false, false, false) == kP2);
    for (int cut = 0; cut < 2; ++cut) {
      --b.z1;
      CHECK(pass_kernel(l, b, 4, true, false, false, false) == ((b.z1 - b.z0) % 2 == 0 ? kP2 : kTb));
    }
    // the analytic start takes at most 4 steps
    CHECK(pass_kernel(l, full, 4, true, true, false, false) == kP2);
    CHECK(pass_kernel(l, full, 5, true, true, false, false) == kTb);
    CHECK(pass_kernel(l, full, 5, true, false, false, false) == kP2);
    // S = 5 without the pair-tiled kernel: k_leapfrog_tb's launcher, which then refuses the depth
    CHECK(pass_kernel(l, full, 5, false, false, false, false) == kTb);
  }
  CHECK(odd_ends >= 1);
}

// The box checks both launchers share (pass_grid.hpp pass_box_check), on ranks of a 3 × 3 × 3 world at N = 40 with
// 3-deep ghosts: the middle rank, and the two corner ranks at the global boundary.
void test_pass_box_check() {
  const Dims d{3, 3, 3};
  const Layout mid = block_layout(40, d, 13, 3), low = block_layout(40, d, 0, 3), high = block_layout(40, d, 26, 3);
  LBox fmid = compute_box(mid), flow = compute_box(low), fhigh = compute_box(high);
  // stage-real ranges as the schedule sets them: T1 nodes beyond every face with a neighbour
  auto real_of = [&](const Layout& l, int rank, i64 T1) {
    LBox r = compute_box(l);
    for (int a = 0; a < 3; ++a) {
      if (neighbor_rank(d, rank, a, 0) >= 0) edge(r, a, 0) -= T1;
      if (neighbor_rank(d, rank, a, 1) >= 0) edge(r, a, 1) += T1;
    }
    return r;
  };
  // the compute box, one node in from both ends of every axis but `axis`
  auto shrunk = [](const Layout& l, int axis) {
    LBox b = compute_box(l);
    for (int a = 0; a < 3; ++a)
      if (a != axis) ++edge(b, a, 0), --edge(b, a, 1);
    return b;
  };
  auto check = [](const Layout& l, const LBox& b, i64 S, const LBox& real, bool tb) {
    return pass_box_check(l, b, S, real, tb ? "leapfrog_tb" : "leapfrog_p2", tb);
  };
  const char* ax[3] = {"x", "y", "z"};
  // a defaulted real range: x the compute box, y / z the whole allocation
  {
    const LBox r = check(low, shrunk(low, -1), 2, tb_default_real(), true), f = compute_box(low);
    CHECK(r.x0 == f.x0 && r.x1 == f.x1 && r.y0 == -3 && r.y1 == low.ny + 3 && r.z0 == -3 && r.z1 == low.nz + 3);
    const LBox q = check(low, shrunk(low, -1), 2, LBox{1, 0, -2, 5, 1, 0}, false);
    CHECK(q.x0 == f.x0 && q.x1 == f.x1 && q.y0 == -2 && q.y1 == 5);
  }
  for (bool tb : {true, false})
    for (int a = 0; a < 3; ++a) {
      const std::string name = tb ? "leapfrog_tb: " : "leapfrog_p2: ";
      // S = 4 reads 4 nodes beyond the box: deeper than 3 ghosts on either end of the middle rank ...
      for (int side = 0; side < 2; ++side) {
        LBox b = shrunk(mid, -1);
        edge(b, a, side) = edge(fmid, a, side);
        CHECK(throws_with([&] { check(mid, b, 4, real_of(mid, 13, 3), tb); },
                          name + "halo deeper than the ghosts in " + ax[a]));
        CHECK(!throws([&] { check(mid, b, 3, real_of(mid, 13, 3), tb); }));
        // ... but beyond the global boundary nothing is read: the same box of a corner rank, at its boundary end
        const Layout& c = side == 0 ? low : high;
        LBox bc = shrunk(c, -1);
        edge(bc, a, side) = edge(side == 0 ? flow : fhigh, a, side);
        CHECK(!throws([&] { check(c, bc, 4, real_of(c, side == 0 ? 0 : 26, 3), tb); }));
      }
      // a real range beyond the allocation, a stage-1 range that ends at the box: x in both kernels, y / z in
      // k_leapfrog_tb (the pair-tiled pass has no y / z real range and ignores it)
      LBox wide = real_of(mid, 13, 1), narrow = real_of(mid, 13, 2);
      edge(wide, a, 0) = -4;
      edge(narrow, a, 1) = edge(fmid, a, 1);
      if (tb || a == 0) {
        CHECK(throws_with([&] { check(mid, shrunk(mid, -1), 2, wide, tb); },
                          name + "real range outside the allocation in " + ax[a]));
        CHECK(throws_with([&] { check(mid, shrunk(mid, a), 3, narrow, tb); },
                          name + "stage-1 range does not cover the box halo in " + ax[a]));
      } else {
        CHECK(!throws([&] { check(mid, shrunk(mid, -1), 2, wide, tb); }));
        CHECK(!throws([&] { check(mid, shrunk(mid, a), 3, narrow, tb); }));
      }
      CHECK(!throws([&] { check(mid, shrunk(mid, a), 3, real_of(mid, 13, 2), tb); }));
      // a box that leaves the compute box: k_leapfrog_tb only (the pair-tiled pass has its own box rule)
      LBox out = shrunk(mid, -1);
      edge(out, a, 0) = -1;
      if (tb)
        CHECK(throws_with([&] { check(mid, out, 2, real_of(mid, 13, 3), tb); }, "leapfrog_tb box outside the compute box"));
      else
        CHECK(!throws([&] { check(mid, out, 2, real_of(mid, 13, 3), tb); }));
    }
}

}  // namespace

int main() {
  test_split_axis();
  test_decompositions();
  test_layout();
  test_lap7_quadratic();
  test_problem();
  test_pack_unpack();
  test_cpu_solver_golden();
  test_unit_lists();
  test_mode_table();
  test_deep_tb_worlds();
  test_traffic();
  test_combine_error_log();
  test_pass_grids();
  test_pass_kernel();
  test_pass_box_check();
  std::printf("test_core: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
