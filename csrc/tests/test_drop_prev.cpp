// Host-only unit tests of UnitPlan::drop_prev (schedule.hpp): which unit of a solve leaves u^{K−1} out. Only the last
// one, and only a fused pass on the pair-tiled kernel with no exchange, four field buffers, a transport other than push
// and SolverOptions::keep_prev off; every rank of a world decides alike. Built with -fsanitize=address,undefined in
// tests/test_drop_prev_native.py.
#include <cstdio>
#include <string>
#include <vector>

#include "wave3d/pass_grid.hpp"
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

RankSchedule sched(i64 N, int K, const SolverOptions& o, int rank = 0, int world = 1, double free_bytes = 1e13) {
  Problem p;
  p.N = N;
  p.K = K;
  return make_rank_schedule(p, o, rank, world, free_bytes);
}

std::vector<UnitPlan> fresh_units(const RankSchedule& s) {
  const bool analytic = (s.mode == Mode::kFusedSingle || s.mode == Mode::kDeepTb) && s.analytic_ok();
  return plan_units(s, analytic ? 1 : s.opt.init2 && s.prob.K >= 2 ? 2 : 1, analytic);
}

// no unit but the last carries the flag; returns the last one's
bool last_only(const std::vector<UnitPlan>& u) {
  for (size_t i = 0; i + 1 < u.size(); ++i) CHECK(!u[i].drop_prev);
  CHECK(!u.empty());
  return !u.empty() && u.back().drop_prev;
}

void test_one_rank() {
  // K = 20: analytic start of 4, three 5-step passes; the last drops, and nothing does with keep_prev
  for (i64 N : {40, 63, 64, 512}) {
    SolverOptions o;
    const RankSchedule s = sched(N, 20, o);
    const std::vector<UnitPlan> u = fresh_units(s);
    CHECK(s.mode == Mode::kFusedSingle && s.nbuf == 4);
    CHECK(u.size() == 4 && u.back().steps == 5 && !u.back().analytic && !u.back().exchange);
    CHECK(last_only(u));
    o.keep_prev = true;
    CHECK(!last_only(fresh_units(sched(N, 20, o))));
  }
  // K = 5: the analytic start is the whole solve, and the last unit
  {
    SolverOptions o;
    const std::vector<UnitPlan> u = fresh_units(sched(63, 5, o));
    CHECK(u.size() == 1 && u[0].analytic && u[0].steps == 4);
    CHECK(last_only(u));
  }
  // every K: the flag goes with a fused last unit, never with a single step (which writes in place over u^{n−1})
  int singles = 0, fused[6] = {0, 0, 0, 0, 0, 0};
  for (int K = 3; K <= 24; ++K)
    for (int ce : {0, 2, 3}) {
      SolverOptions o;
      o.check_every = ce;
      const RankSchedule s = sched(63, K, o);
      const std::vector<UnitPlan> u = fresh_units(s);
      const bool d = last_only(u);
      CHECK(d == u.back().fused());
      if (u.back().fused())
        ++fused[u.back().steps];
      else
        ++singles;
    }
  CHECK(fused[2] > 0 && fused[3] > 0 && fused[4] > 0 && fused[5] > 0);
  {  // a last unit of one step, whatever the cost table chose above: one step per pass
    SolverOptions o;
    o.temporal = 1;
    const RankSchedule s = sched(63, 8, o);
    const std::vector<UnitPlan> u = fresh_units(s);
    CHECK(u.back().steps == 1 && !last_only(u));
    ++singles;
  }
  CHECK(singles > 0);
  // without the LDS passes (two-step register passes) and in two-buffer mode nothing drops
  {
    SolverOptions o;
    o.tb = false;
    const RankSchedule s = sched(63, 20, o);
    CHECK(s.mode == Mode::kFusedSingle && !last_only(fresh_units(s)));
  }
  {
    SolverOptions o;
    o.tiling_tb.p2 = false;  // (k_leapfrog_tb is left as it is)
    CHECK(!last_only(fresh_units(sched(63, 20, o))));
  }
  {
    SolverOptions o;
    const RankSchedule s = sched(64, 20, o, 0, 1, 2.005e9);  // (four buffers of 65³ doubles and the headroom do not fit)
    CHECK(s.mode == Mode::kSingleStep && s.nbuf == 2);
    CHECK(!last_only(fresh_units(s)));
  }
}

void test_worlds() {
  struct W {
    const char* dec;
    int world;
  };
  for (const W& w : {W{"slab", 2}, W{"slab", 3}, W{"2x1x2", 4}, W{"2x2x2", 8}})
    for (int overlap = 0; overlap < 2; ++overlap)
      for (int keep = 0; keep < 2; ++keep) {
        SolverOptions o;
        o.decomp = w.dec;
        o.overlap = overlap != 0;
        o.keep_prev = keep != 0;
        o.tb_min_planes = 8;
        for (int K : {20, 21}) {
          int ndrop = 0;
          for (int r = 0; r < w.world; ++r) {
            const RankSchedule s = sched(64, K, o, r, w.world);
            CHECK(s.mode == Mode::kDeepTb);
            const std::vector<UnitPlan> u = fresh_units(s);
            CHECK(!u.back().exchange && u.back().shells.empty() && u.back().ghost_bits == 0);
            const bool p2 = pass_kernel(s.lay, s.full, u.back().steps, s.opt.tiling_tb.p2, u.back().analytic, s.push,
                                        s.block_tb && s.opt.fused_pack) == PassKernel::kP2;
            CHECK(last_only(u) == (p2 && !o.keep_prev));
            ndrop += u.back().drop_prev ? 1 : 0;
          }
          CHECK(ndrop == (o.keep_prev ? 0 : w.world));  // (every rank alike)
        }
      }
  // the push transport keeps both levels (its passes are k_leapfrog_tb's)
  for (int r = 0; r < 2; ++r) {
    SolverOptions o;
    o.push = true;
    const RankSchedule s = sched(64, 20, o, r, 2);
    CHECK(s.push && s.mode == Mode::kDeepTb);
    CHECK(!last_only(fresh_units(s)));
  }
  // the copy-engine transport drops as RCCL does, except under poison_ghosts (its end of solve fills ghost regions of
  // what may be the last unit's inputs)
  for (int poison = 0; poison < 2; ++poison)
    for (int r = 0; r < 2; ++r) {
      SolverOptions o;
      o.sdma = true;
      o.poison_ghosts = poison != 0;
      const RankSchedule s = sched(64, 20, o, r, 2);
      CHECK(s.sdma && s.mode == Mode::kDeepTb);
      CHECK(last_only(fresh_units(s)) == (poison == 0));
    }
  // single steps and two-step deep halos on several ranks: no LDS pass, nothing drops
  for (int r = 0; r < 3; ++r) {
    SolverOptions o;
    o.tb = false;
    o.deep_min_planes = 3;
    const RankSchedule s = sched(66, 20, o, r, 3);
    CHECK(s.mode == Mode::kDeep && !last_only(fresh_units(s)));
    SolverOptions o1;
    o1.temporal = 1;
    CHECK(!last_only(fresh_units(sched(66, 20, o1, r, 3))));
  }
}

// traffic() counts the schedule's compulsory bytes: a dropped level is still in it
void test_traffic_unchanged() {
  SolverOptions o;
  const RankSchedule a = sched(64, 20, o);
  o.keep_prev = true;
  const RankSchedule b = sched(64, 20, o);
  const Traffic ta = traffic(a, fresh_units(a), false), tb = traffic(b, fresh_units(b), false);
  CHECK(ta.field_bytes == tb.field_bytes && ta.halo_bytes == tb.halo_bytes);
  CHECK(ta.field_bytes == (2.0 + 3.0 * 4.0) * 63.0 * 63.0 * 63.0 * 8.0);
}

}  // namespace

int main() {
  test_one_rank();
  test_worlds();
  test_traffic_unchanged();
  std::printf("test_drop_prev: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail == 0 ? 0 : 1;
}
