// The host-side solve schedule. See wave3d/schedule.hpp.
#include "wave3d/schedule.hpp"

#include <algorithm>
#include <cmath>

#include "wave3d/pass_grid.hpp"

namespace wave3d {

namespace {

// 5-step passes exist only in the pair-tiled kernel (k_leapfrog_p2): temporal 5 becomes 4 when that kernel is off
// (tb or tiling_tb.p2 unset), and on several ranks unless they run deep-tb on a transport other than push (whose
// forwarding stores are k_leapfrog_tb's, S ≤ 4). (3-D blocks, overlapped or not, keep 5: the overlapped schedule's
// shell and interior boxes are cut on whole pairs, cpu.hpp deep_split.) These are consequences of pass_kernel
// (pass_grid.hpp), decided here before a layout exists to ask it about.
int clamp_temporal(const SolverOptions& o, int world, bool deep_tb) {
  const bool five = o.tb && o.tiling_tb.p2 && (world == 1 || (deep_tb && !o.push));
  return o.temporal == 5 && !five ? 4 : o.temporal;
}

// Deep-halo fused passes need every unit to be a pair with no error check on its intermediate step, starting from the
// analytic (u¹, u²): K even and no odd check step below K.
bool pairable(const RankSchedule& s) {
  const int K = s.prob.K;
  if (!s.opt.init2 || K < 4 || (K - 2) % 2 != 0) return false;
  for (int n = 3; n < K; n += 2)
    if (s.is_check(n)) return false;
  return true;
}

}  // namespace

std::string RankSchedule::mode_name() const {
  switch (mode) {
    case Mode::kFusedSingle: return "fused-single";
    case Mode::kDeep: return "deep-halo";
    case Mode::kDeepTb: return block_tb ? "deep-tb-block" : "deep-tb";
    default: return "single-step";
  }
}

// (u¹ is the pass's input level: it cannot carry a check)
bool RankSchedule::analytic_ok() const { return opt.tb && opt.init2 && opt.temporal >= 2 && prob.K >= 3 && !is_check(1); }

RankSchedule make_rank_schedule(const Problem& prob, const SolverOptions& opt, int rank, int world,
                                double free_device_bytes) {
  RankSchedule s;
  s.prob = prob;
  s.opt = opt;
  s.rank = rank;
  s.world = world;
  W3D_REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank/world");
  W3D_REQUIRE(!(opt.push && opt.sdma), "push and sdma are two different transports");
  W3D_REQUIRE(opt.temporal >= 1 && opt.temporal <= 5, "temporal must be 1..5");
  s.dims = parse_dims(opt.decomp, world, prob.N);
  const Box box = rank_box(prob, s.dims, rank);
  W3D_REQUIRE(box.nx() >= 1 && box.ny() >= 1 && box.nz() >= 1,
              "decomposition leaves a rank without nodes; use fewer ranks or a larger N");
  // schedule mode: temporal blocking on one rank, or on a 1-D slab decomposition with `temporal`-deep x halos (LDS
  // passes) or 2-deep ones (two-step passes).
  const Dims& d = s.dims;
  const bool slab = d.py == 1 && d.pz == 1;
  s.opt.temporal = clamp_temporal(opt, world, true);  // (the pass depth if this world gets deep-tb)
  if (s.opt.temporal >= 2 && world == 1) s.mode = Mode::kFusedSingle;
  if (s.opt.temporal >= 2 && world > 1) {
    // smallest extent of any rank along each axis (every rank must be able to feed its neighbours' deep halos)
    i64 mn[3] = {box.nx(), box.ny(), box.nz()};
    for (int r = 0; r < world; ++r) {
      const Box b = rank_box(prob, d, r);
      mn[0] = imin(mn[0], b.nx());
      mn[1] = imin(mn[1], b.ny());
      mn[2] = imin(mn[2], b.nz());
    }
    const int rem = prob.K - (s.analytic_ok() ? 1 : 2);  // steps left to the passes (each takes 2..temporal)
    const i64 T2 = 2 * s.opt.temporal;
    // 3-D blocks: S-deep ghosts on every split axis, one exchange (faces, edges, corners) between passes
    const bool block_fits = (d.px == 1 || mn[0] >= imax(T2, 8)) && (d.py == 1 || mn[1] >= imax(T2, 8)) &&
                            (d.pz == 1 || mn[2] >= imax(T2, 8));
    if (opt.tb && opt.init2 && rem >= 2 && (slab ? mn[0] >= imax(opt.tb_min_planes, T2) : block_fits))
      s.mode = Mode::kDeepTb;
    // (two-step passes, measured with --fake-rank on 512³: they win from ~128 local planes up, but at 64 planes the
    // two 2-plane shell passes and the per-chunk stage-1 recompute cost more than the saved traffic)
    else if (slab && mn[0] >= opt.deep_min_planes && mn[0] >= 3 && pairable(s))
      s.mode = Mode::kDeep;
  }
  s.block_tb = s.mode == Mode::kDeepTb && !slab;
  s.opt.temporal = clamp_temporal(opt, world, s.mode == Mode::kDeepTb);
  // (the fused z-face pack lives in k_leapfrog_tb — a launch with a pack never goes to the pair-tiled pass, pass_kernel
  // in pass_grid.hpp — so with that pass asked for, the pack kernel packs the z faces too)
  if (s.block_tb && opt.tiling_tb.p2) s.opt.fused_pack = false;
  if (opt.push && world > 1) {
    W3D_REQUIRE(s.mode == Mode::kDeepTb && !s.block_tb,
                "push transport: slab LDS passes (deep-tb) only, not " + s.mode_name());
    s.push = true;
  }
  for (int attempt = 0; attempt < 2; ++attempt) {
    const i64 T = s.opt.temporal;
    s.lay = make_layout(prob, box, 16, s.mode == Mode::kDeep ? 2 : (s.mode == Mode::kDeepTb && d.px > 1) ? T : 1,
                        s.block_tb && d.py > 1 ? T : 1, s.block_tb && d.pz > 1 ? T : 1);
    // memory plan: temporal blocking needs four field buffers; fall back to the two-buffer in-place scheme when four
    // do not fit next to the other allocations (2049³ fp64 is 68.8 GB per buffer)
    const double need2 = 2.0 * static_cast<double>(s.lay.bytes()), headroom = 2.0e9;
    if (s.mode != Mode::kSingleStep && 2.0 * need2 + headroom > free_device_bytes) {
      W3D_REQUIRE(!s.push, "push transport: four field buffers do not fit");
      s.mode = Mode::kSingleStep;
      s.block_tb = false;
      continue;
    }
    W3D_REQUIRE(need2 + 1.0e8 < free_device_bytes,
                "not enough device memory for two field buffers of " + std::to_string(s.lay.bytes()) + " bytes");
    break;
  }
  s.nbuf = s.mode == Mode::kSingleStep ? 2 : 4;
  if (opt.sdma && world > 1) {
    W3D_REQUIRE(s.mode == Mode::kDeepTb,
                "sdma transport: LDS multi-step passes (deep-tb, slab or block) only, not " + s.mode_name());
    s.sdma = true;
  }
  // (stream memops are not captured into graphs, running epochs are per-launch arguments; timers and the per-step
  // synchronisation need eager launches)
  if ((s.push && (opt.push_cp_wait || opt.push_no_collective)) || opt.timers || opt.debug_sync) s.opt.graph = false;
  s.halo = make_halo_plan(s.lay, d, rank);
  s.full = compute_box(s.lay);

  // interior = compute box minus one layer on every side that has a neighbour; shell = the rest (cpu.hpp shell_split)
  for (int a = 0; a < 3; ++a)
    for (int sd = 0; sd < 2; ++sd) s.nb[a][sd] = neighbor_rank(d, rank, a, sd) >= 0;
  const auto& nb = s.nb;
  const LBox& full = s.full;
  shell_split(full, nb, s.shell, s.interior);

  // deep-halo slab: the 2 owned planes next to each neighbour are the shell (they are what the neighbours receive);
  // stage-1 values are real one ghost plane beyond each neighbour face
  if (s.mode == Mode::kDeep) {
    i64 lo = full.x0, hi = full.x1;
    if (nb[0][0]) {
      const i64 e = imin(full.x0 + 2, full.x1);
      s.dshell.push_back(LBox{full.x0, e, full.y0, full.y1, full.z0, full.z1});
      lo = e;
    }
    if (nb[0][1]) {
      const i64 b = imax(full.x1 - 2, lo);
      if (b < full.x1) s.dshell.push_back(LBox{b, full.x1, full.y0, full.y1, full.z0, full.z1});
      hi = b;
    }
    s.dint = hi > lo ? LBox{lo, hi, full.y0, full.y1, full.z0, full.z1} : LBox{};
    s.sx0 = full.x0 - (nb[0][0] ? 1 : 0);
    s.sx1 = full.x1 + (nb[0][1] ? 1 : 0);
  }
  // deep-tb: stage values are real up to temporal − 1 nodes beyond each neighbour face (recomputed from the
  // temporal-deep halo); the shell/interior split depends on the next pass's depth and is made per unit
  if (s.mode == Mode::kDeepTb) {
    const i64 T1 = s.opt.temporal - 1;
    s.sx0 = full.x0 - (nb[0][0] ? T1 : 0);
    s.sx1 = full.x1 + (nb[0][1] ? T1 : 0);
    s.sreal = LBox{s.sx0, s.sx1, full.y0 - (nb[1][0] ? T1 : 0), full.y1 + (nb[1][1] ? T1 : 0),
                   full.z0 - (nb[2][0] ? T1 : 0), full.z1 + (nb[2][1] ? T1 : 0)};
  }
  // 3-D block passes: one plan per pass depth that can follow an exchange. The send staging holds one region per depth
  // (sbase): the fused z-face pack writes only the real nodes of its message parts and leaves the global-boundary
  // entries at their initial zero, which a region shared with the messages of another depth (whose parts land at other
  // offsets) would overwrite — measured: a depth-3 exchange followed by a depth-4 one sent the depth-3 values of those
  // entries as boundary ghosts
  for (int st = 2; st <= s.opt.temporal && s.block_tb; ++st) {
    s.deep[st] = make_deep_plan(s.lay, d, rank, st);
    s.deep_max = imax(s.deep_max, s.deep[st].total);
    s.sbase[st] = s.send_total;
    s.send_total += round_up(s.deep[st].total, 32);
  }
  return s;
}

namespace {

// Whether the pair-tiled kernel runs the passes of `stages` steps of this rank (pass_kernel, asked about the whole
// compute box: deep_split cuts the overlapped schedule's sub-boxes on whole pairs, so they get the same answer).
bool runs_p2(const RankSchedule& s, int stages, bool analytic) {
  return pass_kernel(s.lay, s.full, stages, s.opt.tiling_tb.p2, analytic, s.push, s.block_tb && s.opt.fused_pack) ==
         PassKernel::kP2;
}

// Split the steps start_n..K into passes of 1..temporal steps minimising the summed cost: µs per step of a pass of s
// steps with every 2nd level checked, measured at 512³ (tools/tune_leapfrog.py --tb); the analytic first pass reads
// nothing but computes u⁰, u¹ (compute-bound). Slab and block ranks (deep-tb) take passes of ≥ 2 steps only: every
// pass writes the two levels the next one reads, so each exchange is one message pair per face.
void plan_passes(const RankSchedule& s, int n, bool analytic, std::vector<UnitPlan>& units, bool varc = false) {
  static const double kStepCostTb[6] = {0.0, 610.0, 437.0, 302.0, 258.0, 1e9};
  // (analytic: φ-stage start, re-measured)
  static const double kAnalyticCostTb[6] = {0.0, 1e9, 346.0, 300.0, 318.0, 1e9};
  // the pair-tiled passes (k_leapfrog_p2, one rank): µs per step at 512³ (profiles/r5/)
  static const double kStepCostP2[6] = {0.0, 610.0, 430.0, 290.0, 225.0, 180.0};
  static const double kAnalyticCostP2[6] = {0.0, 1e9, 300.0, 200.0, 135.0, 1e9};
  // ... with a coefficient field (VARC, 512³, profiles/speed_fused/README.md): the single step 853, the 3-step pass
  // 995–1007 and the 4-step pass 1170 µs per launch; the 2-step pass was not timed at 512³ and stands at the constant
  // pass's 430 times the byte ratio 1.25. No 5-step pass is built.
  static const double kStepCostVarc[6] = {0.0, 853.0, 538.0, 333.0, 292.0, 1e9};
  const bool p2 = runs_p2(s, 2, false);
  const double* kStepCost = varc ? kStepCostVarc : p2 ? kStepCostP2 : kStepCostTb;
  const double* kAnalyticCost = p2 ? kAnalyticCostP2 : kAnalyticCostTb;
  const int K = s.prob.K, rem = K - n, smax = std::min(s.opt.temporal, varc ? kP2VarcMaxStages : 5), smin = s.mode == Mode::kDeepTb ? 2 : 1;
  std::vector<double> best(static_cast<size_t>(rem + 1), 1e300);
  std::vector<int> take(static_cast<size_t>(rem + 1), 1);
  best[0] = 0.0;
  for (int r = 1; r <= rem; ++r)
    for (int st = smin; st <= std::min(smax, r); ++st) {
      const double c = best[static_cast<size_t>(r - st)] + st * kStepCost[st];
      if (c < best[static_cast<size_t>(r)]) {
        best[static_cast<size_t>(r)] = c;
        take[static_cast<size_t>(r)] = st;
      }
    }
  if (analytic) {
    // the analytic first pass takes 2..temporal steps: minimise its cost plus the best split of the rest
    int bf = 2;
    double bc = 1e300;
    for (int f = 2; f <= std::min(smax, rem); ++f) {
      const double c = f * kAnalyticCost[f] + best[static_cast<size_t>(rem - f)];
      if (c < bc) {
        bc = c;
        bf = f;
      }
    }
    units.push_back(UnitPlan{n, bf, true});
    n += bf;
  }
  W3D_REQUIRE(best[static_cast<size_t>(K - n)] < 1e299, "no pass schedule for the remaining steps");
  for (int r = K - n; r > 0; r -= take[static_cast<size_t>(r)]) {
    units.push_back(UnitPlan{n, take[static_cast<size_t>(r)]});
    n += take[static_cast<size_t>(r)];
  }
}

// The messages of unit u's exchange, which a pass of `u.depth` steps follows (deep modes).
void plan_msgs(const RankSchedule& s, UnitPlan& u) {
  const Layout& l = s.lay;
  const i64 P = l.plane, nx = l.nx;
  if (s.block_tb) {
    // one packed message per neighbour (faces, edges, corners): u^{n+S} s deep, then u^{n+S−1} s − 1 deep
    for (const DeepPeer& q : s.deep[u.depth].peers)
      u.msgs.push_back(MsgPlan{q.peer, 0, MsgField::kStaging, s.sbase[u.depth] + q.buf_off, q.buf_off, q.count});
    return;
  }
  for (const Face& f : s.halo.faces) {
    if (s.mode == Mode::kDeepTb || s.mode == Mode::kDeep) {
      // the next pass of w steps reads u^{n+S} (this pass's out2) on w ghost planes and u^{n+S−1} (out1) on w − 1
      // (deep-halo: 2 and 1). ghost_bits: the pass stored u^{n+S−1} on the first ghost plane itself; that part then
      // starts one plane further from the face on both ends: our planes 1..w−2 / nx−w+1..nx−2 into the peer's ghosts
      // at distance 2..w−1
      W3D_REQUIRE(f.axis == 0, "deep-tb and deep-halo modes are slab-only");
      const i64 w = s.mode == Mode::kDeep ? 2 : u.depth, g = (u.ghost_bits >> f.side) & 1, d1 = w - 1 - g;
      const i64 s2 = f.side == 0 ? 0 : nx - w, s1 = f.side == 0 ? g : nx - (w - 1);
      const i64 r2 = f.side == 0 ? -w : nx, r1 = f.side == 0 ? -(w - 1) : nx + g;
      u.msgs.push_back(MsgPlan{f.peer, 0, MsgField::kOut2, l.plane_off(s2), l.plane_off(r2), w * P});
      if (d1 > 0) u.msgs.push_back(MsgPlan{f.peer, 1, MsgField::kOut1, l.plane_off(s1), l.plane_off(r1), d1 * P});
    } else if (f.contiguous) {
      u.msgs.push_back(MsgPlan{f.peer, 0, MsgField::kCurrent, f.send_off, f.recv_off, f.count});
    } else {
      u.msgs.push_back(MsgPlan{f.peer, 0, MsgField::kStaging, f.pack_off, f.pack_off, f.count});
    }
  }
}

}  // namespace

bool speed_fused_ok(const RankSchedule& s) {
  return s.world == 1 && s.mode == Mode::kFusedSingle && s.opt.tb && s.opt.temporal >= 3 && !s.push && !s.sdma &&
         runs_p2(s, 2, false);
}

std::vector<UnitPlan> plan_units(const RankSchedule& s, int start_n, bool analytic, bool sources, SpeedPlan speed) {
  std::vector<UnitPlan> units;
  const int K = s.prob.K;
  int n = start_n;
  const bool varc = speed != SpeedPlan::kNone;
  W3D_REQUIRE(!varc || (s.world == 1 && !analytic), "speed: one rank and a stored start only");
  if (s.prob.order == 4) {
    // the fourth-order operator has single steps only (k_leapfrog4), whatever temporal and tb say: no analytic-start
    // pass, no exchange, no drop_prev
    W3D_REQUIRE(s.world == 1 && !analytic && !varc, "order: one rank, a stored start and no speed field only");
    for (; n <= K - 1; ++n) {
      units.push_back(UnitPlan{n, 1});
      units.back().interior = s.full;
    }
    return units;
  }
  if (speed == SpeedPlan::kFused && !speed_fused_ok(s)) speed = SpeedPlan::kPairs;  // (e.g. a box the pass does not take)
  if (speed == SpeedPlan::kFused) {
    // the split of a stored start by the coefficient passes' own measured costs, no deeper than they are built
    plan_passes(s, n, false, units, true);
  } else if (((s.mode == Mode::kFusedSingle && s.opt.tb) || s.mode == Mode::kDeepTb) && !varc) {
    plan_passes(s, n, analytic, units);
  } else if (s.mode == Mode::kFusedSingle) {
    while (n <= K - 1) {
      const bool f = n + 2 <= K && !s.is_check(n + 1) && speed != SpeedPlan::kSingles;
      units.push_back(UnitPlan{n, f ? 2 : 1});
      n += f ? 2 : 1;
    }
  } else {
    const int st = s.mode == Mode::kDeep ? 2 : 1;
    for (; n <= K - 1; n += st) units.push_back(UnitPlan{n, st});
  }
  const int nu = static_cast<int>(units.size());
  const bool tb = s.mode == Mode::kDeepTb;
  for (int i = 0; i < nu; ++i) {
    UnitPlan& u = units[static_cast<size_t>(i)];
    u.interior = s.full;
    // (push: the passes deliver the ghosts themselves)
    u.exchange = s.halo.any() && !s.push && (s.post_exchange() ? i + 1 < nu : i > 0);
    if (!u.exchange) continue;
    if (tb) u.depth = units[static_cast<size_t>(i) + 1].steps;
    if (tb && s.opt.ghost_store && !s.block_tb && runs_p2(s, u.steps, u.analytic))
      for (const Face& f : s.halo.faces)
        if (f.axis == 0) u.ghost_bits |= 1 << f.side;
    plan_msgs(s, u);
    if (tb && !s.late_exchange()) {
      deep_split(s.full, s.nb, u.depth, kTbTile, u.shells, u.interior);
      W3D_REQUIRE(static_cast<int>(u.shells.size()) < kTbSlots, "deep-tb: too many shell boxes");
    }
  }
  // nothing inside the solve reads the last pass's u^{K−1}: no pass follows, and no exchange sends it. (Not under
  // --poison-ghosts on the copy-engine transport: its end of solve NaN-fills the ghost regions of buffers 2 and 3 for
  // the next solve's first exchange, and those can be the last unit's inputs, which a rebuild reads again.)
  // (Nor with point sources: the source correction is added to the stored u^K after the pass, and a rebuild runs the
  // pass again over it.)
  if (nu > 0 && !sources && !varc && !s.opt.keep_prev && s.nbuf == 4 && !s.push && !(s.sdma && s.opt.poison_ghosts) &&
      ((s.mode == Mode::kFusedSingle && s.opt.tb) || tb)) {
    UnitPlan& u = units.back();
    u.drop_prev = u.fused() && !u.exchange && runs_p2(s, u.steps, u.analytic);
  }
  return units;
}

std::vector<PoisonRange> plan_poison(const RankSchedule& s, const UnitPlan& u) {
  std::vector<PoisonRange> v;
  if (s.block_tb) return v;
  const Layout& l = s.lay;
  for (const MsgPlan& m : u.msgs) v.push_back(PoisonRange{m.field, m.recv_off, m.count, 1, 0, false});
  // the plane plan_msgs left out of the kOut1 message of that side
  for (int side = 0; side < 2; ++side)
    if ((u.ghost_bits >> side) & 1)
      v.push_back(PoisonRange{MsgField::kOut1, l.off(side == 0 ? -1 : l.nx, s.full.y0, s.full.z0), s.full.z1 - s.full.z0,
                              s.full.y1 - s.full.y0, l.pitch, true});
  return v;
}

std::vector<LinkPlan> plan_links(const RankSchedule& s) {
  std::vector<LinkPlan> v;
  if (!s.block_tb) {
    for (int side = 0; side < 2; ++side) {
      const int peer = neighbor_rank(s.dims, s.rank, 0, side);
      if (peer < 0) continue;
      LinkPlan l;
      l.peer = peer;
      l.side = side;
      // the peer's links are [its lower neighbour (if any), its upper]: this rank is the peer's upper neighbour when
      // the peer is below it
      l.slot = side == 0 ? (neighbor_rank(s.dims, peer, 0, 0) >= 0 ? 1 : 0) : 0;
      l.peer_nx = rank_box(s.prob, s.dims, peer).nx();
      v.push_back(l);
    }
    return v;
  }
  for (const DeepPeer& q : s.deep[2].peers) {
    LinkPlan l;
    l.peer = q.peer;
    // the peer's plan (its layout has the same ghost depths): this rank's index among its peers, and where its message
    // lands in the peer's staging for every pass depth
    const Layout pl = make_layout(s.prob, rank_box(s.prob, s.dims, q.peer), 16, s.lay.xg, s.lay.yg, s.lay.zg);
    W3D_REQUIRE(s.opt.temporal < static_cast<int>(sizeof(l.recv_off) / sizeof(l.recv_off[0])),
                "sdma: pass depth beyond the link's offset table");
    for (int st = 2; st <= s.opt.temporal; ++st) {
      const DeepPlan pp = make_deep_plan(pl, s.dims, q.peer, st);
      int idx = -1;
      for (size_t k = 0; k < pp.peers.size(); ++k)
        if (pp.peers[k].peer == s.rank) idx = static_cast<int>(k);
      W3D_REQUIRE(idx >= 0, "sdma: peer plan does not list this rank");
      const DeepPeer& back = pp.peers[static_cast<size_t>(idx)];
      const DeepPeer* mine = nullptr;
      for (const DeepPeer& m : s.deep[st].peers)
        if (m.peer == q.peer) mine = &m;
      W3D_REQUIRE(mine && mine->count == back.count, "sdma: message sizes differ between the two ends of a link");
      l.slot = idx;
      l.recv_off[st] = back.buf_off;
    }
    v.push_back(l);
  }
  return v;
}

Traffic traffic(const RankSchedule& s, const std::vector<UnitPlan>& units, bool init_kernel, bool speed) {
  Traffic t;
  const Layout& l = s.lay;
  const double plane_bytes = static_cast<double>(l.plane) * sizeof(double);
  const double node_bytes = static_cast<double>(l.cx1 - l.cx0) * static_cast<double>(l.cy1 - l.cy0) *
                            static_cast<double>(l.cz1 - l.cz0) * sizeof(double);
  if (init_kernel) t.field_bytes += 2.0 * node_bytes;  // init kernel: u¹, u² (or u⁰, u¹)
  // (a speed field: the first-step kernel and every unit read lamf once)
  if (speed) t.field_bytes += node_bytes * static_cast<double>(units.size() + (init_kernel ? 1 : 0));
  for (const UnitPlan& u : units) {
    t.field_bytes += node_bytes * (u.analytic ? 2.0 : u.fused() ? 4.0 : 3.0);
    // (the stored u^{n+S−1} ghost planes: one plane per face)
    t.field_bytes += static_cast<double>((u.ghost_bits & 1) + (u.ghost_bits >> 1)) * plane_bytes;
    for (const MsgPlan& m : u.msgs) t.halo_bytes += static_cast<double>(m.count) * sizeof(double);
    // sponge layers: a fused unit's slabs are recomputed from its inputs (k_sponge_box) — two levels read on every box
    // grown by the unit's steps and clipped to the interior, two levels written on the box
    if (s.prob.sponge.on() && u.fused())
      for (const LBox& b : sponge_boxes(s.prob, l, u.steps)) {
        const double g = static_cast<double>(imin(b.x1 + u.steps, l.cx1) - imax(b.x0 - u.steps, l.cx0)) *
                         static_cast<double>(imin(b.y1 + u.steps, l.cy1) - imax(b.y0 - u.steps, l.cy0)) *
                         static_cast<double>(imin(b.z1 + u.steps, l.cz1) - imax(b.z0 - u.steps, l.cz0));
        t.field_bytes += 2.0 * (g + static_cast<double>(b.count())) * sizeof(double);
      }
  }
  if (s.push) {  // each pass but the last forwards T planes of u^{n+S} and T − 1 of u^{n+S−1} per face
    const double T = static_cast<double>(l.xg);
    t.halo_bytes = static_cast<double>(s.halo.faces.size()) * (2.0 * T - 1.0) * plane_bytes *
                   static_cast<double>(units.empty() ? 0 : units.size() - 1);
  }
  return t;
}

std::vector<Receiver> plan_receivers(const Problem& p, const Dims& d, int rank, const Layout& l,
                                     const std::vector<std::array<i64, 3>>& nodes) {
  const Box b = rank_box(p, d, rank);
  W3D_REQUIRE(l.gx0 == b.x0 && l.gy0 == b.y0 && l.gz0 == b.z0 && l.nx == b.nx() && l.ny == b.ny() && l.nz == b.nz(),
              "plan_receivers: the layout is not this rank's");
  std::vector<Receiver> v;
  for (size_t r = 0; r < nodes.size(); ++r) {
    const i64 i = nodes[r][0], j = nodes[r][1], k = nodes[r][2];
    W3D_REQUIRE(i >= 0 && i <= p.N && j >= 0 && j <= p.N && k >= 0 && k <= p.N,
                "receiver " + std::to_string(r) + " = (" + std::to_string(i) + ", " + std::to_string(j) + ", " +
                    std::to_string(k) + ") is outside the grid 0.." + std::to_string(p.N));
    if (i < b.x0 || i >= b.x1 || j < b.y0 || j >= b.y1 || k < b.z0 || k >= b.z1) continue;
    const i64 x = i - b.x0, y = j - b.y0, z = k - b.z0;
    v.push_back(Receiver{static_cast<i64>(r), x, y, z, l.off(x, y, z)});
  }
  return v;
}

SourcePlan plan_sources(const Problem& p, const Dims& d, int rank, const Layout& l,
                        const std::vector<std::array<i64, 3>>& nodes, int radius) {
  const Box b = rank_box(p, d, rank);
  W3D_REQUIRE(l.gx0 == b.x0 && l.gy0 == b.y0 && l.gz0 == b.z0 && l.nx == b.nx() && l.ny == b.ny() && l.nz == b.nz(),
              "plan_sources: the layout is not this rank's");
  W3D_REQUIRE(radius >= 0, "plan_sources: negative radius");
  const size_t Q = nodes.size();
  for (size_t q = 0; q < Q; ++q) {
    const i64 i = nodes[q][0], j = nodes[q][1], k = nodes[q][2];
    W3D_REQUIRE(i > 0 && i < p.N && j > 0 && j < p.N && k > 0 && k < p.N,
                "sources: source " + std::to_string(q) + " = (" + std::to_string(i) + ", " + std::to_string(j) + ", " +
                    std::to_string(k) + ") is not strictly inside the grid 1.." + std::to_string(p.N - 1) +
                    " (a node on a global face or outside the grid)");
  }
  // colour classes over the WHOLE list (every rank computes the same ones): greedy in list order, a source joins the
  // first class whose members are all farther than 2·radius from it
  std::vector<int> colour(Q, 0);
  std::vector<std::vector<size_t>> classes;
  auto dist = [&](size_t a, size_t c) {
    i64 s = 0;
    for (int k = 0; k < 3; ++k) s += nodes[a][k] > nodes[c][k] ? nodes[a][k] - nodes[c][k] : nodes[c][k] - nodes[a][k];
    return s;
  };
  for (size_t q = 0; q < Q; ++q) {
    size_t c = 0;
    for (; c < classes.size(); ++c) {
      bool ok = true;
      for (size_t m : classes[c])
        if (dist(q, m) <= 2 * static_cast<i64>(radius)) {
          ok = false;
          break;
        }
      if (ok) break;
    }
    if (c == classes.size()) classes.emplace_back();
    classes[c].push_back(q);
    colour[q] = static_cast<int>(c);
  }
  // this rank's: the L1 ball meets the allocation [−g, n + g) on every axis (the L1 distance from the node to the box)
  SourcePlan out;
  out.class_begin.push_back(0);
  const i64 lo[3] = {-l.xg, -l.yg, -l.zg}, hi[3] = {l.nx + l.xg - 1, l.ny + l.yg - 1, l.nz + l.zg - 1};
  for (const std::vector<size_t>& cl : classes) {
    for (size_t q : cl) {
      const i64 loc[3] = {nodes[q][0] - b.x0, nodes[q][1] - b.y0, nodes[q][2] - b.z0};
      i64 away = 0;
      for (int k = 0; k < 3; ++k) away += loc[k] < lo[k] ? lo[k] - loc[k] : loc[k] > hi[k] ? loc[k] - hi[k] : 0;
      if (away > radius) continue;
      // (off: Layout::off's formula on signed nodes; outside the allocation it addresses nothing and is never used alone)
      out.table.push_back(Source{static_cast<i64>(q), loc[0], loc[1], loc[2], l.off(loc[0], loc[1], loc[2])});
    }
    out.class_begin.push_back(static_cast<int>(out.table.size()));
  }
  return out;
}

ErrorLog combine_error_log(const double* xy, int nsrc, int K, int N, const std::vector<int>& checked) {
  ErrorLog r;
  const size_t per = static_cast<size_t>(K + 1);
  const double n_int = static_cast<double>(N - 1);
  const double denom = n_int * n_int * n_int;
  for (int n : checked) {
    double m = 0.0, sum = 0.0;
    for (int q = 0; q < nsrc; ++q) {  // fixed rank order
      const double* v = xy + (static_cast<size_t>(q) * per + static_cast<size_t>(n)) * 2;
      m = v[0] > m || std::isnan(v[0]) ? v[0] : m;
      sum += v[1];
    }
    r.steps.push_back(n);
    r.max_err.push_back(m);
    r.rms_err.push_back(std::sqrt(sum / denom));
    if (!std::isfinite(m) || !std::isfinite(sum)) r.finite = false;
  }
  return r;
}

}  // namespace wave3d
