// The solve schedule of one rank, decided on the host from integers alone (no HIP header): what is fixed for the life
// of a solver (make_rank_schedule), the units of one solve with their exchanges (plan_units), the copy-engine links
// (plan_links) and the bytes moved (traffic). GpuSolver (solver.hpp) allocates and launches what they say.
#pragma once

#include <array>
#include <string>
#include <vector>

#include "wave3d/deep_plan.hpp"
#include "wave3d/tiling.hpp"

namespace wave3d {

struct SolverOptions {
  std::string decomp = "slab";  // slab | block | PxQxR
  int check_every = 2;          // error check cadence (reference prints every 2nd step); 0 = only the last step
  bool overlap = true;          // shell/interior split with the halo exchange on a side stream
  bool graph = true;            // capture the whole solve into a hipGraph, replay it on every run()
  bool timers = false;          // per-phase hipEvent timers (adds events to the stream; disables the graph)
  bool debug_sync = false;      // hipDeviceSynchronize after every step (race triage; disables the graph)
  bool poison_ghosts = false;   // NaN-fill ghost layers before each exchange (a missed halo poisons the errors)
  bool fake_comm = false;       // perf study only: run rank `rank` of `world` alone, exchanges replaced by no-ops
  bool fake_traffic = false;    // ... unless set: the exact message set goes to itself over a one-rank communicator
                                // (RCCL copy kernels and bytes next to the passes; the received values are its own)
  LeapfrogTiling tiling;
  // Temporal blocking: up to `temporal` (2..5) steps per HBM pass wherever no halo exchange intervenes. One rank:
  // k_leapfrog_p2 passes (pair-tiled, S ≤ 5; all levels in LDS, error checks at any level), the steps split into
  // passes by measured per-step cost; slab and 3-D block ranks: the same passes with `temporal`-deep ghosts, one
  // exchange per pass (the push transport: k_leapfrog_tb, S ≤ 4; tb = false: two-step k_leapfrog2 passes with 2-deep
  // halos). 1 = one step per pass everywhere.
  int temporal = 5;
  bool tb = true;  // one rank: LDS kernel (false: k_leapfrog2 pairs, only where the intermediate step has no check)
  Leapfrog2Tiling tiling2;
  LeapfrogTbTiling tiling_tb;
  // Start from u¹, u² computed analytically in one write-only pass (k_init_two) instead of u⁰, u¹ + a first step.
  bool init2 = true;
  // Slab ranks use the deep-halo fused schedule only from this many owned x-planes up (below, single steps are faster).
  int deep_min_planes = 96;
  // Slab ranks use the LDS multi-step passes (deep-tb) when every rank owns at least this many x-planes (and at least
  // 2·temporal: each pass first computes the `steps` planes next to each neighbour, the shells that are sent).
  int tb_min_planes = 16;
  // Slab LDS passes (deep-tb) only: the "push" halo transport. Each pass stores the face planes its neighbours read as
  // ghosts a second time, straight into their fine-grained staging over xGMI (TbPush, kernels.hpp): no exchange phase,
  // no RCCL kernels competing for CUs, no shell launches; with `overlap` the pass produces both face regions first so
  // the remote stores drain while it marches on. Cross-rank order: flags in uncached memory, raised at the end of a
  // pass and waited for at the start of the next one (in the kernel; push_cp_wait: by the command processor with
  // hipStreamWaitValue32 — eager launches only, for ranks that share one GPU). Peers are connected with
  // connect_push() (multi-process: IPC handles) or by a GpuGroup.
  bool push = false;
  // Copy-engine ("sdma") transport (deep-tb slab and block ranks): the halo regions are copied into the neighbours'
  // memory (IPC-mapped: their field buffers' ghost planes for slabs, their staging buffers for blocks) by
  // hipMemcpyAsync(..., hipMemcpyDeviceToDeviceNoCU) on copy streams — the SDMA engines move them, no compute unit is
  // taken from the LDS passes — and cross-rank order is kept by flag words in uncached device memory (waits: one-
  // workgroup kernels; "arrived": a 4-byte copy-engine write behind the data). See transport_sdma.cpp for the protocol.
  bool sdma = false;
  // 3-D block LDS passes: the pass stores the z-face message parts of the next exchange straight into the send staging
  // (TbPack, kernels.hpp); the pack kernel then copies only the x / y faces, edges and corners (A/B: --no-fused-pack)
  bool fused_pack = true;
  // slab LDS passes (deep-tb, pair-tiled kernel; RCCL / loopback / copy-engine transports): each pass also stores the
  // u^{n+S−1} plane next to each neighbour face (it computes it anyway), so the exchange sends S planes of u^{n+S} and
  // S − 2 (not S − 1) of u^{n+S−1} per face — 8 instead of 9 planes for a 5-step pass (A/B: --no-ghost-store)
  bool ghost_store = true;
  // false: a solve's last pair-tiled pass stores u^K only (UnitPlan::drop_prev) and u^{K−1} is rebuilt when something
  // first asks for it (GpuSolver: energy(0), download(1), field_hash(1)); true: every pass stores both levels (A/B:
  // --keep-prev)
  bool keep_prev = false;
  // deep-tb with overlap: the shell boxes run on the side stream concurrently with the interior (true), or on s0 before
  // it (false: they get the whole GPU and finish first, so the exchange starts earlier — measured faster with the copy
  // engines at 512³ and 2048³; concurrent helps the small block shells when no transfer follows; env W3D_SHELLS)
  bool shells_concurrent = false;
  // CUs kept free of the passes for RCCL's copy kernels (0: none). The compute stream gets a CU mask without the top
  // `reserve_cus` CUs (KFD deals mask bits to the XCDs round-robin, so a multiple of 8 frees the same number of CUs in
  // every XCD); a pass occupies a whole CU (LDS, VGPRs), so without a reserve RCCL's kernels of an overlapped exchange
  // wait for the pass's last workgroups. The passes' x chunking then targets the remaining CUs. Env W3D_RESERVE_CUS.
  int reserve_cus = 0;
  // copy-engine transport: copy streams (each gets its own SDMA engine; 0 = auto: one per slab face, one for a block
  // rank's messages — in a replayed graph a second copy stream made the 2048³ 2x2x2 rank slower, 48.8 vs 43.6 ms)
  int sdma_streams = 0;
  // copy-engine transport: bound of one in-kernel flag wait in seconds (0 = min(W3D_TIMEOUT_S / 2, 60)); the autotune
  // sets a short one so a candidate whose peer is lost costs seconds, not minutes. It is baked into the captured
  // graphs. Half the host's own wait bound by default, so the device reports the lost peer before the host gives up.
  double flag_timeout_s = 0.0;
  bool push_cp_wait = false;
  // push ranks without an end-of-solve collective (no RCCL communicator): the flag epochs run on over the solves
  // instead of being reset (eager launches: every launch carries its own epochs)
  bool push_no_collective = false;
};

// A solve is an init followed by units; a unit advances one step (in place over u^{n−1}) or 2..5 (a fused pass into
// the two free buffers). Multi-rank units run shell -> exchange -> interior.
enum class Mode { kSingleStep, kFusedSingle, kDeep, kDeepTb };
constexpr int kTbSlots = 8;  // LDS pass launches with error partials per level and unit (shell boxes + interior)

struct RankSchedule {
  Problem prob;
  SolverOptions opt;  // as actually used (temporal, fused_pack and graph may be lowered)
  int rank = 0, world = 1;
  Mode mode = Mode::kSingleStep;
  bool push = false, sdma = false;  // the transport in use (SolverOptions::push / sdma on several ranks)
  bool block_tb = false;            // deep-tb on a 3-D block decomposition (S-deep ghosts on every split axis)
  int nbuf = 2;                     // field buffers: 4 with temporal blocking
  Dims dims;
  Layout lay;
  HaloPlan halo;
  bool nb[3][2] = {};             // neighbour on [axis][side]
  LBox full;                      // the nodes this rank updates
  std::vector<LBox> shell;        // single steps with overlap: one layer next to every neighbour (cpu.hpp shell_split) ...
  LBox interior;                  // ... and the rest
  std::vector<LBox> dshell;       // deep mode: output x-slabs next to neighbours (shell) ...
  LBox dint;                      // ... and the rest (interior)
  i64 sx0 = 0, sx1 = 0;           // deep modes: stage-1 x range (ghost planes recomputed beyond each neighbour face)
  LBox sreal;                     // deep-tb: stage-real ranges per axis (temporal − 1 nodes into each neighbour's ghosts)
  DeepPlan deep[6];               // block_tb: exchange plan before a pass of s steps (index s = 2..temporal)
  i64 deep_max = 0;               // largest staging buffer of those plans (doubles): the receive staging
  i64 sbase[6] = {};              // send staging: the region of depth s starts at sbase[s] (one region per depth)
  i64 send_total = 0;             // ... and its size (doubles)

  // "single-step" | "fused-single" (temporal blocking, one rank) | "deep-tb" (LDS multi-step passes, slab ranks)
  // | "deep-tb-block" (the same on a 3-D block decomposition) | "deep-halo" (two-step passes, slab ranks)
  std::string mode_name() const;
  bool is_check(int n) const { return n >= 1 && ((opt.check_every > 0 && n % opt.check_every == 0) || n == prob.K); }
  bool analytic_ok() const;  // the first unit can be an analytic-start LDS pass
  bool split() const { return opt.overlap && halo.any(); }
  // the unit's NEW field is exchanged after its shell (else: the current field, before the unit)
  bool post_exchange() const { return mode == Mode::kDeep || mode == Mode::kDeepTb || split(); }
  // deep-tb without overlap: no shell launches; each pass runs whole and its faces are exchanged after it. (3-D block
  // passes included: the y/z face shells of S-deep halos would be thin tile strips recomputing most of their tiles)
  bool late_exchange() const { return mode == Mode::kDeepTb && !opt.overlap; }
  bool side_stream() const { return post_exchange() && opt.overlap && !late_exchange() && !push; }
  // the halo overlap that actually runs: the exchange is issued on the side stream while the pass's interior runs
  // (push: the passes produce their face planes first); false for schedules that exchange after the whole pass
  bool overlapped() const { return halo.any() && world > 1 && (push ? opt.overlap : side_stream()); }
};

// Decided from the SMALLEST rank box, so every rank of a world gets the same mode and pass depth. The two-buffer
// in-place scheme replaces temporal blocking when four field buffers do not fit into free_device_bytes.
RankSchedule make_rank_schedule(const Problem& prob, const SolverOptions& opt, int rank, int world,
                                double free_device_bytes);

// One point-to-point message of an exchange; `tag` pairs it with the peer's matching message. Offsets are doubles from
// the start of `field`: a pass's outputs u^{n+S−1} (out1) / u^{n+S} (out2), the field a single step exchanges, or the
// send / receive staging buffers (packed y/z faces, 3-D block messages).
enum class MsgField { kOut1, kOut2, kCurrent, kStaging };
struct MsgPlan {
  int peer, tag;
  MsgField field;
  i64 send_off, recv_off, count;
};

struct UnitPlan {
  int n;      // current level u^n before the unit
  int steps;  // 1: in-place single step; >= 2: one fused pass writing u^{n+steps−1}, u^{n+steps}
  bool analytic = false;  // LDS pass from n = 1 computing u⁰, u¹ in the kernel (no init kernel, no reads)
  bool fused() const { return steps >= 2; }
  bool exchange = false;  // an exchange goes with this unit (RankSchedule::post_exchange: after its shell, else before)
  int depth = 0;          // ... deep-tb: its depth, the next unit's steps
  // ... x sides whose u^{n+S−1} ghost plane the unit's passes store themselves (SolverOptions::ghost_store; bit 0:
  // plane −1, bit 1: plane nx), which the exchange then leaves out. Slab ranks only (a 3-D block rank's edge and corner
  // regions would become L-shaped messages), and only where every pass of the unit runs on the pair-tiled kernel.
  // Every rank computes the same bits for the same exchange, so both ends of a face agree on the message size.
  int ghost_bits = 0;
  // the pass does not store u^{n+steps−1}: the LAST unit of a solve when it is a fused pass on the pair-tiled kernel
  // with no exchange, four field buffers are in use, the transport is not push (nor the copy engines under
  // poison_ghosts, whose end of solve writes into the unit's inputs) and SolverOptions::keep_prev is off.
  // Decided from integers every rank shares, so the ranks of a world agree.
  bool drop_prev = false;
  std::vector<MsgPlan> msgs;
  // deep-tb with overlap: the boxes the neighbours receive, computed first (cpu.hpp deep_split with w = depth), and the
  // rest; otherwise no shells and the whole compute box
  std::vector<LBox> shells;
  LBox interior;
};

// The units of a solve that starts at level start_n (1, 2 or a resumed step); analytic: the first is an analytic start.
// sources: point sources are set (plan_sources) — the last unit then keeps both levels (no drop_prev: the correction is
// added to the stored u^K after the pass, and rebuilding u^{K−1} would run the pass over it again).
// speed: a coefficient field is set (SpeedPlan). One rank's fused-single mode then runs single steps and k_leapfrog2 pairs
// wherever the intermediate step needs no check — the tb = false unit list, whatever `tb` says, because only those
// kernels read a coefficient per node — or single steps only (receivers, sources or a sponge are set too: the cone
// kernels and k_sponge_box recompute with the constant operator). kFused: the pair-tiled passes' coefficient form
// (PassArgs::lamf) — the pass split of a stored start at n = 1 (like set_initial's), no deeper than kP2VarcMaxStages;
// where speed_fused_ok says no (tb off, temporal ≤ 2, several ranks, a box the pair-tiled pass does not take) it is the
// kPairs plan. No unit gets drop_prev.
// Problem::order = 4: single steps only (one rank), whatever the mode, temporal and tb; no unit is analytic or gets drop_prev.
enum class SpeedPlan { kNone = 0, kPairs = 1, kSingles = 2, kFused = 3 };
bool speed_fused_ok(const RankSchedule& s);
std::vector<UnitPlan> plan_units(const RankSchedule& s, int start_n, bool analytic, bool sources = false,
                                 SpeedPlan speed = SpeedPlan::kNone);

// --poison-ghosts where the messages land in the field buffers themselves (every schedule but the 3-D block passes,
// whose receive regions k_box_copy fills): what a unit's exchange NaN-fills. `rows` runs of `count` doubles, `pitch`
// apart, from `off` in `field`.
//   before_pass = false  the receive range of a message, before the exchange that must overwrite it;
//   before_pass = true   the u^{n+S−1} ghost plane the unit's own passes store (ghost_bits; the nodes of the compute
//                        box's y / z range on plane −1 / nx of out1: not the zero slot, the boundary nodes or the row
//                        padding, which no pass writes), on the passes' stream before the unit's first launch — a pass
//                        that stops storing the plane then shows in every solve, not only while the buffer is fresh.
// Together, on a slab unit followed by a pass of w steps: ghost planes [−w, 0) / [nx, nx + w) of u^{n+S} (out2) and
// [−(w − 1), 0) / [nx, nx + w − 1) of u^{n+S−1} (out1), with or without ghost_store.
struct PoisonRange {
  MsgField field;
  i64 off, count, rows, pitch;
  bool before_pass;
};
std::vector<PoisonRange> plan_poison(const RankSchedule& s, const UnitPlan& u);

// Copy-engine transport: link k = one neighbour; slab ranks [lo, hi] (faces that exist), block ranks the peers of
// deep[] in direction order.
struct LinkPlan {
  int peer = -1;
  int side = 0;                  // slab: 0 = lower neighbour, 1 = upper
  int slot = 0;                  // this rank's link index in the PEER's flags
  i64 peer_nx = 0;               // slab: the peer's owned planes
  i64 recv_off[6] = {0, 0, 0, 0, 0, 0};  // block: offset of this rank's message in the peer's staging, per depth
                                         // s = 2..5 (indexed by s, like deep[] and sbase[])
};
std::vector<LinkPlan> plan_links(const RankSchedule& s);

// Bytes one solve moves, from the unit schedule (SURVEY.md §5.5 effective GB/s). field_bytes: the compulsory
// device-memory traffic over the nodes this rank updates — a fused pass reads u^n, u^{n−1} and writes two levels,
// an analytic-start pass only writes its two, a single step reads two and writes one, the init kernel writes two;
// tile-halo re-reads that miss L2 are not in it (rocprof FETCH_SIZE counts those). halo_bytes: what this rank sends
// its neighbours per solve (RCCL / copy-engine messages, or the push transport's forwarded face planes). A level the
// last pass leaves out (UnitPlan::drop_prev) is still counted: the figure describes the schedule, not that saving.
struct Traffic {
  double field_bytes = 0.0, halo_bytes = 0.0;
};
// speed: every unit and the first-step kernel also read the coefficient field once over the compute box.
Traffic traffic(const RankSchedule& s, const std::vector<UnitPlan>& units, bool init_kernel, bool speed = false);

// Receivers: grid nodes whose value u^n is recorded for every n = 0..K. `nodes` holds R global (i, j, k) triples, each
// index in 0..N; slot r of a trace row is node r of the list (a node listed twice fills two slots with the same values).
// plan_receivers returns the ones inside rank_box(p, d, rank), in list order: every node belongs to exactly one rank.
struct Receiver {
  i64 slot;     // index in the global list
  i64 x, y, z;  // local node
  i64 off;      // Layout::off(x, y, z)
};
std::vector<Receiver> plan_receivers(const Problem& p, const Dims& d, int rank, const Layout& l,
                                     const std::vector<std::array<i64, 3>>& nodes);

// Point sources: grid nodes strictly inside the domain at which a forcing term is added after every step. Because the
// leapfrog update is linear, a pass of s steps with forcing = the pass without + the response of a zero field to the
// forcing, which is non-zero only on the L1 ball of radius s − 1 around the node (k_source_cone adds it to the pass's
// two stored levels). plan_sources returns, for one rank, every source of the list whose L1 ball of `radius` meets the
// rank's ALLOCATION (owned box plus ghost layers): a neighbour's source reaches into this rank's ghost planes, which
// this rank corrects itself, so the node may lie outside the allocation (x, y, z and off are signed; off follows
// Layout::off's formula and addresses memory only for nodes inside the allocation). Refused: a node on a global face or
// outside the grid. The table is ordered by COLOUR CLASS, then by list order: classes are a greedy partition of the whole
// list in list order in which two sources share a class only if their L1 distance exceeds 2·radius — their balls are
// disjoint, so one launch per class adds without atomics; every rank computes the same classes, hence adds in the
// same order. class_begin has one entry per class plus the end: class c = table[class_begin[c] .. class_begin[c + 1])
// (possibly empty on this rank).
struct Source {
  i64 slot;     // index in the global list (the column of the addend array a[K][Q])
  i64 x, y, z;  // local node, signed
  i64 off;      // Layout::off's formula at (x, y, z)
};
struct SourcePlan {
  std::vector<Source> table;
  std::vector<int> class_begin;
  int classes() const { return static_cast<int>(class_begin.size()) - 1; }
};
SourcePlan plan_sources(const Problem& p, const Dims& d, int rank, const Layout& l,
                        const std::vector<std::array<i64, 3>>& nodes, int radius);

// The global error log from the ranks' logs. Rank q's entry of step n is the pair xy[(q·(K+1) + n)·2 + {0, 1}] = (max
// |e|, Σe²) over its nodes; per step of `checked`, in fixed rank order: the maximum (a NaN sticks) and Σe² summed left
// to right.
struct ErrorLog {
  std::vector<int> steps;       // checked steps
  std::vector<double> max_err;  // L∞ (global)
  std::vector<double> rms_err;  // sqrt(Σe² / (N−1)³) (global)
  bool finite = true;           // no maximum and no Σe² is NaN or infinite
};
ErrorLog combine_error_log(const double* xy, int nsrc, int K, int N, const std::vector<int>& checked);

}  // namespace wave3d
