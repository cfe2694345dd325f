// GPU solver runtime: one process (rank) per MI355X, RCCL point-to-point halo exchange over xGMI.
//
// Reference call stack being replaced (report.pdf p.15-16 §4.2.4-4.4): MPI_Init → cudaSetDevice →
// host init + H2D → per step {D2H faces → MPI_Sendrecv → H2D; step kernel; BC kernel; error kernel + MPI_Reduce}.
// Here:
//   * fields are initialised on the device (no H2D), both in-place leapfrog levels live in HBM;
//   * per step the boundary SHELL of the local box is updated first, then its faces go to the neighbours with
//     ncclSend/ncclRecv on a side stream while the INTERIOR update runs on the compute stream;
//   * error partials stay on the device; the whole error log crosses to the host once, with one all-gather;
//   * the full K-step solve can be captured into one hipGraph and replayed.
#pragma once

#include <hip/hip_runtime.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "wave3d/decomp.hpp"
#include "wave3d/kernels.hpp"
#include "wave3d/problem.hpp"
#include "wave3d/schedule.hpp"

namespace wave3d {

#define W3D_HIP(expr)                                                                                \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess) ::wave3d::fail(std::string(#expr) + ": " + hipGetErrorString(_e));          \
  } while (0)

// Summed device time per phase of the last run() (SolverOptions::timers). compute = interior / whole-box / fused
// passes; comm overlaps compute when the exchange runs on the side stream; gather is host wall time.
struct PhaseTimes {
  double init_ms = 0, shell_ms = 0, interior_ms = 0, comm_ms = 0, check_ms = 0, gather_ms = 0;
};

// Device time of one schedule unit (SolverOptions::timers; --trace): shell = the boundary part computed first,
// comm = its exchange (side stream, overlapping compute), compute = the rest, check = error reductions.
struct UnitTrace {
  int unit = 0, n = 0, steps = 0;
  double shell_ms = 0, comm_ms = 0, compute_ms = 0, check_ms = 0;
};

struct RunResult : ErrorLog {     // (schedule.hpp: steps, max_err, rms_err, finite)
  double solve_s = 0.0;           // host wall time of run(): field init → last error gathered
  PhaseTimes phases;              // only with SolverOptions::timers
  std::vector<UnitTrace> trace;   // per unit, only with SolverOptions::timers
  bool batched = false;           // run_batch's pipelined path: solve_s is the batch's wall time / n
};

// Thin owner of an RCCL communicator.
class Comm {
 public:
  // 128-byte ncclUniqueId as raw bytes (call on rank 0, ship to the others).
  static std::string make_unique_id();
  Comm(int rank, int world, const std::string& unique_id);
  // every visible device's rank of one communicator, created in this process (ncclCommInitAll over devices
  // 0..world−1): the single-process multi-GPU mode
  static std::vector<std::shared_ptr<Comm>> init_all(int world);
  ~Comm();
  Comm(const Comm&) = delete;
  Comm& operator=(const Comm&) = delete;
  int rank() const { return rank_; }
  int world() const { return world_; }
  // ranks of the communicator as RCCL itself reports them (ncclCommCount): proof of what RCCL saw
  int count() const;
  // device the communicator is bound to (ncclCommCuDevice)
  int device() const;
  void* raw() const { return comm_; }  // ncclComm_t
  // Raise if RCCL reported an asynchronous error.
  void check_async() const;

 private:
  Comm() = default;
  int rank_ = 0, world_ = 1;
  void* comm_ = nullptr;
};

class GpuSolver {
 public:
  // loopback = true: this rank is driven by a GpuGroup (in-process ranks, device-copy halos; tests)
  GpuSolver(const Problem& prob, const SolverOptions& opt, int rank, int world, std::shared_ptr<Comm> comm,
            bool loopback = false);
  ~GpuSolver();
  GpuSolver(const GpuSolver&) = delete;
  GpuSolver& operator=(const GpuSolver&) = delete;

  // One full solve: u⁰, u¹ → K−1 leapfrog steps with error checks → global error log on the host.
  RunResult run();
  // n solves back to back (bench.py's timed block): a solver with a captured graph (one rank, RCCL ranks, fake ranks)
  // enqueues all n replays, each followed by the gather (RCCL ranks: all-gather) and copy of its own error log into
  // its slot of a pinned host buffer, and synchronises once at the end; the CLI then checks every timed solve's log
  // against the warmup solve's. Every solve runs in full. (The host round trip it removes between solves measured
  // within noise of 0 at 512³: profiles/r4/vmcnt/README.md.) Copy-engine, push, timers, resume and no-graph runs call
  // run() n times. solve_s: on the pipelined path the batch's wall time / n (RunResult::batched = true), otherwise
  // each run()'s own time.
  std::vector<RunResult> run_batch(int n);
  // Per-phase event timers for the following run() calls (those launch eagerly; the captured graph is kept for when
  // the timers are switched off again): a phase breakdown of exactly the schedule the graph replays.
  void set_timers(bool on) { sch_.opt.timers = on; }
  // Loaded-field start (resume): every following run() starts at step n0 from u^{n0−1} = prev and
  // u^{n0} = cur (GLOBAL (N+1)³ C-order fields; each rank takes its box and all its ghost layers from them, so the
  // first pass needs no exchange) and continues the same schedule kinds to K, checking the steps after n0. The
  // state is uploaded at the start of each run (eager launches, no graph).
  void set_state(const double* prev_global, const double* cur_global, int n0);
  // User-supplied initial data φ = u(·,0), ψ = u_t(·,0) (GLOBAL (N+1)³ C-order fields, face values ignored; psi_global
  // = nullptr: ψ = 0). Each rank slices them ONCE into device-resident buffers with one ghost layer more than the solve
  // layout; every following run() starts with k_first_step_field (u⁰, u¹ over every owned and ghost node, so the first
  // pass needs no exchange) and runs the ordinary schedule from step 1 — no analytic start, no init2, nothing on the
  // host per solve: the solve is graph-captured and run_batch pipelined exactly where the default solve is. The error
  // log then is the difference from the eigenmode. set_state's preconditions for a start at step 1, with its messages.
  // It and set_state replace each other; either drops the captured graph.
  void set_initial(const double* phi_global, const double* psi_global);
  // Receivers: R global grid nodes (ijk: R triples, each index in 0..N) whose value u^n every following solve records for
  // n = 0..K, on its ordinary schedule. Every rank of a world is given the same list and records the nodes of its own
  // box (plan_receivers). The levels of a fused unit are recomputed from the unit's inputs by k_record_cone, enqueued on
  // s0 at the top of unit_shell (the inputs' ghosts are complete there and nothing writes them before the next unit's
  // pass); stored levels — the start levels, a single-step unit's output — are gathered by k_record_gather. The pass
  // kernels are untouched. With receivers the solve stores both start levels (no analytic start, no init2): rows 0 and
  // 1 are gathered from memory. The trace buffer lives on the device and is NaN-filled at the start of every solve, so
  // a row nothing wrote shows (after set_state at n0: the rows below n0 − 1). Nothing on the host per solve: the solve
  // stays graph-captured and run_batch pipelined. Replaces an earlier list (R = 0: removes it and restores the default
  // start) and drops the captured graph. Refused on the push transport, whose ghosts live in its staging, on fake_comm
  // ranks and on the two-step deep-halo schedule, which only starts from the analytic pair.
  void set_receivers(const i64* ijk, int R);
  // The last solve's (K+1) × owned() values, row n = u^n (run_batch: its last solve's), and the owned receivers' slots
  // in the global list.
  struct Traces {
    std::vector<double> values;
    std::vector<i64> slots;
  };
  Traces traces() const;
  // Point sources: u_tt = Δu + Σ_q w_q(t) δ(x − x_q) at Q global nodes strictly inside the grid (ijk: Q triples; a node
  // listed twice is added twice), w[K][Q] the wavelet samples, row m = w_q(m·τ) (cpu.hpp CpuSolver::set_sources: the
  // definition). The pass kernels are untouched: by linearity a forced pass = the pass + the response of a zero field to
  // its forcing, which k_source_cone (kernels_source.hip) adds to the pass's two stored levels — on s0, for the start
  // right after the start levels are stored (before rows 0 and 1 of the traces are gathered), for unit i at the top of
  // unit_shell(i + 1) (after the last unit: at the end of the solve), the point where the unit's exchange has been joined
  // into s0.
  //   Ghost invariant: exchanged ghost planes always carry UNCORRECTED values — every exchange of unit i's outputs
  //   is complete before the correction of unit i — and every rank then corrects every node of its own allocation that
  //   lies in a source's ball, ghost layers and the ghost_store plane included (plan_sources keeps the sources of the
  //   neighbours whose balls reach in). The addend depends on the source, a and Coeffs only and the colour classes are
  //   computed from the whole list, so a ghost node and its owner's node receive the same addends in the same order
  //   and stay bit-equal. In a GpuGroup, lb_fence(i) puts every rank's s0 behind EVERY rank's pull of unit i (all_pulled),
  //   so no rank corrects a region a peer has yet to read. (A single-step rank without overlap exchanges u^n before
  //   unit n instead: there the owner's corrected value travels, and overwrites the ghost's own correction.)
  // With sources the start stores u⁰, u¹ (no analytic start, no init2) and the last pass keeps both levels (no
  // drop_prev: rebuilding u^{K−1} would run the pass over the corrected u^K). Nothing on the host per solve: the solve
  // stays graph-captured and run_batch pipelined. The error log then has no meaning. Q = 0 removes the sources. Drops
  // the captured graph. Refused (messages start with "sources:"): the push transport, fake_comm ranks, the two-step
  // deep-halo schedule, the copy-engine transport (peers write this rank's ghosts on their own streams: the invariant
  // is not argued for it), ranks of a multi-process world, and set_state together with sources.
  void set_sources(const i64* ijk, int Q, const double* w);
  int sources() const { return n_src_; }
  // Sponge layers (Problem::sponge; cpu.hpp CpuSolver is the definition, the fields match it bit for bit). The LDS pass
  // kernels are untouched: every fused unit runs undamped and is followed, on s0, by k_sponge_box launches that recompute
  // the slabs within reach of the layers (cpu.hpp sponge_boxes) from the unit's inputs with the damped operator and store
  // both levels over the pass's outputs; single-step units run the DAMP instantiations of the single-step kernels. The
  // start levels are stored (no analytic start, no init2) and the last pass keeps both levels (no drop_prev). Nothing on
  // the host per solve: the solve stays graph-captured and run_batch pipelined. The error log then has no meaning.
  // Refused (messages start with "sponge:"): a world larger than 1 of any kind, fake ranks, the push and copy-engine
  // transports, tb = false (k_leapfrog2 pairs), and a receiver or source within W + temporal nodes of a damped face (the
  // cone kernels recompute with the undamped operator, which equals the damped one only outside that reach).
  bool sponge() const { return sch_.prob.sponge.on(); }
  // Problem::order = 4: the fourth-order operator (stencil.hpp d4sum_t; CpuSolver is the definition, the fields, the
  // error log and the traces match it bit for bit). Every unit is a single k_leapfrog4 step whatever temporal and tb say;
  // the start — the eigenmode array or set_initial's φ, ψ — is the first-step-field kernel's fourth-order form; receivers
  // use the single-step gather, sources the single-step add; the solve stays graph-captured. Refused (messages start with
  // "order:"): a world larger than 1 of any kind and group ranks (the halo would be two deep per step), fake ranks, the
  // push and copy-engine transports, a sponge (Problem::validate), set_speed, energy / energy_sums, set_state.
  bool order4() const { return sch_.prob.order == 4; }
  // Problem::time_order = 4 (with order = 4): fourth order in time (stencil.hpp leapfrog_t4; CpuSolver is the definition,
  // matched bit for bit). Every unit is a single step of two launches, k_lap4 (v = τ²L_h u^n into field buffer 2, which
  // an order-4 solve otherwise leaves unused; allocated here where the schedule has two buffers) and k_leapfrog44; the
  // start is launch_first_step_t4. Receivers, the check cadence, graph capture and set_initial work as for order 4;
  // everything order 4 refuses stays refused, and set_sources is refused with a "time_order:" message.
  bool time_order4() const { return sch_.prob.time_order == 4; }
  // Variable wave speed u_tt = c²(x)·Δu (cpu.hpp speed_to_local; CpuSolver is the definition, the fields match it bit for
  // bit). c: a global (N+1)³ field, face values ignored, interior values finite and > 0; courant()·max c ≤ 1 unless
  // `force`; nullptr clears it. lamf = lam·c² is a fifth device buffer in the solve layout, refused when it does not fit
  // into free device memory. A solve with a speed field runs the VARC instantiations: on the default schedule (temporal
  // = 5) the pair-tiled passes' (k_leapfrog_p2, up to kP2VarcMaxStages steps per pass, 40/S bytes per node-step;
  // SpeedPlan::kFused), with temporal ≤ 2, tb = false or a box the pass does not take those of the single-step kernels
  // and of k_leapfrog2_rq — single steps and two-step pairs (the tb = false unit list); single steps only with
  // receivers, sources or a sponge (the cone kernels and k_sponge_box recompute with the constant operator;
  // k_record_gather and the one-step source add are coefficient-free). The start is
  // stored by k_first_step_field<VARC> from step 1 — from set_initial's φ, ψ, else from the eigenmode array kept in
  // init_[0] (no analytic start, no init2); no drop_prev. Everything is on s0, graph-captured, run_batch pipelined.
  // Dropping or setting it drops the captured graph. Refused (messages start with "speed:"): a world larger than 1 of any
  // kind, fake ranks, the push and copy-engine transports, 8 rows per wave (4 with a sponge), set_state, temporal = 3 or 4
  // (a depth of its own; the default 5 runs the deepest built coefficient pass), and energy() — Solver.energy downloads both levels and runs
  // cpu_energy with the mass weight.
  void set_speed(const double* c_global, bool force = false);
  bool speed() const { return lamf_dev_ != nullptr; }
  SpeedRange speed_range() const { return speed_range_; }
  // Discrete energy (cpu.hpp cpu_energy): which = 0: E^{K−1/2} of the retained u^{K−1}, u^K; which = 1: E^{1/2},
  // computed inside the solve right after the first-step kernel (solves started by set_initial) and kept on the
  // device. One rank only. energy_sums: the kinetic and potential sums themselves.
  double energy(int which) const;
  Partial energy_sums(int which) const;

  // Host copy of the local array holding u^K (which = 0) or u^{K−1} (which = 1), full padded layout.
  std::vector<double> download(int which) const;
  // Order-independent 64-bit hash of the OWNED nodes of u^K (which = 0) or u^{K−1} (which = 1) after the last run():
  // Σ mix(bits(u) ^ mix(global node index)) mod 2⁶⁴. Summed over the ranks (mod 2⁶⁴) it is the same for every
  // decomposition and schedule that computes bit-identical fields — the autotune's field check (one read pass).
  unsigned long long field_hash(int which) const;
  int device() const { return dev_; }  // the HIP device this rank's buffers and streams live on

  const Layout& layout() const { return sch_.lay; }
  const Dims& dims() const { return sch_.dims; }
  const HaloPlan& halo() const { return sch_.halo; }
  const Problem& problem() const { return sch_.prob; }
  const SolverOptions& options() const { return sch_.opt; }
  int rank() const { return sch_.rank; }
  int world() const { return sch_.world; }
  std::vector<LBox> shell_boxes() const { return sch_.shell; }
  LBox interior_box() const { return sch_.interior; }
  std::vector<int> check_steps() const;
  size_t device_bytes() const;
  // "single-step" | "fused-single" | "deep-tb" | "deep-tb-block" | "deep-halo" (RankSchedule::mode_name)
  std::string mode() const { return sch_.mode_name(); }
  // push transport: this rank's staging + flag IPC handles (opaque bytes), and connecting to the neighbours from
  // every rank's handles (index = rank); GpuGroup ranks are connected in-process instead
  bool push() const { return sch_.push; }
  std::string push_handles() const;
  void connect_push(const std::vector<std::string>& all);
  void connect_push_self();  // perf study (fake rank): forward into the own staging, wait for the own signals
  // copy-engine transport: this rank's IPC handles (field buffers, staging, flags) + layout facts, and connecting to
  // every neighbour from all ranks' handles (index = rank); a fake rank connects to itself
  bool sdma() const { return sch_.sdma; }
  int copy_streams() const { return static_cast<int>(xcs_.size()); }
  std::string sdma_handles() const;
  void connect_sdma(const std::vector<std::string>& all);
  void connect_sdma_self();
  // the halo overlap that actually runs, whatever options().overlap says (RankSchedule::overlapped)
  bool overlapped() const { return sch_.overlapped(); }
  // halo transport actually in use: "none" (one rank), "rccl", "push", "sdma", "fake" (perf study, no transport)
  std::string transport() const;
  // Bytes the last run() moved (schedule.hpp traffic; units_ is rebuilt at the start of every solve)
  using Traffic = wave3d::Traffic;
  Traffic traffic() const { return wave3d::traffic(sch_, units_, !analytic_ && resume_n_ == 0, speed()); }
  // whether the last solve's passes stored u^{K−1} themselves (false: its last pass left it out, UnitPlan::drop_prev,
  // and the first of energy(0), download(1), field_hash(1) rebuilds it)
  bool stored_prev() const { return units_.empty() || !units_.back().drop_prev; }
  // steps of every unit of the last run()'s plan, in order (1: a single step; ≥ 2: one fused pass)
  std::vector<int> unit_steps() const {
    std::vector<int> v;
    for (const UnitPlan& u : units_) v.push_back(u.steps);
    return v;
  }
  // whether the last solve's first pass computed u⁰, u¹ itself (no init kernel; never with receivers)
  bool analytic_start() const { return analytic_; }

 private:
  friend class GpuGroup;
  void enqueue_solve();  // all device work of one solve on s0/s1 (graph-capturable)
  // One halo exchange on stream st: pack → ncclGroup{ncclSend/ncclRecv per message} → unpack. `pull` != null: this
  // rank belongs to an in-process group driven over a one-rank communicator (GpuGroup "rccl-self"); every message is
  // then moved by a self send/recv pair on THIS rank's communicator, sending the peer's matching face (already packed
  // by the peer) into this rank's receive region — the same RCCL calls, stream and events as the multi-process path.
  void exchange(hipStream_t st, const std::vector<GpuSolver*>* pull = nullptr);
  bool packs() const;               // this schedule's messages go through the staging buffers
  void pack_halo(hipStream_t st);   // faces (single steps) / S-deep regions (block passes) → send_buf_
  void unpack_halo(hipStream_t st); // recv_buf_ → ghost layers
  void gather_errors(RunResult& r);
  void decode_log(const Partial* host, int nsrc, RunResult& r) const;  // per-rank partials → r's log (rank order)
  // The schedule (schedule.hpp) is decided once (sch_) and planned per solve (units_, in phase_init); the unit whose
  // exchange is being issued is units_[cur_unit_]. A message's offsets become pointers where it is used: its field's
  // buffer (uf: the two buffers the unit's pass writes), or the send / receive staging.
  double* msg_buf(MsgField f, bool send, const int uf[2]) const;
  const double* msg_send(const MsgPlan& m) const { return msg_buf(m.field, true, uf_) + m.send_off; }
  double* msg_recv(const MsgPlan& m) const { return msg_buf(m.field, false, uf_) + m.recv_off; }
  // (group ranks) the send region of the peer's message that pairs with m
  const double* peer_send(const MsgPlan& m, const std::vector<GpuSolver*>& ranks) const;
  bool needs_exchange(int i) const { return units_[static_cast<size_t>(i)].exchange; }
  hipStream_t xstream() const { return sch_.side_stream() ? s1_ : s0_; }
  void phase_init();
  void check_stored(int n, const double* buf);  // phase_init: the stored u^n (step 1's check) → the error log
  void unit_shell(int i);
  void unit_exchange_rccl(int i);
  void unit_exchange(int i) { sch_.sdma ? unit_exchange_sdma(i) : unit_exchange_rccl(i); }  // by the transport in use
  void unit_interior(int i);
  // What the LDS pass launches of unit u share: the buffers, the tiling, time factors and check mask of its levels, its
  // slot of partials (counted in tb_slots_ when a level is checked) and the stage-real ranges.
  PassArgs tb_args(const UnitPlan& u);
  // ... the part that needs no slot: buffers (indices into u_), tiling, time factors, stage-real ranges; no check
  PassArgs tb_args_fields(const UnitPlan& u, int prev, int cur, int out1, int out2) const;
  // The last pass of a solve may leave u^{K−1} out (UnitPlan::drop_prev). After every solve (run, each solve of
  // run_batch, a GpuGroup's run; so also the first one after set_state / set_initial) solve_done() notes whether it
  // did; energy(0), download(1) and field_hash(1) then call materialise_prev(), which relaunches that one unit with
  // both outputs (bit-identical: see its definition) and clears the mark.
  void solve_done() { prev_missing_ = !units_.empty() && units_.back().drop_prev; }
  void materialise_prev() const;
  mutable bool prev_missing_ = false;  // u_[prev_buf_] does not hold the last solve's u^{K−1} yet
  int last_in_[2] = {0, 1};            // buffers the last unit read: u^{n−1}, u^n
  // whether unit u's passes pack the z faces of the exchange that follows it (entry u.depth of pk_host_ / pk_dev_)
  bool tb_packs(const UnitPlan& u) const { return pk_dev_ != nullptr && u.exchange && pk_host_[u.depth].w == u.depth; }
  void tb_pass(const UnitPlan& u, const LBox& box, int phase, hipStream_t st = nullptr);  // one k_leapfrog_tb launch
  // the unit's shell boxes in ONE pair-tiled launch when that applies (returns false: launch them one by one)
  bool tb_pass_boxes(const UnitPlan& u, const std::vector<LBox>& boxes, int phase, hipStream_t st);
  // in-process group steps (GpuGroup): pack own faces → (group barrier) → pull peers' faces → (group barrier)
  void lb_pack(int i);
  void lb_pull(int i, const std::vector<GpuSolver*>& ranks, hipEvent_t all_packed);
  void lb_fence(int i, hipEvent_t all_pulled);

  RankSchedule sch_;
  Coeffs coef_;
  int dev_ = 0;
  std::shared_ptr<Comm> comm_;
  bool loopback_ = false;

  double* u_[4] = {nullptr, nullptr, nullptr, nullptr};  // [2], [3] only with temporal blocking
  std::vector<UnitPlan> units_;
  int uf_[2] = {2, 3};            // output buffers of the current fused unit
  BoxCopyTable pack_tab_[6], unpack_tab_[6];  // block_tb: device job tables of sch_.deep[] (send / receive regions)
  TbPack pk_host_[6];                          // fused z-face pack per exchange depth (fused_pack; w = 0: none)
  TbPack* pk_dev_ = nullptr;                   // ... the same five entries in device memory
  std::vector<int> n_dshell_;     // partials per deep shell launch
  int n_dint_ = 0;
  int prev_buf_ = 1;             // buffer index holding u^{K−1} after a solve
  double* d_s_ = nullptr;        // extended sin table (+1 applied when passed to kernels)
  double* send_buf_ = nullptr;   // packed y/z faces
  double* recv_buf_ = nullptr;
  Partial* partials_ = nullptr;
  int n_partials_ = 0;
  Partial* errlog_ = nullptr;    // [K+1]
  Partial* errall_ = nullptr;    // [world][K+1]
  Partial* hbatch_ = nullptr;    // pinned [batch][K+1] (run_batch)
  int hbatch_n_ = 0;
  std::vector<double> ct_;       // cos(a_t n τ)
  hipStream_t s0_ = nullptr, s1_ = nullptr;
  bool own_s0_ = true;  // false: a GpuGroup "push" rank on the group's shared compute stream
  hipEvent_t ev_shell_ = nullptr, ev_halo_ = nullptr, ev_packed_ = nullptr;
  int n_full_ = 0, n_shell_ = 0, n_int_ = 0, n_fused_ = 0;  // error partials of each launch kind
  bool own_v_ = false;                                      // time_order4(): buffer 2 was allocated for v alone
  int n_full4_ = 0;                                         // ... of the fourth-order single step (order4())
  int n_tb_ = 0;                                            // ... per level of a k_leapfrog_tb pass
  // deep-tb: per level, the partials of this unit's launches (shell lo, shell hi, interior) follow each other
  int tb_slots_ = 0;                                        // launches of the current unit with partials so far
  // LDS passes: each unit's partials go to region tb_region_ of kTbRegions; their reductions are queued and issued as
  // one batched launch when the regions wrap and at the end of the solve (one launch instead of one per checked step)
  static constexpr int kTbRegions = 8;
  static constexpr int kTbLevels = 5; // levels per pass (5-step passes: k_leapfrog_p2)
  Partial* tb_partials_ = nullptr;
  int tb_region_ = 0;
  // a level's partials within a region: a unit's launch slots (kTbSlots on multi-rank ranks, else 1) of n_tb_ each
  int tb_level_stride() const { return (sch_.mode == Mode::kDeepTb ? kTbSlots : 1) * n_tb_; }
  Partial* tb_region(int r) const { return tb_partials_ + r * (kTbLevels * tb_level_stride()); }
  size_t tb_bytes_ = 0, send_bytes_ = 0, recv_bytes_ = 0;  // allocated: tb_partials_, send_buf_, recv_buf_
  std::vector<ReduceJob> pending_;
  void flush_reduces();
  int cur_ = 1, old_ = 0;                     // buffer roles during enqueue
  int start_n_ = 1;                           // first leapfrog step after the init kernel
  bool analytic_ = false;                     // the first unit computes u⁰, u¹ itself (no init kernel)
  std::vector<char> is_check_;
  int resume_n_ = 0;                  // > 0: runs start at this step from resume_[0..1]
  std::vector<double> resume_[2];     // local (padded) u^{n0−1}, u^{n0}
  int initial_runs_ = 0;              // solves since set_initial (energy() refuses the fields of an older start)
  bool initial_ = false;              // set_initial: runs start with k_first_step_field on init_[0] = φ, init_[1] = ψ
  Layout init_lay_;                   // ... their layout (the solve layout's box, one ghost layer more)
  double* init_[2] = {nullptr, nullptr};  // device (init_[1] null: ψ = 0)
  bool recording_ = false;            // set_receivers with R > 0 (on every rank of a world, whatever it owns)
  std::vector<Receiver> recv_;        // this rank's receivers; slot = the index in the GLOBAL list ...
  Receiver* recv_dev_ = nullptr;      // ... and in device memory with slot = the column of trace_ (the index in recv_)
  double* trace_ = nullptr;           // device: [K + 1][recv_.size()]
  int n_recv() const { return static_cast<int>(recv_.size()); }
  void record_stored(int n, const double* buf);  // row n from a stored level, on s0
  void record_unit(const UnitPlan& u);           // top of unit_shell: a fused unit's levels from its inputs, on s0
  int n_src_ = 0;                     // set_sources: sources in the global list (on every rank, whatever it keeps)
  SourcePlan src_;                    // the ones whose ball meets this rank's allocation, by colour class
  Source* src_dev_ = nullptr;         // ... in device memory
  double* src_a_ = nullptr;           // device: the scaled addends a[K][n_src_]
  // the correction of the start level (u == nullptr: u¹ in `last`) or of unit u's outputs prev = u^{n+s−1}, last =
  // u^{n+s}, on s0
  void source_correct(const UnitPlan* u, double* prev, double* last);
  void source_finish();  // end of the solve: the last unit's correction
  double* lamf_dev_ = nullptr;        // set_speed: lam·c² in the solve layout (null: constant speed 1)
  SpeedRange speed_range_;
  int temporal_asked_ = 0;            // SolverOptions::temporal as given (sch_.opt.temporal may be lowered)
  bool speed_fused_ = false;          // this solve's units are pair-tiled passes with the coefficient (SpeedPlan::kFused)
  bool speed_eig_ = false;            // init_[0] holds the eigenmode array set_speed put there (no set_initial yet)
  SpeedPlan speed_plan() const {
    return !speed()                                    ? SpeedPlan::kNone
           : (recording_ || n_src_ > 0 || sponge()) ? SpeedPlan::kSingles
           : speed_fused_ok(sch_)                     ? SpeedPlan::kFused
                                                      : SpeedPlan::kPairs;
  }
  double* sponge_dev_ = nullptr;      // sponge layers: the six tables (N + 3 entries each) in device memory ...
  SpongeView sponge_view_;            // ... and their node-0 pointers
  std::vector<LBox> sponge_boxes_[6]; // ... and the slabs a fused unit of s = 2..5 steps recomputes (cpu.hpp sponge_boxes)
  const SpongeView* sponge_arg() const { return sponge() ? &sponge_view_ : nullptr; }
  void sponge_unit(const UnitPlan& u);  // after a fused unit's pass, on s0: the slabs of its two outputs, damped
  // a receiver or a source's ball must stay out of the layers' reach (refusal; `what` names the list)
  void sponge_check_nodes(const i64* ijk, int n, const char* what) const;
  mutable Partial* energy_part_ = nullptr;  // k_energy's partials, then [n] = E^{K−1/2}'s sums, [n + 1] = E^{1/2}'s
  void energy_alloc() const;
  void drop_graphs();
  hipGraphExec_t graph_exec_ = nullptr;
  int runs_ = 0;  // completed run() calls (RCCL ranks capture the graph only after one eager solve)
  int final_buf_ = 0;            // buffer index holding u^K after a solve
  // per-phase timers
  enum { kPhaseInit = 0, kPhaseShell, kPhaseCompute, kPhaseComm, kPhaseCheck, kPhaseGather, kNumPhases };
  struct Mark {
    int phase, unit;  // unit −1: init
    hipEvent_t b, e;
  };
  int cur_unit_ = -1;
  std::vector<hipEvent_t> ev_pool_;
  size_t ev_next_ = 0;
  std::vector<Mark> marks_;
  template <class F>
  void timed(int phase, hipStream_t st, F&& f);
  void collect_phases(RunResult& r);
  // --poison-ghosts: NaN into the ghost regions u's exchange fills (uf: the buffers u's pass writes); before_pass: into
  // the ghost plane u's passes store themselves (UnitPlan::ghost_bits), issued by unit_shell before their launches
  void poison(const UnitPlan& u, const int uf[2], hipStream_t st, bool before_pass = false);
  // push transport (slab deep-tb; transport_push.cpp)
  double* stg_ = nullptr;       // [parity][field (0: u^{n+S−1}, 1: u^{n+S})][side (0: lo ghosts, 1: hi)][T planes]
  unsigned* flags_ = nullptr;   // uncached: [0] raised by the lower neighbour, [1] by the upper, [4] timeout, [8] done
  double* peer_stg_[2] = {nullptr, nullptr};   // neighbours' staging (lo, hi)
  unsigned* peer_flags_[2] = {nullptr, nullptr};
  bool peer_ipc_[2] = {false, false};          // opened with hipIpcOpenMemHandle (closed in the destructor)
  int push_epoch_ = 0;                         // passes of the earlier solves (push_cp_wait: epochs run on)
  TbPush* push_host_ = nullptr;                // per pass of a solve (pinned; [0, K) captured, [K, 2K) eager), ...
  TbPush* push_tab_ = nullptr;                 // ... the half the solve being enqueued uses, uploaded at its start ...
  TbPush* push_dev_ = nullptr;                 // ... to this device table the passes read
  TbPush make_push(int j, int npass) const;    // pass j (1-based) of npass
  mutable unsigned push_uid_ = 0;              // solver instance number (table tags)
  i64 stg_off(int par, int field, int side) const { return ((par * 2 + field) * 2 + side) * sch_.lay.xg * sch_.lay.plane; }
  void connect_push_peer(int side, double* stg, unsigned* flags, bool ipc);
  void push_alloc();                 // constructor: staging, flags, pass tables
  void push_begin_solve();           // s0, start of a solve: reset the signal counter (--poison-ghosts: NaN staging)
  void push_upload();                // s0, once units_ is planned: every pass's TbPush → push_dev_
  void push_pass_args(PassArgs& a);  // the current unit's table entries (and its command-processor waits, on s0)
  void push_finish(hipStream_t st);  // end of a solve: zero this rank's flags (after its last wait)
  void push_check();                 // after a solve: fail if a wait timed out
  // copy-engine transport (transport_sdma.cpp). Link k = one neighbour (schedule.hpp LinkPlan). This rank's flag
  // words: [2k] "arrived" (link k's copies into this rank are complete), [2k + 1] "done" (link k has consumed this
  // rank's previous message and finished the pass that read the regions the next message overwrites).
  struct XLink : LinkPlan {
    unsigned* flags = nullptr;     // the peer's flag words (IPC-mapped, or this rank's own for a fake rank)
    double* u[4] = {nullptr, nullptr, nullptr, nullptr};  // slab: the peer's field buffers
    double* recv = nullptr;        // block: the peer's receive staging
    bool ipc = false;              // mapped with hipIpcOpenMemHandle (closed in the destructor)
  };
  std::vector<XLink> xlinks_;
  unsigned* xflags_ = nullptr;     // uncached: 2 words per link
  int xpar_ = 0;                   // parity of the solve being enqueued (flag values alternate between two sets)
  unsigned long long xsolves_ = 0; // solves enqueued so far (every rank runs the same number)
  hipGraphExec_t xgraph_[2] = {nullptr, nullptr};  // captured solves of either parity
  // copy streams: link k's wait / copies / signal go to xcs_[k % size] (each stream gets its own SDMA engine, measured:
  // 2 streams move 118 GB/s on one GPU where one moves 60), forked from the exchange stream and joined back
  std::vector<hipStream_t> xcs_;
  std::vector<hipEvent_t> xcev_;
  hipEvent_t xfork_ = nullptr;
  // flag values as device words ([parity][i] = xval(i)): the "arrived" signal is a 4-byte copy-engine write queued
  // after the data copies on the same stream, so no compute queue waits for the copies (a signal kernel would, and a
  // hardware queue shared with s0 would hold the interior pass behind it: measured, profiles/r3)
  unsigned* xvals_ = nullptr;
  unsigned xval(int i) const { return (xpar_ ? 0x10000u : 0u) + static_cast<unsigned>(i + 1); }
  unsigned xend(int par) const { return (par ? 0x10000u : 0u) + 0xFFFFu; }
  void sdma_alloc();
  unsigned* xsig(const XLink& l, int word) const { return l.flags + 2 * l.slot + word; }
  void unit_exchange_sdma(int i);  // side stream after unit i's shells (or s0 after the pass): copies + "arrived"
  void sdma_receive(int i);        // s0 before unit i ≥ 1: wait "arrived" (i − 1), unpack, signal "done" (i − 1)
  void sdma_finish();              // s0 after the last unit: "done" for the next solve's first exchange
  unsigned long long flag_ticks() const;     // bound of one in-kernel flag wait (wall-clock ticks)
  // every link has the peer pointers its copies and signals use (connect_sdma / connect_sdma_self / a group): a
  // solver used unconnected would make the copy engines and k_flag_sync write through null + offset (a GPU fault)
  void sdma_check_connected() const;
};

// Per-phase device timers (SolverOptions::timers, eager launches only): every timed launch group is bracketed by two
// events on its stream; after the solve the intervals are summed per phase (and per unit for --trace). Each group is
// also a roctx range ("w3d:<phase>:u<unit>"), so rocprofv3 --marker-trace timelines show the schedule.
template <class F>
void GpuSolver::timed(int phase, hipStream_t st, F&& f) {
  if (!sch_.opt.timers) {
    f();
    return;
  }
  static const char* const kNames[kNumPhases] = {"init", "shell", "compute", "exchange", "check", "gather"};
  char label[48];
  std::snprintf(label, sizeof label, "w3d:%s:u%d", kNames[phase], cur_unit_);
  roctxRangePushA(label);
  auto take = [&]() {
    if (ev_next_ == ev_pool_.size()) {
      hipEvent_t e;
      W3D_HIP(hipEventCreate(&e));
      ev_pool_.push_back(e);
    }
    return ev_pool_[ev_next_++];
  };
  hipEvent_t a = take(), b = take();
  W3D_HIP(hipEventRecord(a, st));
  f();
  W3D_HIP(hipEventRecord(b, st));
  roctxRangePop();
  marks_.push_back({phase, cur_unit_, a, b});
}

}  // namespace wave3d

namespace wave3d {

// P ranks of one decomposition inside ONE process on the current device, halos moved by device-to-device copies.
// Same GpuSolver code as production except the transport; used to validate the multi-rank path on one GPU.
// Transports:
//   "loopback"  : halos by hipMemcpyAsync between the ranks' buffers (no RCCL);
//   "multi-device": rank r on device r (world ≤ visible GPUs), one RCCL communicator over all of them from
//                 ncclCommInitAll, each rank's production solve driven by its own host thread (RCCL needs the ranks'
//                 calls concurrently): real cross-device RCCL / copy-engine traffic without a launcher;
//   "rccl-self" : every rank owns a ONE-rank RCCL communicator (RCCL refuses two ranks of one communicator on one
//                 device, but a one-rank communicator may send to itself) and moves each of its messages with
//                 ncclGroupStart; ncclSend(peer's face, 0); ncclRecv(own ghosts, 0); ncclGroupEnd on its side stream,
//                 the error logs go through ncclAllGather on the same communicators. This executes the production
//                 RCCL calls, their stream placement and event joins on a one-GPU box.
// With options.graph the whole group solve (every rank's streams forked from one group stream) is captured into one
// hipGraph after the first (eager) run and replayed, RCCL kernels included.
class GpuGroup {
 public:
  GpuGroup(const Problem& prob, const SolverOptions& opt, int world, const std::string& transport = "loopback");
  ~GpuGroup();
  GpuGroup(const GpuGroup&) = delete;
  GpuGroup& operator=(const GpuGroup&) = delete;
  RunResult run();  // global error log (rank-ordered combine), solve_s = wall time of the group solve
  GpuSolver& rank(int r) { return *ranks_[static_cast<size_t>(r)]; }
  const Problem& problem() const { return ranks_[0]->problem(); }
  int world() const { return static_cast<int>(ranks_.size()); }
  const std::string& transport() const { return transport_; }
  bool graph_enabled() const { return multi_ ? ranks_[0]->options().graph : graph_; }
  // RCCL communicators in use and the rank count each reports (rccl-self: world one-rank communicators)
  std::vector<int> comm_counts() const;
  void set_state(const double* prev_global, const double* cur_global, int n0);  // every rank (GpuSolver::set_state)
  void set_initial(const double* phi_global, const double* psi_global);         // every rank (GpuSolver::set_initial)
  // every rank (GpuSolver::set_receivers); traces(): the global (K+1) × R array of the last run(), assembled from the
  // ranks' columns
  void set_receivers(const i64* ijk, int R);
  std::vector<double> traces() const;
  // every rank (GpuSolver::set_sources: the loopback and rccl-self groups)
  void set_sources(const i64* ijk, int Q, const double* w);
  int sources() const { return ranks_[0]->sources(); }

 private:
  void enqueue();
  void join();
  void wire_sdma();  // copy-engine ranks: every link's peer pointers
  std::vector<std::unique_ptr<GpuSolver>> ranks_;
  std::string transport_;
  bool graph_ = false;
  bool graph0_ = false;  // graph_ as the constructor decided it (set_initial after a set_state restores it)
  int runs_ = 0;
  hipStream_t gs_ = nullptr;
  hipEvent_t fork_ = nullptr;
  hipEvent_t all_packed_ = nullptr, all_pulled_ = nullptr;  // group barriers on gs_ (see enqueue)
  std::vector<hipEvent_t> join_;
  hipGraphExec_t exec_ = nullptr;
  bool multi_ = false;  // "multi-device": every rank on its own GPU, solved by its own thread
  int n_recv_ = 0;      // receivers in the global list
};

// Host-scalar collectives over the RCCL communicator (timer max-reduction, barriers). Blocking.
double comm_allreduce(const Comm& c, double v, bool max_op);
// Every rank's bytes (equal sizes), in rank order, through ncclAllGather. Blocking.
std::vector<std::string> comm_allgather_bytes(const Comm& c, const std::string& mine);
int rccl_version();  // ncclGetVersion of the RCCL resolved at run time
// Whether this process's HIP runtime captures the multi-rank (multi-stream) schedules correctly (HIP >= 7.2).
bool multistream_capture_safe();
void comm_barrier(const Comm& c);
}  // namespace wave3d
