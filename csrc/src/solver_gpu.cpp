// GPU solver runtime, the GpuSolver core. See wave3d/solver.hpp. (The communicator: comm.cpp; the push and copy-engine
// transports: transport_push.cpp, transport_sdma.cpp; GpuGroup: gpu_group.cpp.)
#include <algorithm>
#include <cstring>

#include "solver_internal.hpp"
#include "wave3d/capture_guard.hpp"
#include "wave3d/pass_grid.hpp"

namespace wave3d {

// Multi-stream captures with cross-stream event joins repeated per unit (the multi-rank schedules: side-stream
// exchange joined back every pass) crash inside hipStreamEndCapture of the HIP 7.0 runtime that PyTorch-ROCm bundles
// (tools/probes/capture_probe.hip pattern 5, capture_probe2.hip); the system ROCm 7.2 runtime captures them correctly
// (probed, and the rccl-self group graphs). Multi-rank solves are therefore captured only on HIP >= 7.2 (the native
// CLI, which bench.py runs per rank, always is); inside a torch process they run eagerly. W3D_FORCE_CAPTURE=1
// overrides the check.
bool multistream_capture_safe() {
  static const bool ok = [] {
    if (const char* f = std::getenv("W3D_FORCE_CAPTURE"); f && *f == '1') return true;
    int v = 0;
    if (hipRuntimeGetVersion(&v) != hipSuccess) return false;
    return v >= 70200000;
  }();
  return ok;
}

GpuSolver::GpuSolver(const Problem& prob, const SolverOptions& opt, int rank, int world, std::shared_ptr<Comm> comm,
                     bool loopback)
    : coef_(Coeffs::from(prob)), comm_(std::move(comm)), loopback_(loopback) {
  prob.validate();
  W3D_HIP(hipGetDevice(&dev_));
  SolverOptions o = opt;
  // (perf studies: tiling overrides of the LDS S-step kernel; W3D_TB_TARGET=B splits the x march into chunks when the
  // tile grid has fewer than B tiles, W3D_TB_MINCHUNK its minimum planes, W3D_TB_XCDBLOCKS=1 square XCD blocks)
  if (const char* v = std::getenv("W3D_TB_TARGET")) o.tiling_tb.target_blocks = std::atoi(v);
  if (const char* v = std::getenv("W3D_RESERVE_CUS")) o.reserve_cus = std::atoi(v);
  if (const char* v = std::getenv("W3D_TB_MINCHUNK")) o.tiling_tb.min_chunk = std::atoi(v);
  if (const char* v = std::getenv("W3D_TB_XCDBLOCKS")) o.tiling_tb.xcd_blocks = *v == '1';
  if (const char* v = std::getenv("W3D_TB_XCDREMAP")) o.tiling_tb.xcd_remap = *v == '1';  // (A/B runs)
  if (prob.sponge.on()) {  // (sponge layers: solver.hpp sponge())
    W3D_REQUIRE(!o.fake_comm, "sponge: not on a fake rank");
    W3D_REQUIRE(!o.push && !o.sdma, "sponge: not on the push or copy-engine transports");
    W3D_REQUIRE(world == 1 && !loopback_, "sponge: one GPU rank only (no GpuGroup, RCCL ranks, --np or runtime=\"process\": the "
                                          "layers' slabs are recomputed over the whole domain)");
    // (k_leapfrog_rq<8> spills with or without DAMP, the damped one 340-404 B per lane: profiles/sponge/README.md)
    W3D_REQUIRE(!(o.tiling.variant == 1 && o.tiling.rows == 8),
                "sponge: the register-queue single step with 8 rows per wave spills its damped form; use 1, 2 or 4 rows");
    W3D_REQUIRE(o.temporal < 2 || o.tb,
                "sponge: tb = false runs k_leapfrog2 pairs, which have no damped form; use the LDS passes or temporal = 1");
  }
  if (prob.order == 4) {  // (the fourth-order operator: solver.hpp order4())
    W3D_REQUIRE(world == 1 && !loopback_, "order: order = 4 runs on one GPU rank only (no GpuGroup, RCCL ranks, --np or "
                                          "runtime=\"process\": the stencil needs ghosts two deep per step)");
    W3D_REQUIRE(!o.fake_comm, "order: not on a fake rank");
    W3D_REQUIRE(!o.push && !o.sdma, "order: not on the push or copy-engine transports");
  }
  // (the push transport's kernels exist for cubes only: kernels_leapfrog_tb_push.hip)
  W3D_REQUIRE(!(o.push && world > 1 && coef_.box),
              "the push transport has no rectangular-box kernels: run a --box problem over rccl or sdma");
  W3D_REQUIRE(world == 1 || comm_ || loopback_ || o.fake_comm || ((o.push || o.sdma) && o.push_no_collective),
              "world > 1 needs an RCCL communicator (or the loopback group, or the push / sdma transport without one)");
  size_t free_b = 0, total_b = 0;
  W3D_HIP(hipMemGetInfo(&free_b, &total_b));
  sch_ = make_rank_schedule(prob, o, rank, world, static_cast<double>(free_b));
  temporal_asked_ = o.temporal;

  // device memory
  int ncu = 0;
  W3D_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev_));
  auto masked_stream = [&](int first_cu, int last_cu) {  // s0_: a compute stream confined to CUs [first_cu, last_cu)
    std::vector<uint32_t> mask(static_cast<size_t>((ncu + 31) / 32), 0u);
    for (int c = first_cu; c < last_cu; ++c) mask[static_cast<size_t>(c / 32)] |= 1u << (c % 32);
    W3D_HIP(hipExtStreamCreateWithCUMask(&s0_, static_cast<uint32_t>(mask.size()), mask.data()));
  };
  if (const char* cs = std::getenv("W3D_CU_SPLIT"); cs && !loopback_ && (std::strchr(cs, '/') || !std::strcmp(cs, "auto"))) {
    // rehearsal of several ranks on ONE GPU with truly concurrent passes (W3D_CU_SPLIT=r/P, or auto = rank/world):
    // this rank's compute stream only gets the r-th of P disjoint CU ranges, so a pass waiting in the kernel for a
    // peer can never hold the CUs the peer's pass needs
    const bool au = !std::strcmp(cs, "auto");
    const int r = au ? rank : std::atoi(cs), P = au ? world : std::atoi(std::strchr(cs, '/') + 1);
    W3D_REQUIRE(P >= 1 && r >= 0 && r < P && ncu >= P, "W3D_CU_SPLIT must be r/P with 0 <= r < P <= CUs");
    masked_stream(r * ncu / P, (r + 1) * ncu / P);
  } else if (sch_.opt.reserve_cus > 0) {
    W3D_REQUIRE(sch_.opt.reserve_cus < ncu, "reserve_cus must leave the passes at least one CU");
    masked_stream(0, ncu - sch_.opt.reserve_cus);
    if (sch_.opt.tiling_tb.target_blocks == LeapfrogTbTiling{}.target_blocks) sch_.opt.tiling_tb.target_blocks = ncu - sch_.opt.reserve_cus;
  } else {
    W3D_HIP(hipStreamCreateWithFlags(&s0_, hipStreamNonBlocking));
  }
  {
    // the exchange stream gets the highest priority so RCCL's copy kernels are dispatched ahead of the waiting
    // interior workgroups: the halo overlaps the interior update instead of queueing behind it
    int lo = 0, hi = 0;
    W3D_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    W3D_HIP(hipStreamCreateWithPriority(&s1_, hipStreamNonBlocking, hi));
  }
  W3D_HIP(hipEventCreateWithFlags(&ev_shell_, hipEventDisableTiming));
  W3D_HIP(hipEventCreateWithFlags(&ev_halo_, hipEventDisableTiming));
  W3D_HIP(hipEventCreateWithFlags(&ev_packed_, hipEventDisableTiming));
  for (int b = 0; b < sch_.nbuf; ++b) {
    W3D_HIP(hipMalloc(&u_[b], static_cast<size_t>(sch_.lay.bytes())));
    W3D_HIP(hipMemset(u_[b], 0, static_cast<size_t>(sch_.lay.bytes())));
  }
  if (time_order4() && !u_[2]) {  // v = τ²L_h u^n: buffer 2, which a single-step schedule does not allocate itself
    W3D_HIP(hipMalloc(&u_[2], static_cast<size_t>(sch_.lay.bytes())));
    W3D_HIP(hipMemset(u_[2], 0, static_cast<size_t>(sch_.lay.bytes())));
    own_v_ = true;
  }
  if (sch_.push) push_alloc();
  const std::vector<double> s = sin_table_ext(sch_.prob);
  W3D_HIP(hipMalloc(&d_s_, s.size() * sizeof(double)));
  W3D_HIP(hipMemcpy(d_s_, s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice));
  const i64 stage = imax(sch_.halo.packed_doubles, sch_.deep_max);
  if (stage > 0) {
    recv_bytes_ = static_cast<size_t>(stage) * sizeof(double);
    send_bytes_ = static_cast<size_t>(imax(stage, sch_.send_total)) * sizeof(double);
    W3D_HIP(hipMalloc(&send_buf_, send_bytes_));
    W3D_HIP(hipMalloc(&recv_buf_, recv_bytes_));
    W3D_HIP(hipMemset(send_buf_, 0, send_bytes_));
  }
  if (sch_.sdma) sdma_alloc();
  if (sch_.block_tb) {
    // fused z-face pack (its message parts live in send_buf_, zeroed once: nodes on the global boundary are never
    // written — each exchange depth has its own send region, sch_.sbase — and arrive as the zero boundary ghosts)
    const bool fused = sch_.opt.fused_pack && sch_.opt.tb;
    for (int st = 2; st <= sch_.opt.temporal; ++st) {
      pack_tab_[st] = make_box_copy_table(sch_.deep[st], false, fused);
      unpack_tab_[st] = make_box_copy_table(sch_.deep[st], true);
      if (!fused) continue;
      TbPack& k = pk_host_[st];
      k.w = st;
      k.ny = static_cast<int>(sch_.lay.ny);
      k.nz = static_cast<int>(sch_.lay.nz);
      for (const DeepPeer& q : sch_.deep[st].peers)
        if (q.dir[0] == 0 && q.dir[1] == 0)
          for (const DeepPart& part : q.parts) k.zf[q.dir[2] > 0 ? 1 : 0][part.field] = send_buf_ + sch_.sbase[st] + q.buf_off + part.off;
    }
    if (fused) {
      W3D_HIP(hipMalloc(&pk_dev_, sizeof(pk_host_)));
      W3D_HIP(hipMemcpy(pk_dev_, pk_host_, sizeof(pk_host_), hipMemcpyHostToDevice));
    }
  }
  n_full_ = leapfrog_blocks(sch_.lay, &sch_.full, 1, sch_.opt.tiling);
  n_shell_ = leapfrog_blocks(sch_.lay, sch_.shell.data(), static_cast<int>(sch_.shell.size()), sch_.opt.tiling);
  n_int_ = leapfrog_blocks(sch_.lay, &sch_.interior, 1, sch_.opt.tiling);
  n_fused_ = (sch_.mode == Mode::kFusedSingle && !sch_.full.empty()) ? leapfrog2_partials(sch_.lay, sch_.full, sch_.opt.tiling2) : 0;
  if ((sch_.mode == Mode::kFusedSingle || sch_.mode == Mode::kDeepTb) && sch_.opt.tb && !sch_.full.empty()) {
    LeapfrogTbTiling t = sch_.opt.tiling_tb;
    t.stages = sch_.opt.temporal;  // partials per level do not depend on the stage count
    // (multi-rank units also launch sub-boxes of the compute box, shells and interior: pass_grid.hpp)
    n_tb_ = tb_slot_blocks(sch_.lay, sch_.full, t, sch_.mode == Mode::kDeepTb);
    leapfrog_tb_prepare(sch_.push);
  }
  int n_deep = 0;
  for (const LBox& b : sch_.dshell) {
    n_dshell_.push_back(leapfrog2_partials(sch_.lay, b, sch_.opt.tiling2));
    n_deep += n_dshell_.back();
  }
  n_dint_ = sch_.dint.empty() ? 0 : leapfrog2_partials(sch_.lay, sch_.dint, sch_.opt.tiling2);
  n_deep += n_dint_;
  if (order4()) n_full4_ = leapfrog4_blocks(sch_.lay, &sch_.full, 1, sch_.opt.tiling);
  if (time_order4()) n_full4_ = leapfrog44_blocks(sch_.lay, &sch_.full, 1, sch_.opt.tiling);
  n_partials_ = std::max({n_full_, n_full4_, n_shell_ + n_int_, error_blocks(sch_.lay, sch_.full), n_fused_, n_deep,
                          sch_.opt.init2 ? init_two_partials(sch_.lay) : 0, 1});
  W3D_HIP(hipMalloc(&partials_, static_cast<size_t>(n_partials_) * sizeof(Partial)));
  // the LDS passes' partials live apart: their reductions are deferred, so the immediate users of partials_ (init,
  // single steps between passes) must not overwrite them
  tb_bytes_ = static_cast<size_t>(kTbRegions) * kTbLevels * kTbSlots * static_cast<size_t>(n_tb_) * sizeof(Partial);
  if (n_tb_ > 0) W3D_HIP(hipMalloc(&tb_partials_, tb_bytes_));
  W3D_HIP(hipMalloc(&errlog_, static_cast<size_t>(sch_.prob.K + 1) * sizeof(Partial)));
  W3D_HIP(hipMemset(errlog_, 0, static_cast<size_t>(sch_.prob.K + 1) * sizeof(Partial)));
  W3D_HIP(hipMalloc(&errall_, static_cast<size_t>(sch_.world) * (sch_.prob.K + 1) * sizeof(Partial)));
  ct_.resize(static_cast<size_t>(sch_.prob.K + 1));
  for (int n = 0; n <= sch_.prob.K; ++n) ct_[static_cast<size_t>(n)] = time_factor(sch_.prob, n);
  if (loopback_) sch_.opt.graph = false;  // (group ranks: the GpuGroup captures the whole group solve itself)
  if (sch_.prob.sponge.on()) {
    const SpongeTables t = sponge_tables(sch_.prob);
    const size_t n = static_cast<size_t>(sch_.prob.N + 3);
    W3D_HIP(hipMalloc(&sponge_dev_, 6 * n * sizeof(double)));
    for (int a = 0; a < 3; ++a) {
      W3D_HIP(hipMemcpy(sponge_dev_ + a * n, t.g[a].data(), n * sizeof(double), hipMemcpyHostToDevice));
      W3D_HIP(hipMemcpy(sponge_dev_ + (3 + a) * n, t.r[a].data(), n * sizeof(double), hipMemcpyHostToDevice));
    }
    sponge_view_ = SpongeView{sponge_dev_ + 1,         sponge_dev_ + n + 1,     sponge_dev_ + 2 * n + 1,
                              sponge_dev_ + 3 * n + 1, sponge_dev_ + 4 * n + 1, sponge_dev_ + 5 * n + 1};
    sponge_box_prepare();  // (the dynamic-LDS limit: before any capture)
    for (int st = 2; st <= 5; ++st) sponge_boxes_[st] = sponge_boxes(sch_.prob, sch_.lay, st);
  }
  if (order4()) {  // no analytic start: the eigenmode array through the first-step-field path until set_initial replaces it
    init_lay_ = initial_layout(sch_.prob, sch_.lay);
    const std::vector<double> phi0 = eigenmode_local(sch_.prob, init_lay_);
    W3D_HIP(hipMalloc(&init_[0], static_cast<size_t>(init_lay_.bytes())));
    W3D_HIP(hipMemcpy(init_[0], phi0.data(), static_cast<size_t>(init_lay_.bytes()), hipMemcpyHostToDevice));
  }
}

void GpuSolver::set_speed(const double* c, bool force) {
  W3D_REQUIRE(!c || !order4(), "order: no speed field with order = 4 (the coefficient form of the fourth-order operator is "
                               "a follow-up)");
  DeviceScope scope(dev_, true);
  if (!c) {
    if (!speed()) return;
    W3D_HIP(hipDeviceSynchronize());
    drop_graphs();
    W3D_HIP(hipFree(lamf_dev_));
    lamf_dev_ = nullptr;
    speed_range_ = SpeedRange{};
    if (speed_eig_) {
      W3D_HIP(hipFree(init_[0]));
      init_[0] = nullptr;
      speed_eig_ = false;
    }
    return;
  }
  W3D_REQUIRE(sch_.world == 1 && !loopback_, "speed: one GPU rank that spans the domain only (no GpuGroup, RCCL ranks, --np, "
                                             "runtime=\"process\" or multi-device group)");
  W3D_REQUIRE(!sch_.opt.fake_comm, "speed: not on a fake rank");
  W3D_REQUIRE(!sch_.push && !sch_.sdma && !sch_.opt.push && !sch_.opt.sdma, "speed: not on the push or copy-engine transports");
  W3D_REQUIRE(!(sch_.opt.tiling.variant == 1 && sch_.opt.tiling.rows == 8),
              "speed: the register-queue single step with 8 rows per wave has no form with a speed field (it spills "
              "already without one); use 1, 2 or 4 rows");
  W3D_REQUIRE(leapfrog_speed_supported(sch_.opt.tiling, sponge()),
              "speed: with a sponge the register-queue single step is built for 1 or 2 rows per wave only");
  W3D_REQUIRE(resume_n_ == 0, "speed: not together with set_state / --resume");
  W3D_REQUIRE(temporal_asked_ <= 2 || temporal_asked_ == SolverOptions{}.temporal,
              "speed: temporal = " + std::to_string(temporal_asked_) + " asks for a pass depth of its own, which a solve with "
              "a coefficient field does not take; leave temporal at its default (fused passes of up to " +
              std::to_string(kP2VarcMaxStages) + " steps) or use temporal = 1 or 2 (single steps and two-step pairs)");
  std::vector<double> host(static_cast<size_t>(sch_.lay.total));
  const SpeedRange r = speed_to_local(sch_.prob, sch_.lay, c, host.data(), nullptr);
  speed_cfl(sch_.prob, r, force);
  const size_t bytes = static_cast<size_t>(sch_.lay.bytes());
  const Layout il = initial_layout(sch_.prob, sch_.lay);
  if (!lamf_dev_) {  // (the memory planner's view: the fifth field buffer — and the eigenmode array — must fit what is free)
    size_t free_b = 0, total_b = 0;
    W3D_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t need = bytes + (initial_ ? 0u : static_cast<size_t>(il.bytes()));
    W3D_REQUIRE(static_cast<double>(need) <= 0.9 * static_cast<double>(free_b),
                "speed: the coefficient field (" + std::to_string(need >> 20) + " MiB) does not fit into free device memory");
  }
  W3D_HIP(hipDeviceSynchronize());
  drop_graphs();
  if (!lamf_dev_) W3D_HIP(hipMalloc(&lamf_dev_, bytes));
  W3D_HIP(hipMemcpy(lamf_dev_, host.data(), bytes, hipMemcpyHostToDevice));
  speed_range_ = r;
  if (!initial_ && !speed_eig_) {  // no set_initial: the eigenmode array through the first-step-field path
    init_lay_ = il;
    const std::vector<double> phi0 = eigenmode_local(sch_.prob, il);
    W3D_HIP(hipMalloc(&init_[0], static_cast<size_t>(il.bytes())));
    W3D_HIP(hipMemcpy(init_[0], phi0.data(), static_cast<size_t>(il.bytes()), hipMemcpyHostToDevice));
    speed_eig_ = true;
  }
}

void GpuSolver::sponge_check_nodes(const i64* ijk, int n, const char* what) const {
  if (!sponge()) return;
  const Sponge& sp = sch_.prob.sponge;
  const i64 reach = static_cast<i64>(sp.width) + sch_.opt.temporal;
  for (int q = 0; q < n; ++q)
    for (int a = 0; a < 3; ++a)
      for (int side = 0; side < 2; ++side) {
        if (!((sp.faces >> (2 * a + side)) & 1)) continue;
        const i64 d = side == 0 ? ijk[3 * q + a] : sch_.prob.N - ijk[3 * q + a];
        W3D_REQUIRE(d > reach, std::string("sponge: ") + what + " " + std::to_string(q) + " lies " + std::to_string(d) +
                                   " nodes from a damped face, within width + temporal = " + std::to_string(reach) +
                                   " (the cone kernels recompute with the undamped operator)");
      }
}

void GpuSolver::sponge_unit(const UnitPlan& u) {
  if (!sponge() || !u.fused()) return;
  timed(kPhaseCompute, s0_, [&] {
    for (const LBox& b : sponge_boxes_[u.steps])
      launch_sponge_box(sch_.lay, coef_, sponge_view_, u_[old_], u_[cur_], u_[uf_[0]], u_[uf_[1]], b, u.steps, s0_);
  });
}

GpuSolver::~GpuSolver() {
  // a destructor must not throw: release errors are dropped on purpose (the device may already be in an error state)
  if (graph_exec_) (void)hipGraphExecDestroy(graph_exec_);
  for (hipGraphExec_t g : xgraph_)
    if (g) (void)hipGraphExecDestroy(g);
  for (XLink& l : xlinks_)
    if (l.ipc) {
      for (double* p : {l.u[0], l.u[1], l.u[2], l.u[3], l.recv})
        if (p) (void)hipIpcCloseMemHandle(p);
      if (l.flags) (void)hipIpcCloseMemHandle(l.flags);
    }
  if (xflags_) (void)hipFree(xflags_);
  if (xvals_) (void)hipFree(xvals_);
  for (hipStream_t c : xcs_) (void)hipStreamDestroy(c);
  for (hipEvent_t e : xcev_) (void)hipEventDestroy(e);
  if (xfork_) (void)hipEventDestroy(xfork_);
  for (BoxCopyTable& t : pack_tab_) free_box_copy_table(t);
  for (BoxCopyTable& t : unpack_tab_) free_box_copy_table(t);
  if (pk_dev_) (void)hipFree(pk_dev_);
  for (double* p : {u_[0], u_[1], u_[2], u_[3], d_s_, send_buf_, recv_buf_, init_[0], init_[1], sponge_dev_, lamf_dev_})
    if (p) (void)hipFree(p);
  if (energy_part_) (void)hipFree(energy_part_);
  if (recv_dev_) (void)hipFree(recv_dev_);
  if (trace_) (void)hipFree(trace_);
  if (src_dev_) (void)hipFree(src_dev_);
  if (src_a_) (void)hipFree(src_a_);
  if (partials_) (void)hipFree(partials_);
  if (tb_partials_) (void)hipFree(tb_partials_);
  if (errlog_) (void)hipFree(errlog_);
  if (errall_) (void)hipFree(errall_);
  for (hipEvent_t e : ev_pool_) (void)hipEventDestroy(e);
  if (ev_shell_) (void)hipEventDestroy(ev_shell_);
  if (ev_halo_) (void)hipEventDestroy(ev_halo_);
  if (ev_packed_) (void)hipEventDestroy(ev_packed_);
  for (int k = 0; k < 2; ++k)
    if (peer_ipc_[k]) {
      (void)hipIpcCloseMemHandle(peer_stg_[k]);
      (void)hipIpcCloseMemHandle(peer_flags_[k]);
    }
  if (stg_) (void)hipFree(stg_);
  if (push_host_) (void)hipHostFree(push_host_);
  if (hbatch_) (void)hipHostFree(hbatch_);
  if (push_dev_) (void)hipFree(push_dev_);
  if (flags_) (void)hipFree(flags_);
  if (s0_ && own_s0_) (void)hipStreamDestroy(s0_);
  if (s1_) (void)hipStreamDestroy(s1_);
}

size_t GpuSolver::device_bytes() const {
  return static_cast<size_t>(sch_.nbuf + (speed() ? 1 : 0) + (own_v_ ? 1 : 0)) * static_cast<size_t>(sch_.lay.bytes()) +
         recv_bytes_ + send_bytes_ + static_cast<size_t>(n_partials_) * sizeof(Partial) +
         static_cast<size_t>(sch_.prob.N + 3) * sizeof(double) * (sponge() ? 7u : 1u) + tb_bytes_ +
         ((init_[0] ? 1u : 0u) + (init_[1] ? 1u : 0u)) * static_cast<size_t>(init_lay_.bytes()) +
         (energy_part_ ? static_cast<size_t>(energy_partials(sch_.lay) + 2) * sizeof(Partial) : 0u) +
         recv_.size() * (sizeof(Receiver) + static_cast<size_t>(sch_.prob.K + 1) * sizeof(double)) +
         src_.table.size() * sizeof(Source) + (src_a_ ? static_cast<size_t>(sch_.prob.K) * n_src_ * sizeof(double) : 0u);
}

void GpuSolver::drop_graphs() {
  if (graph_exec_) W3D_HIP(hipGraphExecDestroy(graph_exec_));
  graph_exec_ = nullptr;
  for (hipGraphExec_t& g : xgraph_) {
    if (g) W3D_HIP(hipGraphExecDestroy(g));
    g = nullptr;
  }
}

void GpuSolver::energy_alloc() const {
  if (energy_part_) return;
  W3D_HIP(hipMalloc(&energy_part_, static_cast<size_t>(energy_partials(sch_.lay) + 2) * sizeof(Partial)));
}

void GpuSolver::set_initial(const double* phi, const double* psi) {
  W3D_REQUIRE(1 < sch_.prob.K, "resume step must be in [1, K)");
  W3D_REQUIRE(sch_.mode != Mode::kDeepTb || sch_.prob.K - 1 >= 2, "resume: the multi-rank LDS passes need >= 2 steps left");
  W3D_REQUIRE(sch_.mode != Mode::kDeep || (sch_.prob.K - 1) % 2 == 0, "resume: two-step passes need an even step count left");
  DeviceScope scope(dev_, true);
  drop_graphs();
  init_lay_ = initial_layout(sch_.prob, sch_.lay);
  const size_t bytes = static_cast<size_t>(init_lay_.bytes());
  std::vector<double> host(static_cast<size_t>(init_lay_.total));
  for (int k = 0; k < 2; ++k) {
    const double* g = k == 0 ? phi : psi;
    if (!g) {
      if (init_[k]) W3D_HIP(hipFree(init_[k]));
      init_[k] = nullptr;
      continue;
    }
    initial_to_local(init_lay_, g, host.data());
    if (!init_[k]) W3D_HIP(hipMalloc(&init_[k], bytes));
    W3D_HIP(hipMemcpy(init_[k], host.data(), bytes, hipMemcpyHostToDevice));
  }
  if (sch_.world == 1 && !order4()) energy_alloc();
  speed_eig_ = false;  // (init_[0] is the caller's φ now)
  initial_ = true;
  initial_runs_ = 0;
  resume_n_ = 0;
  resume_[0] = std::vector<double>();
  resume_[1] = std::vector<double>();
}

void GpuSolver::set_receivers(const i64* ijk, int R) {
  W3D_REQUIRE(R >= 0 && (R == 0 || ijk != nullptr), "set_receivers: bad receiver list");
  if (R > 0) {
    W3D_REQUIRE(!sch_.push, "receivers: not on the push transport (its ghost planes live in the staging buffers, which "
                            "the record kernel does not read); use rccl or sdma");
    W3D_REQUIRE(!sch_.opt.fake_comm, "receivers: a fake rank's ghosts are never delivered");
    W3D_REQUIRE(sch_.mode != Mode::kDeep, "receivers: the two-step deep-halo passes start from the analytic pair only; "
                                          "use the LDS passes or temporal = 1");
  }
  std::vector<std::array<i64, 3>> nodes(static_cast<size_t>(R));
  for (int r = 0; r < R; ++r) nodes[static_cast<size_t>(r)] = {ijk[3 * r], ijk[3 * r + 1], ijk[3 * r + 2]};
  sponge_check_nodes(ijk, R, "receiver");
  std::vector<Receiver> mine = plan_receivers(sch_.prob, sch_.dims, sch_.rank, sch_.lay, nodes);  // (refuses bad nodes)
  DeviceScope scope(dev_, true);
  drop_graphs();
  if (recv_dev_) W3D_HIP(hipFree(recv_dev_));
  if (trace_) W3D_HIP(hipFree(trace_));
  recv_dev_ = nullptr;
  trace_ = nullptr;
  recv_ = std::move(mine);
  recording_ = R > 0;
  if (recv_.empty()) return;
  std::vector<Receiver> cols = recv_;
  for (size_t k = 0; k < cols.size(); ++k) cols[k].slot = static_cast<i64>(k);
  const size_t tbytes = static_cast<size_t>(sch_.prob.K + 1) * recv_.size() * sizeof(double);
  W3D_HIP(hipMalloc(&recv_dev_, cols.size() * sizeof(Receiver)));
  W3D_HIP(hipMemcpy(recv_dev_, cols.data(), cols.size() * sizeof(Receiver), hipMemcpyHostToDevice));
  W3D_HIP(hipMalloc(&trace_, tbytes));
  W3D_HIP(hipMemset(trace_, 0xFF, tbytes));  // (NaN until a solve writes it)
}

GpuSolver::Traces GpuSolver::traces() const {
  W3D_REQUIRE(recording_, "traces: no receivers are set (set_receivers)");
  Traces t;
  for (const Receiver& r : recv_) t.slots.push_back(r.slot);
  t.values.resize(static_cast<size_t>(sch_.prob.K + 1) * recv_.size());
  if (recv_.empty()) return t;
  DeviceScope scope(dev_, true);
  W3D_HIP(hipMemcpy(t.values.data(), trace_, t.values.size() * sizeof(double), hipMemcpyDeviceToHost));
  return t;
}

void GpuSolver::record_stored(int n, const double* buf) {
  if (recv_.empty()) return;
  launch_record_gather(buf, n, recv_dev_, n_recv(), trace_, n_recv(), s0_);
}

void GpuSolver::record_unit(const UnitPlan& u) {
  if (recv_.empty() || !u.fused()) return;
  launch_record_cone(sch_.lay, coef_, u_[old_], u_[cur_], u.n, u.steps, recv_dev_, n_recv(), trace_, n_recv(), s0_);
}

void GpuSolver::set_sources(const i64* ijk, int Q, const double* w) {
  if (Q > 0) {
    W3D_REQUIRE(!time_order4(), "time_order: no point sources with time_order = 4 (the forcing's tau^4 terms are a "
                                "follow-up)");
    W3D_REQUIRE(!sch_.push, "sources: not on the push transport (its ghost planes live in the staging buffers, which the "
                            "source kernel does not correct); use a loopback or rccl-self group");
    W3D_REQUIRE(!sch_.opt.fake_comm, "sources: a fake rank's ghosts are never delivered");
    W3D_REQUIRE(sch_.mode != Mode::kDeep, "sources: the two-step deep-halo passes start from the analytic pair only; use "
                                          "the LDS passes or temporal = 1");
    W3D_REQUIRE(!sch_.sdma, "sources: not on the copy-engine transport (peers write this rank's ghost planes on their "
                            "own streams; that they carry uncorrected values is not argued for it yet)");
    W3D_REQUIRE(sch_.world == 1 || loopback_, "sources: one rank or an in-process group only (ranks of a multi-process "
                                              "world are not supported)");
    W3D_REQUIRE(resume_n_ == 0, "sources: not together with set_state (a resumed solve has no step 0 to start the "
                                "wavelet from)");
  }
  const std::vector<double> a = source_addends(sch_.prob, ijk, Q, w);  // (refuses bad nodes and samples)
  sponge_check_nodes(ijk, Q, "source");
  std::vector<std::array<i64, 3>> nodes(static_cast<size_t>(Q));
  for (int q = 0; q < Q; ++q) nodes[static_cast<size_t>(q)] = {ijk[3 * q], ijk[3 * q + 1], ijk[3 * q + 2]};
  // (radius: the largest ball any pass needs, so one plan and one set of colour classes serves every unit)
  SourcePlan plan = plan_sources(sch_.prob, sch_.dims, sch_.rank, sch_.lay, nodes, kSourceMaxSteps - 1);
  DeviceScope scope(dev_, true);
  drop_graphs();
  if (src_dev_) W3D_HIP(hipFree(src_dev_));
  if (src_a_) W3D_HIP(hipFree(src_a_));
  src_dev_ = nullptr;
  src_a_ = nullptr;
  src_ = std::move(plan);
  n_src_ = Q;
  if (src_.table.empty()) return;
  W3D_HIP(hipMalloc(&src_dev_, src_.table.size() * sizeof(Source)));
  W3D_HIP(hipMemcpy(src_dev_, src_.table.data(), src_.table.size() * sizeof(Source), hipMemcpyHostToDevice));
  W3D_HIP(hipMalloc(&src_a_, a.size() * sizeof(double)));
  W3D_HIP(hipMemcpy(src_a_, a.data(), a.size() * sizeof(double), hipMemcpyHostToDevice));
}

void GpuSolver::source_correct(const UnitPlan* u, double* prev, double* last) {
  if (src_.table.empty()) return;
  timed(kPhaseCompute, s0_, [&] {
    launch_source_cone(sch_.lay, coef_, prev, last, u ? u->n : 0, u ? u->steps : 1, u == nullptr, src_dev_,
                       src_.class_begin.data(), src_.classes(), src_a_, n_src_, u ? recv_dev_ : nullptr, u ? n_recv() : 0,
                       trace_, n_recv(), s0_);
  });
}

Partial GpuSolver::energy_sums(int which) const {
  W3D_REQUIRE(sch_.world == 1, "energy: one rank only (multi-rank: Solver.energy assembles the global fields)");
  W3D_REQUIRE(which == 0 || which == 1, "energy: which is 0 (E at K-1/2) or 1 (E at 1/2)");
  W3D_REQUIRE(!order4(), "order: the second-order discrete energy is not the conserved quantity of the order = 4 scheme");
  W3D_REQUIRE(!speed(), "speed: k_energy has no mass weight 1/c^2; Solver.energy downloads both levels and runs cpu_energy");
  W3D_REQUIRE(runs_ > 0 && (!initial_ || initial_runs_ > 0), "energy: no solve has run yet");
  W3D_REQUIRE(which == 0 || initial_, "energy: E(1/2) is kept by solves that start from set_initial");
  DeviceScope scope(dev_, true);
  energy_alloc();
  const int n = energy_partials(sch_.lay);
  if (which == 0) {
    materialise_prev();
    launch_energy(sch_.lay, coef_, sch_.prob.tau, u_[prev_buf_], u_[final_buf_], energy_part_, nullptr);
    launch_energy_reduce(energy_part_, n, energy_part_ + n, nullptr);
  }
  Partial h;
  W3D_HIP(hipMemcpy(&h, energy_part_ + n + which, sizeof h, hipMemcpyDeviceToHost));
  return h;
}

double GpuSolver::energy(int which) const {
  const Partial s = energy_sums(which);
  return energy_value(sch_.prob, s.x, s.y);
}

void GpuSolver::set_state(const double* prev, const double* cur, int n0) {
  W3D_REQUIRE(n0 >= 1 && n0 < sch_.prob.K, "resume step must be in [1, K)");
  W3D_REQUIRE(sch_.mode != Mode::kDeepTb || sch_.prob.K - n0 >= 2, "resume: the multi-rank LDS passes need >= 2 steps left");
  W3D_REQUIRE(sch_.mode != Mode::kDeep || (sch_.prob.K - n0) % 2 == 0, "resume: two-step passes need an even step count left");
  W3D_REQUIRE(n_src_ == 0, "sources: not together with set_state (a resumed solve has no step 0 to start the wavelet from)");
  W3D_REQUIRE(!speed(), "speed: not together with set_state / --resume");
  W3D_REQUIRE(!order4(), "order: not together with set_state / --resume");
  if (initial_) {  // (the two starts replace each other)
    W3D_HIP(hipDeviceSynchronize());
    for (double*& p : init_) {
      if (p) W3D_HIP(hipFree(p));
      p = nullptr;
    }
    initial_ = false;
  }
  drop_graphs();
  for (int k = 0; k < 2; ++k) {
    resume_[k].assign(static_cast<size_t>(sch_.lay.total), 0.0);
    global_to_local(sch_.lay, k == 0 ? prev : cur, resume_[k].data());
  }
  resume_n_ = n0;
}

std::vector<int> GpuSolver::check_steps() const {
  std::vector<int> v;
  for (int n = resume_n_ + 1; n <= sch_.prob.K; ++n)
    if (sch_.is_check(n)) v.push_back(n);
  return v;
}

std::string GpuSolver::transport() const {
  if (sch_.world == 1) return "none";
  if (sch_.sdma) return "sdma";
  if (sch_.push) return "push";
  if (sch_.opt.fake_comm) return sch_.opt.fake_traffic && comm_ ? "fake-rccl-self" : "fake";
  if (loopback_) return comm_ ? "rccl-self" : "loopback";
  return "rccl";
}

// schedule (decided in schedule.cpp; from here on: its launch sequence)
double* GpuSolver::msg_buf(MsgField f, bool send, const int uf[2]) const {
  switch (f) {
    case MsgField::kOut1: return u_[uf[0]];
    case MsgField::kOut2: return u_[uf[1]];
    case MsgField::kCurrent: return u_[sch_.post_exchange() ? old_ : cur_];
    default: return send ? send_buf_ : recv_buf_;
  }
}

void GpuSolver::phase_init() {
  const int K = sch_.prob.K;
  const double* s = d_s_ + 1;
  is_check_.assign(static_cast<size_t>(K + 1), 0);
  for (int n : check_steps()) is_check_[static_cast<size_t>(n)] = 1;
  cur_unit_ = -1;
  ev_next_ = 0;
  marks_.clear();
  // (the log's checked entries are rewritten by every solve and the others stay 0 from the allocation: cleared only
  // where something else writes into it — the copy-engine and push waits report their status there — or a resumed
  // solve leaves the entries below its start alone)
  if (sch_.sdma || sch_.push || resume_n_ > 0)
    W3D_HIP(hipMemsetAsync(errlog_, 0, static_cast<size_t>(K + 1) * sizeof(Partial), s0_));
  if (sch_.push) push_begin_solve();
  // (receivers: NaN in every row until this solve writes it)
  if (trace_)
    W3D_HIP(hipMemsetAsync(trace_, 0xFF, static_cast<size_t>(K + 1) * recv_.size() * sizeof(double), s0_));
  // one rank on the LDS kernel: the first pass starts from the analytic u⁰, u¹ itself (no init kernel, no reads)
  analytic_ = (sch_.mode == Mode::kFusedSingle || sch_.mode == Mode::kDeepTb) && sch_.analytic_ok() && resume_n_ == 0 &&
              !initial_ && !recording_ && n_src_ == 0 && !sponge() && !speed() && !order4();  // (receivers: both start levels are stored, rows 0
                                                        // and 1 are gathered; sources: u¹ is corrected in memory;
                                                        // sponge layers: the start is stored, as with receivers)
  if (resume_n_ > 0) {  // loaded state: u^{n0−1} → buf 0, u^{n0} → buf 1 (ghosts included)
    const size_t bytes = static_cast<size_t>(sch_.lay.bytes());
    timed(kPhaseInit, s0_, [&] {
      W3D_HIP(hipMemcpyAsync(u_[0], resume_[0].data(), bytes, hipMemcpyHostToDevice, s0_));
      W3D_HIP(hipMemcpyAsync(u_[1], resume_[1].data(), bytes, hipMemcpyHostToDevice, s0_));
    });
    start_n_ = resume_n_;
  } else if (initial_ || speed() || order4()) {  // user-supplied φ, ψ: u⁰ → buf 0, u¹ → buf 1 (ghosts included) from the device-resident copies
    // (a speed field without set_initial: init_[0] is the eigenmode array, init_[1] null; the coefficient per node.
    // order 4 without set_initial likewise; its coefficients select the kernel's fourth-order form)
    timed(kPhaseInit, s0_, [&] {
      if (time_order4())  // (v: buffer 2, whose faces stay the zeros of its allocation — only k_lap4 writes it)
        launch_first_step_t4(sch_.lay, init_lay_, coef_, sch_.prob.tau, init_[0], init_[1], u_[2], u_[0], u_[1],
                             sch_.opt.tiling, s0_);
      else
        launch_first_step_field(sch_.lay, init_lay_, coef_, sch_.prob.tau, init_[0], init_[1], u_[0], u_[1], s0_, lamf_dev_);
    });
    timed(kPhaseCheck, s0_, [&] {
      if (energy_part_ && sch_.world == 1 && !speed() && !order4()) {  // E^{1/2}, kept in its device slot
        const int ne = energy_partials(sch_.lay);
        launch_energy(sch_.lay, coef_, sch_.prob.tau, u_[0], u_[1], energy_part_, s0_);
        launch_energy_reduce(energy_part_, ne, energy_part_ + ne + 1, s0_);
      }
      check_stored(1, u_[1]);
    });
    start_n_ = 1;
  } else if (analytic_) {
    start_n_ = 1;
  } else if (sch_.opt.init2 && K >= 2 && !recording_ && n_src_ == 0 && !sponge()) {
    // u¹ -> buf 0, u² -> buf 1 analytically (no read pass), ghosts included; the first leapfrog step is n = 2
    timed(kPhaseInit, s0_, [&] {
      launch_init_two(sch_.lay, coef_, s, u_[0], u_[1], ct_[2], is_check_[2] ? partials_ : nullptr, s0_);
    });
    timed(kPhaseCheck, s0_, [&] {
      if (is_check_[2]) launch_reduce(partials_, init_two_partials(sch_.lay), errlog_ + 2, s0_);
      check_stored(1, u_[0]);
    });
    start_n_ = 2;
  } else {
    timed(kPhaseInit, s0_, [&] { launch_init_first(sch_.lay, coef_, s, u_[0], u_[1], s0_); });
    timed(kPhaseCheck, s0_, [&] { check_stored(1, u_[1]); });
    start_n_ = 1;
  }
  // sources: ½·a⁰ on u¹ (every start above but init2 left u⁰ in buffer 0 and u¹ in buffer 1), before the gathers below
  if (n_src_ > 0) source_correct(nullptr, u_[0], u_[1]);
  if (recording_) {  // (every start above but init2 left u^{start−1} in buffer 0 and u^{start} in buffer 1)
    timed(kPhaseCheck, s0_, [&] {
      record_stored(start_n_ - 1, u_[0]);
      record_stored(start_n_, u_[1]);
    });
  }
  cur_ = 1;
  old_ = 0;
  // (sponge layers: like sources, the last pass keeps both levels — a rebuild would need the slabs' recomputation too)
  units_ = plan_units(sch_, start_n_, analytic_, n_src_ > 0 || sponge(), speed_plan());
  speed_fused_ = speed_plan() == SpeedPlan::kFused;  // (the units are pair-tiled passes that read lamf)
  if (sch_.push) push_upload();
}

// the stored field `buf` of step n against the analytic solution, into the log (nothing unless step n is checked)
void GpuSolver::check_stored(int n, const double* buf) {
  if (!is_check_[static_cast<size_t>(n)]) return;
  launch_error(sch_.lay, buf, sch_.full, d_s_ + 1, ct_[static_cast<size_t>(n)], partials_, s0_);
  launch_reduce(partials_, error_blocks(sch_.lay, sch_.full), errlog_ + n, s0_);
}

void GpuSolver::unit_shell(int i) {
  cur_unit_ = i;
  const UnitPlan& u = units_[static_cast<size_t>(i)];
  if (u.fused()) {
    int k = 0;
    for (int b = 0; b < 4; ++b)
      if (b != cur_ && b != old_) uf_[k++] = b;
  }
  // (s0: every pass of the unit follows it there — the shells on the side stream wait for ev_shell_, recorded below —
  // and the previous unit's passes, which read that plane of the same buffer as a ghost, precede it)
  // sources: the previous unit's outputs (old_, cur_ since its unit_interior) get its forcing's response before anything
  // reads them. Its exchange has been joined into s0 (in a group: every rank's, lb_fence), so the ghost planes that
  // travelled carried uncorrected values and every rank corrects its own allocation (solver.hpp set_sources).
  if (n_src_ > 0 && i > 0) source_correct(&units_[static_cast<size_t>(i) - 1], u_[old_], u_[cur_]);
  if (sch_.opt.poison_ghosts && u.ghost_bits) poison(u, uf_, s0_, true);
  // receivers: the unit's levels from its inputs, whose ghosts are complete here (the previous unit's exchange has been
  // joined into s0) and which nothing writes before the next unit's pass
  if (recording_ && u.fused()) timed(kPhaseCheck, s0_, [&] { record_unit(u); });
  const int nc = u.n + u.steps;
  const bool chk = is_check_[static_cast<size_t>(nc)] != 0;
  if (sch_.mode == Mode::kDeep) {
    int off = 0;
    for (size_t k = 0; k < sch_.dshell.size(); ++k) {
      timed(kPhaseShell, s0_, [&] {
        launch_leapfrog2(sch_.lay, coef_, u_[old_], u_[cur_], u_[uf_[0]], u_[uf_[1]], sch_.dshell[k], d_s_ + 1,
                         ct_[static_cast<size_t>(nc)], chk ? partials_ + off : nullptr, sch_.opt.tiling2, s0_, sch_.sx0, sch_.sx1);
      });
      off += n_dshell_[k];
    }
  } else if (sch_.mode == Mode::kDeepTb) {
    // the regions the neighbours receive (u.shells) first, on the side stream, CONCURRENTLY with the interior pass
    // that unit_interior launches on s0 (same inputs, disjoint outputs): the shells' partial last waves leave CUs the
    // interior fills, and the exchange follows the shells on the same side stream (no wait between sibling streams)
    tb_slots_ = 0;
    if (u.exchange && !sch_.late_exchange()) {
      hipStream_t xs = xstream();
      if (sch_.opt.shells_concurrent) {
        capture::record(ev_shell_, s0_);  // (the unit's inputs are ready: fork)
        capture::wait(xs, ev_shell_);
        for (const LBox& b : u.shells) tb_pass(u, b, kPhaseShell, xs);
      } else {
        // (serial: the shells own the GPU and finish first, so the exchange starts as early as possible; all of them
        // in one pair-tiled launch where that applies — each alone left CUs idle, profiles/r6/)
        if (!tb_pass_boxes(u, u.shells, kPhaseShell, s0_))
          for (const LBox& b : u.shells) tb_pass(u, b, kPhaseShell, s0_);
        capture::record(ev_shell_, s0_);
        capture::wait(xs, ev_shell_);
      }
      return;
    }
  } else if (sch_.mode == Mode::kSingleStep && sch_.split()) {
    timed(kPhaseShell, s0_, [&] {
      launch_leapfrog(sch_.lay, coef_, u_[cur_], u_[old_], sch_.shell.data(), static_cast<int>(sch_.shell.size()), d_s_ + 1,
                      ct_[static_cast<size_t>(nc)], chk ? partials_ : nullptr, sch_.opt.tiling, s0_, sponge_arg());
    });
  }
  if (u.exchange) capture::record(ev_shell_, s0_);
}

const double* GpuSolver::peer_send(const MsgPlan& m, const std::vector<GpuSolver*>& ranks) const {
  const GpuSolver* q = ranks[static_cast<size_t>(m.peer)];
  const MsgPlan* g = nullptr;
  for (const MsgPlan& h : q->units_[static_cast<size_t>(cur_unit_)].msgs)
    if (h.peer == sch_.rank && h.tag == m.tag) g = &h;
  W3D_REQUIRE(g && g->count == m.count, "group exchange: mismatched messages");
  return q->msg_send(*g);
}

bool GpuSolver::packs() const { return (sch_.mode == Mode::kSingleStep && sch_.halo.packed_doubles > 0) || sch_.block_tb; }

void GpuSolver::pack_halo(hipStream_t st) {
  const int d = units_[static_cast<size_t>(cur_unit_)].depth;
  if (sch_.block_tb)
    launch_box_copy(sch_.lay, pack_tab_[d], 0, u_[uf_[1]], u_[uf_[0]], send_buf_ + sch_.sbase[d], st);
  else if (sch_.mode == Mode::kSingleStep && sch_.halo.packed_doubles > 0)
    launch_pack(sch_.lay, sch_.halo, msg_buf(MsgField::kCurrent, true, uf_), send_buf_, st);
}

void GpuSolver::unpack_halo(hipStream_t st) {
  if (sch_.block_tb)
    launch_box_copy(sch_.lay, unpack_tab_[units_[static_cast<size_t>(cur_unit_)].depth], 1, u_[uf_[1]], u_[uf_[0]],
                    recv_buf_, st);
  else if (sch_.mode == Mode::kSingleStep && sch_.halo.packed_doubles > 0)
    launch_unpack(sch_.lay, sch_.halo, recv_buf_, msg_buf(MsgField::kCurrent, false, uf_), st);
}

void GpuSolver::exchange(hipStream_t st, const std::vector<GpuSolver*>* pull) {
  const bool packed = packs();
  const std::vector<MsgPlan>& msgs = units_[static_cast<size_t>(cur_unit_)].msgs;
  if (packed && !pull) pack_halo(st);  // (group: each rank packed its own faces)
  if (sch_.opt.fake_comm && sch_.opt.fake_traffic && comm_) {
    // perf study: the rank's real message set, sent to and received from itself over a
    // one-rank communicator — RCCL's copy kernels, CU and LDS use and bytes as in the real exchange
    ncclComm_t c = static_cast<ncclComm_t>(comm_->raw());
    W3D_NCCL(ncclGroupStart());
    for (const MsgPlan& m : msgs) {
      W3D_NCCL(ncclSend(msg_send(m), static_cast<size_t>(m.count), ncclFloat64, 0, c, st));
      W3D_NCCL(ncclRecv(msg_recv(m), static_cast<size_t>(m.count), ncclFloat64, 0, c, st));
    }
    W3D_NCCL(ncclGroupEnd());
  } else if (!sch_.opt.fake_comm) {  // fake_comm (perf study): one rank's schedule timed alone, ghosts keep stale values
    ncclComm_t c = static_cast<ncclComm_t>(comm_->raw());
    W3D_NCCL(ncclGroupStart());
    for (const MsgPlan& m : msgs) {
      // (pull, a one-rank communicator: the k-th send to self pairs with the k-th receive from self)
      W3D_NCCL(ncclSend(pull ? peer_send(m, *pull) : msg_send(m), static_cast<size_t>(m.count), ncclFloat64,
                        pull ? 0 : m.peer, c, st));
      W3D_NCCL(ncclRecv(msg_recv(m), static_cast<size_t>(m.count), ncclFloat64, pull ? 0 : m.peer, c, st));
    }
    W3D_NCCL(ncclGroupEnd());
  }
  if (packed) unpack_halo(st);
}

void GpuSolver::unit_exchange_rccl(int i) {
  if (!needs_exchange(i)) return;
  hipStream_t xs = xstream();
  // (deep-tb: the shells ran on xs itself, after its wait for the unit's inputs)
  if (xs != s0_ && sch_.mode != Mode::kDeepTb) capture::wait(xs, ev_shell_);
  if (sch_.opt.poison_ghosts) poison(units_[static_cast<size_t>(i)], uf_, xs);
  timed(kPhaseComm, xs, [&] { exchange(xs); });
  if (xs != s0_) capture::record(ev_halo_, xs);
}

PassArgs GpuSolver::tb_args_fields(const UnitPlan& u, int prev, int cur, int out1, int out2) const {
  PassArgs a;
  a.prev = u_[prev];
  a.cur = u_[cur];
  a.out1 = u_[out1];
  a.out2 = u_[out2];
  a.d_s = d_s_ + 1;
  a.tiling = sch_.opt.tiling_tb;
  a.tiling.stages = u.steps;
  a.tiling.ghost_x1 = u.ghost_bits;
  for (int k = 1; k <= u.steps; ++k) a.ct[k - 1] = ct_[static_cast<size_t>(u.n + k)];
  a.grid_blocks = n_tb_;
  a.real = sch_.mode == Mode::kDeepTb ? sch_.sreal : tb_default_real();
  a.analytic_start = u.analytic;
  a.lamf = speed_fused_ ? lamf_dev_ : nullptr;  // (a speed field: the passes' coefficient form)
  return a;
}

PassArgs GpuSolver::tb_args(const UnitPlan& u) {
  PassArgs a = tb_args_fields(u, old_, cur_, uf_[0], uf_[1]);
  if (u.drop_prev) a.out1 = nullptr;  // (u^{n+S−1} of the solve's last pass: materialise_prev)
  for (int k = 1; k <= u.steps; ++k)
    if (is_check_[static_cast<size_t>(u.n + k)]) a.check_mask |= 1 << (k - 1);
  a.level_stride = tb_level_stride();
  W3D_REQUIRE((tb_slots_ + 1) * n_tb_ <= a.level_stride, "leapfrog_tb: too many launches in one unit");
  // (every launch fills its whole slot of n_tb_ partials: shell and interior boxes may have fewer x chunks)
  if (a.check_mask) a.partials = tb_region(tb_region_) + tb_slots_++ * n_tb_;
  return a;
}

// u^{K−1} of a solve whose last pass left it out (UnitPlan::drop_prev): that one unit again, eagerly on s0 and outside
// any graph, with out1 set. Its inputs are the two other buffers of the four-buffer rotation, ghost layers included, and
// nothing has written them since the unit (it is the last, and it has no exchange), so the same kernel on the same
// inputs stores the same bits — u^K over itself, and the missing level. No check and no partials: the error log, the
// partial regions, pending reductions and the captured graph are not touched.
void GpuSolver::materialise_prev() const {
  if (!prev_missing_) return;
  const UnitPlan& u = units_.back();
  DeviceScope scope(dev_, true);
  PassArgs a = tb_args_fields(u, last_in_[0], last_in_[1], prev_buf_, final_buf_);
  launch_leapfrog_tb(sch_.lay, coef_, u.interior, a, s0_);
  W3D_HIP(hipStreamSynchronize(s0_));
  prev_missing_ = false;
}

// One LDS S-step pass of unit u over `box` on stream st (s0 unless given). Its checked levels' partials go to slot
// tb_slots_ of each level: one slot per level on one rank, up to kTbSlots on multi-rank ranks (the shell boxes, then
// the interior), reduced together after the interior.
void GpuSolver::tb_pass(const UnitPlan& u, const LBox& box, int phase, hipStream_t st) {
  if (st == nullptr) st = s0_;
  PassArgs a = tb_args(u);
  if (sch_.push) push_pass_args(a);
  if (tb_packs(u)) {
    a.pack = &pk_host_[u.depth];
    a.pack_dev = pk_dev_ + u.depth;
  }
  timed(phase, st, [&] { launch_leapfrog_tb(sch_.lay, coef_, box, a, st); });
}

bool GpuSolver::tb_pass_boxes(const UnitPlan& u, const std::vector<LBox>& boxes, int phase, hipStream_t st) {
  // (only where the pair-tiled pass runs every box, the shells' tiles alone do not fill the GPU and the combined grid
  // fits the partial slot: pass_grid.hpp; otherwise one launch per box, each of which fits)
  LeapfrogTbTiling ts = sch_.opt.tiling_tb;
  ts.stages = u.steps;
  if (tb_shells_launch_blocks(sch_.lay, boxes.data(), static_cast<int>(boxes.size()), ts, n_tb_, u.analytic, sch_.push,
                              tb_packs(u)) == 0)
    return false;
  PassArgs a = tb_args(u);
  // (no XCD remap: the boxes' workgroups differ in length, and a contiguous logical range per XCD put the long ones
  // on a few XCDs; dispatch order deals consecutive workgroups to the XCDs round-robin)
  a.tiling.xcd_remap = false;
  timed(phase, st, [&] {
    launch_leapfrog_p2_boxes(sch_.lay, coef_, boxes.data(), static_cast<int>(boxes.size()), a, st);
  });
  return true;
}

void GpuSolver::unit_interior(int i) {
  const UnitPlan& u = units_[static_cast<size_t>(i)];
  const int nc = u.n + u.steps;
  const bool chk = is_check_[static_cast<size_t>(nc)] != 0;
  const double ct = ct_[static_cast<size_t>(nc)];
  const double* s = d_s_ + 1;
  // (group ranks: lb_fence already put s0 behind every rank's pull, ev_halo_ included; a second, redundant wait on
  // the own side stream after that fence crashes HIP 7.2's hipStreamEndCapture — tools/probes/capture_probe2.hip flag 36)
  const bool wait = needs_exchange(i) && xstream() != s0_ && (!loopback_ || sch_.sdma);
  int np = 0;  // partials to reduce
  bool joined = false;
  if (time_order4()) {  // (two launches per single step: v = τ²L_h u^n into buffer 2, then the update from v)
    timed(kPhaseCompute, s0_, [&] {
      launch_lap4(sch_.lay, coef_, u_[cur_], u_[2], &sch_.full, 1, sch_.opt.tiling, s0_);
      launch_leapfrog44(sch_.lay, coef_, u_[cur_], u_[2], u_[old_], &sch_.full, 1, s, ct, chk ? partials_ : nullptr,
                        sch_.opt.tiling, s0_);
    });
    np = n_full4_;
  } else if (order4()) {  // (single steps only: plan_units; one rank, so no shell preceded it)
    timed(kPhaseCompute, s0_, [&] {
      launch_leapfrog4(sch_.lay, coef_, u_[cur_], u_[old_], &sch_.full, 1, s, ct, chk ? partials_ : nullptr, sch_.opt.tiling, s0_);
    });
    np = n_full4_;
  } else if (sch_.mode == Mode::kDeep) {
    int off = 0;
    for (int n : n_dshell_) off += n;
    if (!sch_.dint.empty()) {
      timed(kPhaseCompute, s0_, [&] {
        launch_leapfrog2(sch_.lay, coef_, u_[old_], u_[cur_], u_[uf_[0]], u_[uf_[1]], sch_.dint, s, ct,
                         chk ? partials_ + off : nullptr, sch_.opt.tiling2, s0_, sch_.sx0, sch_.sx1);
      });
    }
    np = off + n_dint_;
  } else if ((sch_.mode == Mode::kFusedSingle && sch_.opt.tb && u.fused() && (!speed() || speed_fused_)) ||
             sch_.mode == Mode::kDeepTb) {
    // S steps in one LDS pass (on slab ranks: the interior left between this unit's shells); every checked level
    // has its own block of partials
    if (sch_.mode != Mode::kDeepTb) tb_slots_ = 0;
    const LBox& b = u.interior;
    if (!b.empty()) tb_pass(u, b, kPhaseCompute);
    sponge_unit(u);  // (sponge layers: the slabs of both outputs again, damped, from the unit's inputs)
    // (the shells ran on the side stream: join it before the reductions read their partials)
    if (wait) {
      capture::wait(s0_, ev_halo_);
      joined = true;
    }
    if (tb_slots_ > 0) {
      for (int k = 1; k <= u.steps; ++k)
        if (is_check_[static_cast<size_t>(u.n + k)])
          pending_.push_back(ReduceJob{tb_region(tb_region_) + (k - 1) * tb_level_stride(), tb_slots_ * n_tb_,
                                       errlog_ + u.n + k});
      tb_region_ = (tb_region_ + 1) % kTbRegions;
      if (tb_region_ == 0 || sch_.opt.timers) flush_reduces();  // the next unit reuses region 0 / per-unit check time
    }
  } else if (sch_.mode == Mode::kFusedSingle) {
    timed(kPhaseCompute, s0_, [&] {
      if (u.fused())
        launch_leapfrog2(sch_.lay, coef_, u_[old_], u_[cur_], u_[uf_[0]], u_[uf_[1]], sch_.full, s, ct,
                         chk ? partials_ : nullptr, sch_.opt.tiling2, s0_, 1, 0, lamf_dev_);
      else
        launch_leapfrog(sch_.lay, coef_, u_[cur_], u_[old_], &sch_.full, 1, s, ct, chk ? partials_ : nullptr, sch_.opt.tiling,
                        s0_, sponge_arg(), lamf_dev_);
    });
    np = u.fused() ? n_fused_ : n_full_;
  } else if (sch_.split()) {
    timed(kPhaseCompute, s0_, [&] {
      launch_leapfrog(sch_.lay, coef_, u_[cur_], u_[old_], &sch_.interior, 1, s, ct, chk ? partials_ + n_shell_ : nullptr,
                      sch_.opt.tiling, s0_, sponge_arg());
    });
    np = n_shell_ + n_int_;
  } else {
    timed(kPhaseCompute, s0_, [&] {
      launch_leapfrog(sch_.lay, coef_, u_[cur_], u_[old_], &sch_.full, 1, s, ct, chk ? partials_ : nullptr, sch_.opt.tiling,
                      s0_, sponge_arg(), lamf_dev_);
    });
    np = n_full_;
  }
  if (wait && !joined) capture::wait(s0_, ev_halo_);
  if (chk && np > 0) timed(kPhaseCheck, s0_, [&] { launch_reduce(partials_, np, errlog_ + nc, s0_); });
  // receivers: a single step's new level, stored in place over u^{n−1} (owned nodes only: no ghost is read)
  if (recording_ && !u.fused()) timed(kPhaseCheck, s0_, [&] { record_stored(nc, u_[old_]); });
  if (sch_.opt.debug_sync) W3D_HIP(hipDeviceSynchronize());
  last_in_[0] = old_;
  last_in_[1] = cur_;
  if (u.fused()) {
    old_ = uf_[0];
    cur_ = uf_[1];
  } else {
    std::swap(cur_, old_);
  }
  final_buf_ = cur_;
  prev_buf_ = old_;
}

// sources: the last unit's correction, at the end of the solve (no unit_shell follows it)
void GpuSolver::source_finish() {
  if (n_src_ > 0 && !units_.empty()) source_correct(&units_.back(), u_[old_], u_[cur_]);
}

void GpuSolver::flush_reduces() {
  if (pending_.empty()) return;
  timed(kPhaseCheck, s0_, [&] { launch_reduce_batch(pending_.data(), static_cast<int>(pending_.size()), s0_); });
  pending_.clear();
}

void GpuSolver::enqueue_solve() {
  if (sch_.sdma) sdma_check_connected();
  phase_init();
  // copy-engine flag values are 16-bit unit indices under a parity bit (xval / xend): more units per solve would alias
  // the end-of-solve word and the other parity's range
  W3D_REQUIRE(!sch_.sdma || units_.size() < 0xFFFEu, "sdma transport: too many passes in one solve for the flag encoding");
  tb_region_ = 0;
  pending_.clear();
  const bool late = sch_.late_exchange();
  for (int i = 0; i < static_cast<int>(units_.size()); ++i) {
    if (sch_.sdma) sdma_receive(i);
    unit_shell(i);
    if (!late) unit_exchange(i);
    unit_interior(i);
    if (late) unit_exchange(i);
  }
  source_finish();
  flush_reduces();
  if (sch_.push) push_finish(s0_);
  if (sch_.sdma) sdma_finish();
  push_epoch_ += static_cast<int>(units_.size());
  final_buf_ = cur_;
  prev_buf_ = old_;
}

// Debug aid: fill the ghost regions that the next exchange must overwrite with NaN, so a halo that
// is not delivered shows up in the error norms at once instead of silently reusing stale values.
// before_pass: the ghost plane the unit's own passes store instead (schedule.hpp plan_poison), filled before they run.
void GpuSolver::poison(const UnitPlan& u, const int uf[2], hipStream_t st, bool before_pass) {
  if (sch_.block_tb) {  // the ghost regions themselves (the messages land in a staging buffer first)
    if (!before_pass) launch_box_copy(sch_.lay, unpack_tab_[u.depth], 2, u_[uf[1]], u_[uf[0]], nullptr, st);
    return;
  }
  for (const PoisonRange& p : plan_poison(sch_, u)) {
    if (p.before_pass != before_pass) continue;
    double* dst = msg_buf(p.field, false, uf) + p.off;
    if (p.rows == 1)
      W3D_HIP(hipMemsetAsync(dst, 0xFF, static_cast<size_t>(p.count) * sizeof(double), st));
    else
      W3D_HIP(hipMemset2DAsync(dst, static_cast<size_t>(p.pitch) * sizeof(double), 0xFF,
                               static_cast<size_t>(p.count) * sizeof(double), static_cast<size_t>(p.rows), st));
  }
}

void GpuSolver::collect_phases(RunResult& r) {
  if (!sch_.opt.timers) return;
  double acc[kNumPhases] = {};
  r.trace.assign(units_.size(), UnitTrace{});
  for (size_t i = 0; i < units_.size(); ++i) {
    r.trace[i].unit = static_cast<int>(i);
    r.trace[i].n = units_[i].n;
    r.trace[i].steps = units_[i].steps;
  }
  for (const auto& m : marks_) {
    float ms = 0.0f;
    W3D_HIP(hipEventElapsedTime(&ms, m.b, m.e));
    acc[m.phase] += ms;
    if (m.unit < 0 || m.unit >= static_cast<int>(r.trace.size())) continue;
    UnitTrace& t = r.trace[static_cast<size_t>(m.unit)];
    (m.phase == kPhaseShell ? t.shell_ms : m.phase == kPhaseComm ? t.comm_ms : m.phase == kPhaseCheck ? t.check_ms
                                                                                                 : t.compute_ms) += ms;
  }
  r.phases.init_ms = acc[kPhaseInit];
  r.phases.shell_ms = acc[kPhaseShell];
  r.phases.interior_ms = acc[kPhaseCompute];
  r.phases.comm_ms = acc[kPhaseComm];
  r.phases.check_ms = acc[kPhaseCheck];
  r.phases.gather_ms = acc[kPhaseGather];  // device: the error log's all-gather and D2H copy after the last pass
}

// ------------------------------------------------------------------------------------------------------------------
// loopback transport (GpuGroup): P ranks in one process on one device, halos moved by device copies. Test-only
// stand-in for RCCL that exercises the identical schedules, shell/interior splits, message plans, pack/unpack and
// stream/event ordering of the production path on a single GPU (RCCL refuses two ranks on one device).
// ------------------------------------------------------------------------------------------------------------------
void GpuSolver::lb_pack(int i) {
  if (!needs_exchange(i)) return;
  hipStream_t xs = xstream();
  if (xs != s0_ && sch_.mode != Mode::kDeepTb) capture::wait(xs, ev_shell_);
  pack_halo(xs);
  capture::record(ev_packed_, xs);
}

void GpuSolver::lb_pull(int i, const std::vector<GpuSolver*>& ranks, hipEvent_t all_packed) {
  if (!needs_exchange(i)) return;
  hipStream_t xs = xstream();
  if (sch_.opt.poison_ghosts) poison(units_[static_cast<size_t>(i)], uf_, xs);
  capture::wait(xs, all_packed);  // every peer's faces are packed
  if (comm_) {  // rccl-self: the production exchange (RCCL send/recv on xs) over this rank's one-rank communicator
    timed(kPhaseComm, xs, [&] { exchange(xs, &ranks); });
  } else {
    for (const MsgPlan& m : units_[static_cast<size_t>(i)].msgs)
      W3D_HIP(hipMemcpyAsync(msg_recv(m), peer_send(m, ranks), static_cast<size_t>(m.count) * sizeof(double),
                             hipMemcpyDeviceToDevice, xs));
    unpack_halo(xs);
  }
  capture::record(ev_halo_, xs);
}

void GpuSolver::lb_fence(int i, hipEvent_t all_pulled) {
  // the peers have read this rank's send regions once their pulls are done: keep both streams behind them (the side
  // stream only when this schedule uses it: a captured stream that only ever waits trips HIP 7.2's end of capture)
  if (!needs_exchange(i)) return;
  capture::wait(s0_, all_pulled);
  if (xstream() != s0_) capture::wait(s1_, all_pulled);
}

void GpuSolver::gather_errors(RunResult& r) {
  const int K = sch_.prob.K;
  const size_t per = static_cast<size_t>(K + 1);
  std::vector<Partial> host(per * static_cast<size_t>(sch_.world));
  cur_unit_ = -1;
  timed(kPhaseGather, s0_, [&] {
    if (sch_.world > 1 && comm_ && !sch_.opt.fake_comm) {  // (a fake rank's communicator is its own one-rank one)
      W3D_NCCL(ncclAllGather(errlog_, errall_, 2 * per, ncclFloat64, static_cast<ncclComm_t>(comm_->raw()), s0_));
      W3D_HIP(hipMemcpyAsync(host.data(), errall_, host.size() * sizeof(Partial), hipMemcpyDeviceToHost, s0_));
    } else {
      host.resize(per);
      W3D_HIP(hipMemcpyAsync(host.data(), errlog_, per * sizeof(Partial), hipMemcpyDeviceToHost, s0_));
    }
  });
  wait_stream(s0_, comm_.get(), gpu_timeout_s());
  push_check();
  decode_log(host.data(), static_cast<int>(host.size() / per), r);
}

void GpuSolver::decode_log(const Partial* host, int nsrc, RunResult& r) const {
  const size_t per = static_cast<size_t>(sch_.prob.K + 1);
  // copy-engine transport: a flag wait that timed out marked word 0 of that rank's log (step 0 is never checked)
  for (int q = 0; q < nsrc && sch_.sdma; ++q)
    W3D_REQUIRE(host[static_cast<size_t>(q) * per].x == 0.0,
                "sdma transport: a flag wait timed out on rank " + std::to_string(nsrc > 1 ? q : sch_.rank) +
                    " (a neighbour stopped or its copies never arrived)");
  static_assert(sizeof(Partial) == 2 * sizeof(double), "the log is read as (max, sum) pairs of doubles");
  static_cast<ErrorLog&>(r) =
      combine_error_log(reinterpret_cast<const double*>(host), nsrc, sch_.prob.K, sch_.prob.N, check_steps());
}

RunResult GpuSolver::run() {
  RunResult r;
  // RCCL ranks run their first solve eagerly: the peer connections (and RCCL's proxy threads) are set up at the
  // first send/recv, which must not happen inside a stream capture; the capture follows on the second run
  if (sch_.world > 1 && !multistream_capture_safe()) sch_.opt.graph = false;
  const bool capture_ok = !(sch_.world > 1 && comm_) || runs_ >= 1;
  // (copy-engine ranks: the flag values of a solve depend on its parity, so there is one graph per parity)
  xpar_ = static_cast<int>(xsolves_ & 1);
  hipGraphExec_t& gx = sch_.sdma ? xgraph_[xpar_] : graph_exec_;
  if (sch_.opt.graph && !gx && capture_ok && !sch_.opt.timers && resume_n_ == 0) {
    // capture once (outside the timed region of later runs); fall back to eager launches if capture is refused
    std::string thrown;
    gx = capture::graph(s0_, [this] { enqueue_solve(); }, &thrown);
    // (an error of the schedule itself is not a capture problem: report it instead of retrying eagerly on streams the
    // aborted capture may have left unusable)
    if (!thrown.empty()) fail("solve schedule failed while being captured: " + thrown);
    if (!gx) sch_.opt.graph = false;
  }
  const double t0 = now_s();
  if (gx && sch_.opt.graph && !sch_.opt.timers && resume_n_ == 0)
    W3D_HIP(hipGraphLaunch(gx, s0_));
  else
    enqueue_solve();
  ++xsolves_;
  gather_errors(r);
  r.solve_s = now_s() - t0;
  collect_phases(r);
  ++runs_;
  if (initial_) ++initial_runs_;
  solve_done();
  return r;
}

std::vector<RunResult> GpuSolver::run_batch(int n) {
  std::vector<RunResult> out;
  if (n <= 0) return out;
  // Graph-captured solves are enqueued back to back, each followed by its error-log gather (RCCL ranks: the all-gather
  // run() issues, on the same stream), and the host synchronises once: no host round trip between solves. Every rank
  // enqueues the same sequence, so the collectives match. (Copy-engine and push ranks carry per-solve flag epochs and
  // host-side checks between solves: one run() each.)
  const bool gathered = sch_.world > 1 && comm_ && !sch_.opt.fake_comm;
  const bool pipelined = !sch_.sdma && !sch_.push && sch_.opt.graph && graph_exec_ && !sch_.opt.timers && resume_n_ == 0 &&
                         (sch_.world == 1 || sch_.opt.fake_comm || gathered);
  if (!pipelined) {
    for (int i = 0; i < n; ++i) out.push_back(run());
    return out;
  }
  const size_t per = static_cast<size_t>(sch_.prob.K + 1);
  const int nsrc = gathered ? sch_.world : 1;
  const size_t slot = per * static_cast<size_t>(nsrc);
  if (hbatch_n_ < n * nsrc) {
    if (hbatch_) W3D_HIP(hipHostFree(hbatch_));
    hbatch_ = nullptr;
    W3D_HIP(hipHostMalloc(reinterpret_cast<void**>(&hbatch_), static_cast<size_t>(n) * slot * sizeof(Partial),
                          hipHostMallocDefault));
    hbatch_n_ = n * nsrc;
  }
  cur_unit_ = -1;
  const double t0 = now_s();
  for (int i = 0; i < n; ++i) {
    W3D_HIP(hipGraphLaunch(graph_exec_, s0_));
    // (stream order: this solve's log is gathered and copied out before the next replay's reductions overwrite it)
    if (gathered)
      W3D_NCCL(ncclAllGather(errlog_, errall_, 2 * per, ncclFloat64, static_cast<ncclComm_t>(comm_->raw()), s0_));
    W3D_HIP(hipMemcpyAsync(hbatch_ + static_cast<size_t>(i) * slot, gathered ? errall_ : errlog_,
                           slot * sizeof(Partial), hipMemcpyDeviceToHost, s0_));
  }
  // (the per-solve bound, per replay: a long timed block is not a hang)
  wait_stream(s0_, comm_.get(), gpu_timeout_s() * n);
  const double dt = (now_s() - t0) / n;
  xsolves_ += static_cast<unsigned>(n);
  runs_ += n;
  if (initial_) initial_runs_ += n;
  solve_done();
  for (int i = 0; i < n; ++i) {
    RunResult r;
    decode_log(hbatch_ + static_cast<size_t>(i) * slot, nsrc, r);
    r.solve_s = dt;
    r.batched = true;
    out.push_back(std::move(r));
  }
  return out;
}

std::vector<double> GpuSolver::download(int which) const {
  std::vector<double> h(static_cast<size_t>(sch_.lay.total));
  const double* src = u_[which == 0 ? final_buf_ : prev_buf_];
  DeviceScope scope(dev_, true);
  if (which != 0) materialise_prev();
  W3D_HIP(hipMemcpy(h.data(), src, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  return h;
}

unsigned long long GpuSolver::field_hash(int which) const {
  DeviceScope scope(dev_, true);
  unsigned long long* d = nullptr;
  W3D_HIP(hipMalloc(&d, sizeof(unsigned long long)));
  W3D_HIP(hipMemset(d, 0, sizeof(unsigned long long)));
  if (which != 0) materialise_prev();
  launch_field_hash(sch_.lay, u_[which == 0 ? final_buf_ : prev_buf_], d, nullptr);
  unsigned long long h = 0;
  W3D_HIP(hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost));
  W3D_HIP(hipFree(d));
  return h;
}

}  // namespace wave3d
