// GPU solver runtime. See wave3d/solver.hpp.
#include "wave3d/capture_guard.hpp"
#include "wave3d/pass_grid.hpp"
#include "wave3d/solver.hpp"

#include <rccl/rccl.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace wave3d {

#define W3D_NCCL(expr)                                                                               \
  do {                                                                                               \
    ncclResult_t _r = (expr);                                                                        \
    if (_r != ncclSuccess) ::wave3d::fail(std::string(#expr) + ": " + ncclGetErrorString(_r));        \
  } while (0)

// ------------------------------------------------------------------------------------------------------------------
// Comm
// ------------------------------------------------------------------------------------------------------------------
std::string Comm::make_unique_id() {
  ncclUniqueId id;
  W3D_NCCL(ncclGetUniqueId(&id));
  return std::string(id.internal, sizeof(id.internal));
}

Comm::Comm(int rank, int world, const std::string& unique_id) : rank_(rank), world_(world) {
  ncclUniqueId id;
  W3D_REQUIRE(unique_id.size() == sizeof(id.internal), "bad RCCL unique id size");
  std::memcpy(id.internal, unique_id.data(), sizeof(id.internal));
  ncclComm_t c = nullptr;
  W3D_NCCL(ncclCommInitRank(&c, world, id, rank));
  comm_ = c;
  // self-test: one all-reduce of 1 per rank must give the world size, and RCCL must report `world` ranks. A
  // communicator that cannot move data fails here (with RCCL's error or the GPU-wait timeout) instead of inside a
  // captured solve. Run for every size (a one-rank communicator of the rccl-self group included).
  try {
    W3D_REQUIRE(count() == world, "RCCL self-test: ncclCommCount gave " + std::to_string(count()));
    const double n = comm_allreduce(*this, 1.0, false);
    W3D_REQUIRE(n == static_cast<double>(world), "RCCL self-test: all-reduce of 1 per rank gave " + std::to_string(n));
  } catch (...) {
    ncclCommAbort(c);  // the destructor does not run for a throwing constructor
    comm_ = nullptr;
    throw;
  }
}

std::vector<std::shared_ptr<Comm>> Comm::init_all(int world) {
  W3D_REQUIRE(world >= 1, "init_all: world must be >= 1");
  std::vector<ncclComm_t> raw(static_cast<size_t>(world), nullptr);
  std::vector<int> devs(static_cast<size_t>(world));
  for (int r = 0; r < world; ++r) devs[static_cast<size_t>(r)] = r;
  W3D_NCCL(ncclCommInitAll(raw.data(), world, devs.data()));
  std::vector<std::shared_ptr<Comm>> out;
  for (int r = 0; r < world; ++r) {
    std::shared_ptr<Comm> c(new Comm());
    c->rank_ = r;
    c->world_ = world;
    c->comm_ = raw[static_cast<size_t>(r)];
    out.push_back(std::move(c));
  }
  return out;
}

int Comm::count() const {
  int n = 0;
  W3D_NCCL(ncclCommCount(static_cast<ncclComm_t>(comm_), &n));
  return n;
}

int Comm::device() const {
  int d = -1;
  W3D_NCCL(ncclCommCuDevice(static_cast<ncclComm_t>(comm_), &d));
  return d;
}

Comm::~Comm() {
  if (comm_) ncclCommDestroy(static_cast<ncclComm_t>(comm_));
}

void Comm::check_async() const {
  ncclResult_t st = ncclSuccess;
  W3D_NCCL(ncclCommGetAsyncError(static_cast<ncclComm_t>(comm_), &st));
  if (st != ncclSuccess && st != ncclInProgress) fail(std::string("RCCL async error: ") + ncclGetErrorString(st));
}

// ------------------------------------------------------------------------------------------------------------------
// GpuSolver
// ------------------------------------------------------------------------------------------------------------------
namespace {

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Upper bound for one blocking wait on the GPU (env W3D_TIMEOUT_S, default 300 s): a lost peer or a stuck halo
// exchange turns into an error instead of a hang.
double gpu_timeout_s() {
  static const double t = [] {
    const char* v = std::getenv("W3D_TIMEOUT_S");
    const double x = v ? std::atof(v) : 0.0;
    return x > 0.0 ? x : 300.0;
  }();
  return t;
}

// Wait for a stream while polling RCCL for asynchronous failures (a dead peer must not hang the job forever).
void wait_stream(hipStream_t s, const Comm* comm, double timeout_s) {
  const double t0 = now_s();
  for (;;) {
    const hipError_t e = hipStreamQuery(s);
    if (e == hipSuccess) return;
    if (e != hipErrorNotReady) fail(std::string("stream failed: ") + hipGetErrorString(e));
    if (comm) comm->check_async();
    if (now_s() - t0 > timeout_s) fail("timed out waiting for the GPU (halo exchange stuck?)");
    std::this_thread::yield();
  }
}

}  // namespace

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
  // (the push transport's kernels exist for cubes only: kernels_leapfrog_tb_push.hip)
  W3D_REQUIRE(!(o.push && world > 1 && coef_.box),
              "the push transport has no rectangular-box kernels: run a --box problem over rccl or sdma");
  W3D_REQUIRE(world == 1 || comm_ || loopback_ || o.fake_comm || ((o.push || o.sdma) && o.push_no_collective),
              "world > 1 needs an RCCL communicator (or the loopback group, or the push / sdma transport without one)");
  size_t free_b = 0, total_b = 0;
  W3D_HIP(hipMemGetInfo(&free_b, &total_b));
  sch_ = make_rank_schedule(prob, o, rank, world, static_cast<double>(free_b));

  // device memory
  if (const char* cs = std::getenv("W3D_CU_SPLIT"); cs && !loopback_ && (std::strchr(cs, '/') || !std::strcmp(cs, "auto"))) {
    // rehearsal of several ranks on ONE GPU with truly concurrent passes (W3D_CU_SPLIT=r/P, or auto = rank/world):
    // this rank's compute stream only gets the r-th of P disjoint CU ranges, so a pass waiting in the kernel for a
    // peer can never hold the CUs the peer's pass needs
    const bool au = !std::strcmp(cs, "auto");
    const int r = au ? rank : std::atoi(cs), P = au ? world : std::atoi(std::strchr(cs, '/') + 1);
    int dev = 0, ncu = 0;
    W3D_HIP(hipGetDevice(&dev));
    W3D_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    W3D_REQUIRE(P >= 1 && r >= 0 && r < P && ncu >= P, "W3D_CU_SPLIT must be r/P with 0 <= r < P <= CUs");
    std::vector<uint32_t> mask(static_cast<size_t>((ncu + 31) / 32), 0u);
    for (int c = r * ncu / P; c < (r + 1) * ncu / P; ++c) mask[static_cast<size_t>(c / 32)] |= 1u << (c % 32);
    W3D_HIP(hipExtStreamCreateWithCUMask(&s0_, static_cast<uint32_t>(mask.size()), mask.data()));
  } else if (sch_.opt.reserve_cus > 0) {
    int dev = 0, ncu = 0;
    W3D_HIP(hipGetDevice(&dev));
    W3D_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    W3D_REQUIRE(sch_.opt.reserve_cus < ncu, "reserve_cus must leave the passes at least one CU");
    std::vector<uint32_t> mask(static_cast<size_t>((ncu + 31) / 32), 0u);
    for (int c = 0; c < ncu - sch_.opt.reserve_cus; ++c) mask[static_cast<size_t>(c / 32)] |= 1u << (c % 32);
    W3D_HIP(hipExtStreamCreateWithCUMask(&s0_, static_cast<uint32_t>(mask.size()), mask.data()));
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
  if (sch_.push) {
    // staging in fine-grained device memory (W3D_PUSH_STAGING=uncached: uncached), flags uncached: the neighbours'
    // stores are write-through (system scope) and a reader invalidates its L2 once per pass after its wait
    // (system-scope acquire, leapfrog_tb_kernel.hpp)
    const size_t sb = static_cast<size_t>(8 * sch_.lay.xg * sch_.lay.plane) * sizeof(double);
    const char* mt = std::getenv("W3D_PUSH_STAGING");  // (experiment: "uncached" instead of fine-grained)
    const unsigned stg_flags = mt && !std::strcmp(mt, "uncached") ? hipDeviceMallocUncached : hipDeviceMallocFinegrained;
    W3D_HIP(hipExtMallocWithFlags(reinterpret_cast<void**>(&stg_), sb, stg_flags));
    W3D_HIP(hipMemset(stg_, 0, sb));
    W3D_HIP(hipExtMallocWithFlags(reinterpret_cast<void**>(&flags_), 256, hipDeviceMallocUncached));
    l2_flush_all(nullptr);  // (no stale dirty line of a freed cached buffer may land on them later: kernels.hpp)
    W3D_HIP(hipDeviceSynchronize());
    W3D_HIP(hipMemset(stg_, 0, sb));
    W3D_HIP(hipMemset(flags_, 0, 256));
    const size_t tb = static_cast<size_t>(sch_.prob.K) * sizeof(TbPush);  // (a solve has at most K passes)
    // two host tables: [0, K) for the captured solve (its H2D copy node reads the table at every replay), [K, 2K) for
    // eager solves — an eager solve after the capture (e.g. the phase-timer solve) must not rewrite the tags the graph's
    // kernel nodes were captured with
    W3D_HIP(hipHostMalloc(reinterpret_cast<void**>(&push_host_), 2 * tb, hipHostMallocDefault));
    // (fine-grained device memory for the pass table: the table is rewritten by host-to-device copies, and each pass
    // starts with a system-scope acquire, so no pass reads it through an L2 line the same memory held for an earlier,
    // freed buffer — measured: a fresh solver's passes once read the previous solver's table there)
    W3D_HIP(hipExtMallocWithFlags(reinterpret_cast<void**>(&push_dev_), tb, hipDeviceMallocFinegrained));
  }
  const std::vector<double> s = sin_table_ext(sch_.prob);
  W3D_HIP(hipMalloc(&d_s_, s.size() * sizeof(double)));
  W3D_HIP(hipMemcpy(d_s_, s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice));
  const i64 stage = imax(sch_.halo.packed_doubles, sch_.deep_max);
  if (stage > 0) {
    const i64 sstage = imax(stage, sch_.send_total);
    W3D_HIP(hipMalloc(&send_buf_, static_cast<size_t>(sstage) * sizeof(double)));
    W3D_HIP(hipMalloc(&recv_buf_, static_cast<size_t>(stage) * sizeof(double)));
    W3D_HIP(hipMemset(send_buf_, 0, static_cast<size_t>(sstage) * sizeof(double)));
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
  n_partials_ = std::max({n_full_, n_shell_ + n_int_, error_blocks(sch_.lay, sch_.full), n_fused_, n_deep,
                          sch_.opt.init2 ? init_two_partials(sch_.lay) : 0, 1});
  W3D_HIP(hipMalloc(&partials_, static_cast<size_t>(n_partials_) * sizeof(Partial)));
  // the LDS passes' partials live apart: their reductions are deferred, so the immediate users of partials_ (init,
  // single steps between passes) must not overwrite them
  if (n_tb_ > 0)
    W3D_HIP(hipMalloc(&tb_partials_, static_cast<size_t>(kTbRegions) * kTbLevels * kTbSlots * n_tb_ * sizeof(Partial)));
  W3D_HIP(hipMalloc(&errlog_, static_cast<size_t>(sch_.prob.K + 1) * sizeof(Partial)));
  W3D_HIP(hipMemset(errlog_, 0, static_cast<size_t>(sch_.prob.K + 1) * sizeof(Partial)));
  W3D_HIP(hipMalloc(&errall_, static_cast<size_t>(sch_.world) * (sch_.prob.K + 1) * sizeof(Partial)));
  ct_.resize(static_cast<size_t>(sch_.prob.K + 1));
  for (int n = 0; n <= sch_.prob.K; ++n) ct_[static_cast<size_t>(n)] = time_factor(sch_.prob, n);
  if (loopback_) sch_.opt.graph = false;  // (group ranks: the GpuGroup captures the whole group solve itself)
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
  for (double* p : {u_[0], u_[1], u_[2], u_[3], d_s_, send_buf_, recv_buf_, init_[0], init_[1]})
    if (p) (void)hipFree(p);
  if (energy_part_) (void)hipFree(energy_part_);
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
  return static_cast<size_t>(sch_.nbuf) * static_cast<size_t>(sch_.lay.bytes()) +
         static_cast<size_t>(imax(sch_.halo.packed_doubles, sch_.deep_max) + imax(sch_.halo.packed_doubles, sch_.send_total)) *
             sizeof(double) +
         static_cast<size_t>(n_partials_) * sizeof(Partial) + static_cast<size_t>(sch_.prob.N + 3) * sizeof(double) +
         static_cast<size_t>(kTbRegions) * kTbLevels * kTbSlots * static_cast<size_t>(n_tb_) * sizeof(Partial) +
         ((init_[0] ? 1u : 0u) + (init_[1] ? 1u : 0u)) * static_cast<size_t>(init_lay_.bytes()) +
         (energy_part_ ? static_cast<size_t>(energy_partials(sch_.lay) + 2) * sizeof(Partial) : 0u);
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
  int cur = 0;
  W3D_HIP(hipGetDevice(&cur));
  W3D_HIP(hipSetDevice(dev_));
  W3D_HIP(hipDeviceSynchronize());
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
  if (sch_.world == 1) energy_alloc();
  W3D_HIP(hipSetDevice(cur));
  initial_ = true;
  initial_runs_ = 0;
  resume_n_ = 0;
  resume_[0] = std::vector<double>();
  resume_[1] = std::vector<double>();
}

Partial GpuSolver::energy_sums(int which) const {
  W3D_REQUIRE(sch_.world == 1, "energy: one rank only (multi-rank: Solver.energy assembles the global fields)");
  W3D_REQUIRE(which == 0 || which == 1, "energy: which is 0 (E at K-1/2) or 1 (E at 1/2)");
  W3D_REQUIRE(runs_ > 0 && (!initial_ || initial_runs_ > 0), "energy: no solve has run yet");
  W3D_REQUIRE(which == 0 || initial_, "energy: E(1/2) is kept by solves that start from set_initial");
  int cur = 0;
  W3D_HIP(hipGetDevice(&cur));
  W3D_HIP(hipSetDevice(dev_));
  W3D_HIP(hipDeviceSynchronize());
  energy_alloc();
  const int n = energy_partials(sch_.lay);
  if (which == 0) {
    launch_energy(sch_.lay, coef_, sch_.prob.tau, u_[prev_buf_], u_[final_buf_], energy_part_, nullptr);
    launch_energy_reduce(energy_part_, n, energy_part_ + n, nullptr);
  }
  Partial h;
  W3D_HIP(hipMemcpy(&h, energy_part_ + n + which, sizeof h, hipMemcpyDeviceToHost));
  W3D_HIP(hipSetDevice(cur));
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
  if (sch_.push) {
    W3D_HIP(hipMemsetAsync(flags_ + 8, 0, sizeof(unsigned), s0_));  // workgroups done (the passes' signal counter)
    // (in-process group only: there every rank's init precedes every pass, so no neighbour has written yet)
    if (sch_.opt.poison_ghosts && loopback_) {
      W3D_HIP(hipMemsetAsync(stg_, 0xFF, static_cast<size_t>(8 * sch_.lay.xg * sch_.lay.plane) * sizeof(double), s0_));
      // ... except each staging plane's zero slot (Layout::zero_off), which positions outside the global interior load
      const size_t pb = static_cast<size_t>(sch_.lay.plane) * sizeof(double);
      W3D_HIP(hipMemset2DAsync(stg_ + sch_.lay.zero_off(), pb, 0, sizeof(double), static_cast<size_t>(8 * sch_.lay.xg), s0_));
    }
  }
  // one rank on the LDS kernel: the first pass starts from the analytic u⁰, u¹ itself (no init kernel, no reads)
  analytic_ = (sch_.mode == Mode::kFusedSingle || sch_.mode == Mode::kDeepTb) && sch_.analytic_ok() && resume_n_ == 0 &&
              !initial_;
  if (resume_n_ > 0) {  // loaded state: u^{n0−1} → buf 0, u^{n0} → buf 1 (ghosts included)
    const size_t bytes = static_cast<size_t>(sch_.lay.bytes());
    timed(kPhaseInit, s0_, [&] {
      W3D_HIP(hipMemcpyAsync(u_[0], resume_[0].data(), bytes, hipMemcpyHostToDevice, s0_));
      W3D_HIP(hipMemcpyAsync(u_[1], resume_[1].data(), bytes, hipMemcpyHostToDevice, s0_));
    });
    start_n_ = resume_n_;
  } else if (initial_) {  // user-supplied φ, ψ: u⁰ → buf 0, u¹ → buf 1 (ghosts included) from the device-resident copies
    timed(kPhaseInit, s0_, [&] {
      launch_first_step_field(sch_.lay, init_lay_, coef_, sch_.prob.tau, init_[0], init_[1], u_[0], u_[1], s0_);
    });
    timed(kPhaseCheck, s0_, [&] {
      if (energy_part_ && sch_.world == 1) {  // E^{1/2}, kept in its device slot
        const int ne = energy_partials(sch_.lay);
        launch_energy(sch_.lay, coef_, sch_.prob.tau, u_[0], u_[1], energy_part_, s0_);
        launch_energy_reduce(energy_part_, ne, energy_part_ + ne + 1, s0_);
      }
      if (is_check_[1]) {
        launch_error(sch_.lay, u_[1], sch_.full, s, ct_[1], partials_, s0_);
        launch_reduce(partials_, error_blocks(sch_.lay, sch_.full), errlog_ + 1, s0_);
      }
    });
    start_n_ = 1;
  } else if (analytic_) {
    start_n_ = 1;
  } else if (sch_.opt.init2 && K >= 2) {
    // u¹ -> buf 0, u² -> buf 1 analytically (no read pass), ghosts included; the first leapfrog step is n = 2
    timed(kPhaseInit, s0_, [&] {
      launch_init_two(sch_.lay, coef_, s, u_[0], u_[1], ct_[2], is_check_[2] ? partials_ : nullptr, s0_);
    });
    timed(kPhaseCheck, s0_, [&] {
      if (is_check_[2]) launch_reduce(partials_, init_two_partials(sch_.lay), errlog_ + 2, s0_);
      if (is_check_[1]) {
        launch_error(sch_.lay, u_[0], sch_.full, s, ct_[1], partials_, s0_);
        launch_reduce(partials_, error_blocks(sch_.lay, sch_.full), errlog_ + 1, s0_);
      }
    });
    start_n_ = 2;
  } else {
    timed(kPhaseInit, s0_, [&] { launch_init_first(sch_.lay, coef_, s, u_[0], u_[1], s0_); });
    timed(kPhaseCheck, s0_, [&] {
      if (is_check_[1]) {
        launch_error(sch_.lay, u_[1], sch_.full, s, ct_[1], partials_, s0_);
        launch_reduce(partials_, error_blocks(sch_.lay, sch_.full), errlog_ + 1, s0_);
      }
    });
    start_n_ = 1;
  }
  cur_ = 1;
  old_ = 0;
  units_ = plan_units(sch_, start_n_, analytic_);
  if (sch_.push) {  // every pass's push parameters, in device memory before the first pass reads them
    const int npass = static_cast<int>(units_.size());
    W3D_REQUIRE(npass <= sch_.prob.K, "push: more passes than steps");
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    W3D_HIP(hipStreamIsCapturing(s0_, &cs));
    push_tab_ = push_host_ + (cs == hipStreamCaptureStatusActive ? 0 : sch_.prob.K);
    for (int j = 1; j <= npass; ++j) push_tab_[j - 1] = make_push(j, npass);
    W3D_HIP(hipMemcpyAsync(push_dev_, push_tab_, static_cast<size_t>(npass) * sizeof(TbPush), hipMemcpyHostToDevice,
                           s0_));
  }
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
  if (sch_.opt.poison_ghosts && u.ghost_bits) poison(u, uf_, s0_, true);
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
                      ct_[static_cast<size_t>(nc)], chk ? partials_ : nullptr, sch_.opt.tiling, s0_);
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

PassArgs GpuSolver::tb_args(const UnitPlan& u) {
  PassArgs a;
  a.prev = u_[old_];
  a.cur = u_[cur_];
  a.out1 = u_[uf_[0]];
  a.out2 = u_[uf_[1]];
  a.d_s = d_s_ + 1;
  a.tiling = sch_.opt.tiling_tb;
  a.tiling.stages = u.steps;
  a.tiling.ghost_x1 = u.ghost_bits;
  for (int k = 1; k <= u.steps; ++k) {
    a.ct[k - 1] = ct_[static_cast<size_t>(u.n + k)];
    if (is_check_[static_cast<size_t>(u.n + k)]) a.check_mask |= 1 << (k - 1);
  }
  const int slots = sch_.mode == Mode::kDeepTb ? kTbSlots : 1;
  W3D_REQUIRE(tb_slots_ < slots, "leapfrog_tb: too many launches in one unit");
  if (a.check_mask) a.partials = tb_partials_ + tb_region_ * (kTbLevels * slots * n_tb_) + tb_slots_++ * n_tb_;
  // (every launch fills its whole slot of n_tb_ partials: shell and interior boxes may have fewer x chunks)
  a.level_stride = slots * n_tb_;
  a.grid_blocks = n_tb_;
  a.real = sch_.mode == Mode::kDeepTb ? sch_.sreal : tb_default_real();
  a.analytic_start = u.analytic;
  return a;
}

// One LDS S-step pass of unit u over `box` on stream st (s0 unless given). Its checked levels' partials go to slot
// tb_slots_ of each level: one slot per level on one rank, up to kTbSlots on multi-rank ranks (the shell boxes, then
// the interior), reduced together after the interior.
void GpuSolver::tb_pass(const UnitPlan& u, const LBox& box, int phase, hipStream_t st) {
  if (st == nullptr) st = s0_;
  PassArgs a = tb_args(u);
  // push transport: this pass's parameters (make_push) from the table phase_init uploaded; the command-processor
  // waits (push_cp_wait) are stream operations issued here, before the launch
  if (sch_.push) {
    a.push = push_tab_ + cur_unit_;
    a.push_dev = push_dev_ + cur_unit_;
    if (sch_.opt.push_cp_wait)
      for (int side = 0; side < 2; ++side)
        if (a.push->wait_side[side] && a.push->cp_wait > 0)
          W3D_HIP(hipStreamWaitValue32(s0_, flags_ + side, a.push->cp_wait, hipStreamWaitValueGte, 0xFFFFFFFFu));
  }
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
  if (sch_.mode == Mode::kDeep) {
    int off = 0;
    for (int n : n_dshell_) off += n;
    if (!sch_.dint.empty()) {
      timed(kPhaseCompute, s0_, [&] {
        launch_leapfrog2(sch_.lay, coef_, u_[old_], u_[cur_], u_[uf_[0]], u_[uf_[1]], sch_.dint, s, ct,
                         chk ? partials_ + off : nullptr, sch_.opt.tiling2, s0_, sch_.sx0, sch_.sx1);
      });
    }
    np = off + n_dint_;
  } else if ((sch_.mode == Mode::kFusedSingle && sch_.opt.tb && u.fused()) || sch_.mode == Mode::kDeepTb) {
    // S steps in one LDS pass (on slab ranks: the interior left between this unit's shells); every checked level
    // has its own block of partials
    if (sch_.mode != Mode::kDeepTb) tb_slots_ = 0;
    const LBox& b = u.interior;
    if (!b.empty()) tb_pass(u, b, kPhaseCompute);
    // (the shells ran on the side stream: join it before the reductions read their partials)
    if (wait) {
      capture::wait(s0_, ev_halo_);
      joined = true;
    }
    const int slots = sch_.mode == Mode::kDeepTb ? kTbSlots : 1;
    if (tb_slots_ > 0) {
      Partial* region = tb_partials_ + tb_region_ * (kTbLevels * slots * n_tb_);
      for (int k = 1; k <= u.steps; ++k)
        if (is_check_[static_cast<size_t>(u.n + k)])
          pending_.push_back(ReduceJob{region + (k - 1) * slots * n_tb_, tb_slots_ * n_tb_, errlog_ + u.n + k});
      tb_region_ = (tb_region_ + 1) % kTbRegions;
      if (tb_region_ == 0 || sch_.opt.timers) flush_reduces();  // the next unit reuses region 0 / per-unit check time
    }
  } else if (sch_.mode == Mode::kFusedSingle) {
    timed(kPhaseCompute, s0_, [&] {
      if (u.fused())
        launch_leapfrog2(sch_.lay, coef_, u_[old_], u_[cur_], u_[uf_[0]], u_[uf_[1]], sch_.full, s, ct,
                         chk ? partials_ : nullptr, sch_.opt.tiling2, s0_);
      else
        launch_leapfrog(sch_.lay, coef_, u_[cur_], u_[old_], &sch_.full, 1, s, ct, chk ? partials_ : nullptr, sch_.opt.tiling,
                        s0_);
    });
    np = u.fused() ? n_fused_ : n_full_;
  } else if (sch_.split()) {
    timed(kPhaseCompute, s0_, [&] {
      launch_leapfrog(sch_.lay, coef_, u_[cur_], u_[old_], &sch_.interior, 1, s, ct, chk ? partials_ + n_shell_ : nullptr,
                      sch_.opt.tiling, s0_);
    });
    np = n_shell_ + n_int_;
  } else {
    timed(kPhaseCompute, s0_, [&] {
      launch_leapfrog(sch_.lay, coef_, u_[cur_], u_[old_], &sch_.full, 1, s, ct, chk ? partials_ : nullptr, sch_.opt.tiling,
                      s0_);
    });
    np = n_full_;
  }
  if (wait && !joined) capture::wait(s0_, ev_halo_);
  if (chk && np > 0) timed(kPhaseCheck, s0_, [&] { launch_reduce(partials_, np, errlog_ + nc, s0_); });
  if (sch_.opt.debug_sync) W3D_HIP(hipDeviceSynchronize());
  if (u.fused()) {
    old_ = uf_[0];
    cur_ = uf_[1];
  } else {
    std::swap(cur_, old_);
  }
  final_buf_ = cur_;
  prev_buf_ = old_;
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
    if (!late) sch_.sdma ? unit_exchange_sdma(i) : unit_exchange_rccl(i);
    unit_interior(i);
    if (late) sch_.sdma ? unit_exchange_sdma(i) : unit_exchange_rccl(i);
  }
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
  const double n_int = static_cast<double>(sch_.prob.N - 1);
  const double denom = n_int * n_int * n_int;
  for (int n : check_steps()) {
    double m = 0.0, sum = 0.0;
    for (int q = 0; q < nsrc; ++q) {  // fixed rank order
      const Partial& v = host[static_cast<size_t>(q) * per + static_cast<size_t>(n)];
      m = v.x > m || std::isnan(v.x) ? v.x : m;
      sum += v.y;
    }
    r.steps.push_back(n);
    r.max_err.push_back(m);
    r.rms_err.push_back(std::sqrt(sum / denom));
    if (!std::isfinite(m) || !std::isfinite(sum)) r.finite = false;
  }
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
    hipGraph_t g = nullptr;
    bool ok = hipStreamBeginCapture(s0_, hipStreamCaptureModeThreadLocal) == hipSuccess;
    std::string thrown;
    if (ok) {
      capture::begin(s0_);  // (every cross-stream wait checked: wave3d/capture_guard.hpp)
      try {
        enqueue_solve();
        capture::finish();
      } catch (const std::exception& ex) {
        ok = false;
        thrown = ex.what();
        capture::close();
      }
      const hipError_t e = hipStreamEndCapture(s0_, &g);
      capture::abandon();
      ok = ok && e == hipSuccess && g != nullptr;
    }
    // (an error of the schedule itself is not a capture problem: report it instead of retrying eagerly on streams the
    // aborted capture may have left unusable)
    if (!thrown.empty()) {
      if (g) (void)hipGraphDestroy(g);
      fail("solve schedule failed while being captured: " + thrown);
    }
    if (ok) ok = hipGraphInstantiate(&gx, g, nullptr, nullptr, 0) == hipSuccess;
    // (upload now rather than at the first replay; the copy-engine runs still show one 9-12 ms solve among their first
    // 2-7 — never later — with or without it: profiles/r4/sdma_streams.md. bench.py warms copy-engine runs up longer)
    if (ok && hipGraphUpload(gx, s0_) != hipSuccess) {
      (void)hipGraphExecDestroy(gx);  // (instantiated but not uploadable: release it, run eagerly)
      ok = false;
    }
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    if (!ok) {
      gx = nullptr;
      sch_.opt.graph = false;
    }
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
  for (int i = 0; i < n; ++i) {
    RunResult r;
    decode_log(hbatch_ + static_cast<size_t>(i) * slot, nsrc, r);
    r.solve_s = dt;
    r.batched = true;
    out.push_back(std::move(r));
  }
  return out;
}

// ------------------------------------------------------------------------------------------------------------------
// push transport (slab LDS passes): peers, IPC, end of solve
// ------------------------------------------------------------------------------------------------------------------
// Pass j (1-based) of npass forwards its faces into the neighbours' staging of parity j % 2, reads its ghosts from its
// own staging of parity (j − 1) % 2 (pass 1: from the field, filled by the init / the loaded state), waits for both
// neighbours' pass j − 1 and signals its own. Epochs: in-kernel waits (graph-replayable) use the pass index j, every
// pass but the last signals (nobody waits for that one) and the flags are reset at the end of the solve, before its
// closing collective (which every multi-process run with in-kernel waits has: the error all-gather). Without a closing
// collective (push_no_collective) or with command-processor waits the epochs run on over the solves, every pass
// signals and pass 1 waits for the neighbours' last pass of the previous solve (no reset needed).
TbPush GpuSolver::make_push(int j, int npass) const {
  W3D_REQUIRE(peer_flags_[0] || !sch_.nb[0][0], "push transport: lower neighbour not connected");
  W3D_REQUIRE(peer_flags_[1] || !sch_.nb[0][1], "push transport: upper neighbour not connected");
  TbPush q;
  q.on = 1;
  q.faces_first = sch_.opt.overlap ? 1 : 0;
  q.T = static_cast<int>(sch_.lay.xg);
  q.nx = static_cast<int>(sch_.lay.nx);
  q.flags = flags_;
  q.status = flags_ + 4;
  q.done = flags_ + 8;
  const bool mono = sch_.opt.push_cp_wait || sch_.opt.push_no_collective;
  const unsigned G = static_cast<unsigned>(mono ? push_epoch_ + j : j);
  const unsigned wait = mono ? G - 1 : (j > 1 ? G - 1 : 0u);
  q.wait_epoch = sch_.opt.push_cp_wait ? 0u : wait;
  q.cp_wait = sch_.opt.push_cp_wait ? wait : 0u;
  q.signal_epoch = (mono || j < npass) ? G : 0u;
  q.done_target = q.signal_epoch ? static_cast<unsigned>(j * n_tb_) : 0u;
  static const unsigned long long ticks = [] {
    int khz = 100000;
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0);
    return static_cast<unsigned long long>(std::min(gpu_timeout_s(), 60.0) * 1e3 * khz);
  }();
  q.spin_ticks = ticks;
  // (tag: unique per solver instance, rank, solve and pass, so a table entry left by another solver never matches)
  static unsigned instances = 0;
  if (push_uid_ == 0) push_uid_ = ++instances;
  // (disjoint fields: the pass index in the low 16 bits, the solve epoch in the high 16, XORed with a hash of the
  // instance and rank — distinct (epoch, pass) pairs never share a tag within 65536 epochs)
  q.tag = ((push_uid_ * 2654435761u) ^ (static_cast<unsigned>(sch_.rank) * 40503u)) ^
          ((static_cast<unsigned>(push_epoch_) & 0xFFFFu) << 16) ^ (static_cast<unsigned>(j) & 0xFFFFu);
  const int par = j % 2, rpar = (j - 1) % 2;
  // (perf attribution of the transport with --fake-rank only: W3D_PUSH_ATTRIB=nofwd / noghost drop the forwarded
  // stores / the staging reads — the results are then wrong)
  const char* attrib = sch_.opt.fake_comm ? std::getenv("W3D_PUSH_ATTRIB") : nullptr;
  const bool nofwd = attrib && std::strstr(attrib, "nofwd"), noghost = attrib && std::strstr(attrib, "noghost");
  if (attrib && std::strstr(attrib, "noacq")) q.acquire = 0;
  if (attrib && std::strstr(attrib, "nosync")) q.wait_epoch = q.signal_epoch = q.done_target = 0;
  for (int side = 0; side < 2; ++side) {
    if (!(side == 0 ? sch_.nb[0][0] : sch_.nb[0][1])) continue;
    q.fwd1[side] = nofwd ? nullptr : peer_stg_[side] + stg_off(par, 0, 1 - side);  // the neighbour's ghosts facing us
    q.fwd2[side] = nofwd ? nullptr : peer_stg_[side] + stg_off(par, 1, 1 - side);
    if (j > 1 && !noghost) {
      q.gprev[side] = stg_ + stg_off(rpar, 0, side);
      q.gcur[side] = stg_ + stg_off(rpar, 1, side);
    }
    q.rflag[side] = peer_flags_[side] + (1 - side);  // our slot in the neighbour's flags
    q.wait_side[side] = 1;
  }
  return q;
}

std::string GpuSolver::push_handles() const {
  W3D_REQUIRE(sch_.push, "push_handles: this solver does not use the push transport");
  hipIpcMemHandle_t h[2];
  W3D_HIP(hipIpcGetMemHandle(&h[0], stg_));
  W3D_HIP(hipIpcGetMemHandle(&h[1], flags_));
  int dv[2] = {0, 0};  // this rank's device and the visible device count (peer-access check on the other side)
  W3D_HIP(hipGetDevice(&dv[0]));
  W3D_HIP(hipGetDeviceCount(&dv[1]));
  return std::string(reinterpret_cast<const char*>(h), sizeof h) + std::string(reinterpret_cast<const char*>(dv), sizeof dv);
}

void GpuSolver::connect_push_peer(int side, double* stg, unsigned* flags, bool ipc) {
  peer_stg_[side] = stg;
  peer_flags_[side] = flags;
  peer_ipc_[side] = ipc;
}

void GpuSolver::connect_push(const std::vector<std::string>& all) {
  W3D_REQUIRE(sch_.push, "connect_push: this solver does not use the push transport");
  W3D_REQUIRE(static_cast<int>(all.size()) == sch_.world, "connect_push: one handle set per rank expected");
  for (int side = 0; side < 2; ++side) {
    const int peer = neighbor_rank(sch_.dims, sch_.rank, 0, side);
    if (peer < 0) continue;
    const std::string& b = all[static_cast<size_t>(peer)];
    hipIpcMemHandle_t h[2];
    int dv[2] = {0, 0};
    W3D_REQUIRE(b.size() == sizeof h + sizeof dv, "connect_push: bad handle size from rank " + std::to_string(peer));
    std::memcpy(h, b.data(), sizeof h);
    std::memcpy(dv, b.data() + sizeof h, sizeof dv);
    // a neighbour on another GPU must be reachable by this GPU's stores (xGMI peer access), else the passes would
    // fault: refuse here, where the autotune can still drop the candidate
    int me = 0, nd = 0;
    W3D_HIP(hipGetDevice(&me));
    W3D_HIP(hipGetDeviceCount(&nd));
    if (dv[1] == nd && dv[0] != me) {
      int can = 0;
      W3D_HIP(hipDeviceCanAccessPeer(&can, me, dv[0]));
      W3D_REQUIRE(can, "push transport: GPU " + std::to_string(me) + " cannot access peer GPU " + std::to_string(dv[0]));
    }
    void* stg = nullptr;
    void* fl = nullptr;
    W3D_HIP(hipIpcOpenMemHandle(&stg, h[0], hipIpcMemLazyEnablePeerAccess));
    W3D_HIP(hipIpcOpenMemHandle(&fl, h[1], hipIpcMemLazyEnablePeerAccess));
    connect_push_peer(side, static_cast<double*>(stg), static_cast<unsigned*>(fl), true);
  }
}

void GpuSolver::connect_push_self() {
  W3D_REQUIRE(sch_.push, "connect_push_self: this solver does not use the push transport");
  for (int side = 0; side < 2; ++side)
    // (the signal raises peer_flags_[side] + (1 − side): aim it at flags_[side], the slot this side waits on)
    if (neighbor_rank(sch_.dims, sch_.rank, 0, side) >= 0) connect_push_peer(side, stg_, flags_ + (2 * side - 1), false);
}

// After the last pass of a solve (which waited for both neighbours' last signals, the final values of this solve's
// flags) the flags go back to 0, before this rank's end-of-solve collective: no neighbour can signal the next solve's
// first pass before that collective has completed everywhere.
void GpuSolver::push_finish(hipStream_t st) {
  if (!sch_.opt.push_cp_wait && !sch_.opt.push_no_collective) W3D_HIP(hipMemsetAsync(flags_, 0, 2 * sizeof(unsigned), st));
}

void GpuSolver::push_check() {
  if (!sch_.push) return;
  unsigned st = 0;
  W3D_HIP(hipMemcpy(&st, flags_ + 4, sizeof st, hipMemcpyDeviceToHost));
  W3D_REQUIRE(st != 2, "push transport: a pass read a stale parameter table (rank " + std::to_string(sch_.rank) + ")");
  W3D_REQUIRE(st == 0, "push transport: a pass timed out waiting for a neighbour's signal (rank " +
                           std::to_string(sch_.rank) + ")");
}

std::vector<double> GpuSolver::download(int which) const {
  std::vector<double> h(static_cast<size_t>(sch_.lay.total));
  const double* src = u_[which == 0 ? final_buf_ : prev_buf_];
  int cur = 0;
  W3D_HIP(hipGetDevice(&cur));
  W3D_HIP(hipSetDevice(dev_));
  W3D_HIP(hipDeviceSynchronize());
  W3D_HIP(hipMemcpy(h.data(), src, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  W3D_HIP(hipSetDevice(cur));
  return h;
}

unsigned long long GpuSolver::field_hash(int which) const {
  int cur = 0;
  W3D_HIP(hipGetDevice(&cur));
  W3D_HIP(hipSetDevice(dev_));
  W3D_HIP(hipDeviceSynchronize());
  unsigned long long* d = nullptr;
  W3D_HIP(hipMalloc(&d, sizeof(unsigned long long)));
  W3D_HIP(hipMemset(d, 0, sizeof(unsigned long long)));
  launch_field_hash(sch_.lay, u_[which == 0 ? final_buf_ : prev_buf_], d, nullptr);
  unsigned long long h = 0;
  W3D_HIP(hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost));
  W3D_HIP(hipFree(d));
  W3D_HIP(hipSetDevice(cur));
  return h;
}

}  // namespace wave3d

namespace wave3d {

double comm_allreduce(const Comm& c, double v, bool max_op) {
  static thread_local hipStream_t st = nullptr;
  static thread_local double* buf = nullptr;
  if (!st) {
    W3D_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    W3D_HIP(hipMalloc(&buf, sizeof(double)));
  }
  W3D_HIP(hipMemcpyAsync(buf, &v, sizeof(double), hipMemcpyHostToDevice, st));
  W3D_NCCL(ncclAllReduce(buf, buf, 1, ncclFloat64, max_op ? ncclMax : ncclSum, static_cast<ncclComm_t>(c.raw()), st));
  double out = 0.0;
  W3D_HIP(hipMemcpyAsync(&out, buf, sizeof(double), hipMemcpyDeviceToHost, st));
  wait_stream(st, &c, gpu_timeout_s());
  return out;
}

void comm_barrier(const Comm& c) { (void)comm_allreduce(c, 0.0, false); }

std::vector<std::string> comm_allgather_bytes(const Comm& c, const std::string& mine) {
  const size_t n = mine.size(), w = static_cast<size_t>(c.world());
  hipStream_t st = nullptr;
  W3D_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  char* d = nullptr;
  W3D_HIP(hipMalloc(&d, n * (w + 1)));
  std::string all(n * w, '\0');
  W3D_HIP(hipMemcpyAsync(d, mine.data(), n, hipMemcpyHostToDevice, st));
  W3D_NCCL(ncclAllGather(d, d + n, n, ncclChar, static_cast<ncclComm_t>(c.raw()), st));
  W3D_HIP(hipMemcpyAsync(all.data(), d + n, n * w, hipMemcpyDeviceToHost, st));
  wait_stream(st, &c, gpu_timeout_s());
  (void)hipFree(d);
  (void)hipStreamDestroy(st);
  std::vector<std::string> v;
  for (size_t r = 0; r < w; ++r) v.push_back(all.substr(r * n, n));
  return v;
}

int rccl_version() {
  int v = 0;
  (void)ncclGetVersion(&v);
  return v;
}

}  // namespace wave3d

namespace wave3d {

GpuGroup::GpuGroup(const Problem& prob, const SolverOptions& opt, int world, const std::string& transport)
    : transport_(transport) {
  W3D_REQUIRE(world >= 1, "world must be >= 1");
  W3D_REQUIRE(transport == "loopback" || transport == "rccl-self" || transport == "push" || transport == "sdma" ||
                  transport == "multi-device",
              "group transport must be loopback, rccl-self, push, sdma or multi-device, not " + transport);
  SolverOptions o = opt;
  if (transport == "multi-device") {
    // one rank per visible device, each with its rank of one communicator; the production GpuSolver (not a group
    // member): its own graph, RCCL exchanges and error-log all-gather; opt.sdma selects the copy engines between the
    // devices (peer pointers, peer access enabled), else RCCL
    multi_ = true;
    int ndev = 0, dev0 = 0;
    W3D_HIP(hipGetDeviceCount(&ndev));
    W3D_HIP(hipGetDevice(&dev0));
    W3D_REQUIRE(world <= ndev, "multi-device group: " + std::to_string(world) + " ranks but " + std::to_string(ndev) +
                                   " visible GPU(s)");
    const auto comms = Comm::init_all(world);
    for (int r = 0; r < world; ++r) {
      W3D_HIP(hipSetDevice(r));
      for (int q = 0; q < world && o.sdma; ++q)
        if (q != r) {
          int can = 0;
          W3D_HIP(hipDeviceCanAccessPeer(&can, r, q));
          W3D_REQUIRE(can, "multi-device sdma: GPU " + std::to_string(r) + " cannot access GPU " + std::to_string(q));
          const hipError_t e = hipDeviceEnablePeerAccess(q, 0);
          if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) W3D_HIP(e);
          (void)hipGetLastError();
        }
      ranks_.push_back(std::make_unique<GpuSolver>(prob, o, r, world, comms[static_cast<size_t>(r)], false));
    }
    if (o.sdma && world > 1)
      for (auto& sp : ranks_)
        for (GpuSolver::XLink& l : sp->xlinks_) {
          GpuSolver* q = ranks_[static_cast<size_t>(l.peer)].get();
          l.flags = q->xflags_;
          for (int b = 0; b < q->sch_.nbuf; ++b) l.u[b] = q->u_[b];
          l.recv = q->recv_buf_;
        }
    W3D_HIP(hipSetDevice(dev0));
    return;
  }
  o.push = transport == "push";
  o.sdma = transport == "sdma";
  for (int r = 0; r < world; ++r) {
    std::shared_ptr<Comm> c;
    if (transport == "rccl-self") c = std::make_shared<Comm>(0, 1, Comm::make_unique_id());
    ranks_.push_back(std::make_unique<GpuSolver>(prob, o, r, world, c, true));
  }
  if (o.push && world > 1) {
    // the ranks' passes wait for each other in the kernel: on ONE GPU they must not run concurrently (a waiting pass
    // could hold every CU while the pass it waits for cannot start), so every rank launches on rank 0's compute stream
    // in schedule order (rank 0 unit i, rank 1 unit i, ...) and each wait is already satisfied when it is reached.
    // The data path (forwarded faces in the neighbours' staging, ghosts read from the own staging, flags, counters,
    // epochs, flag reset) is the multi-process one; peers are the other ranks' buffers instead of IPC mappings.
    for (int r = 0; r < world; ++r) {
      GpuSolver* s = ranks_[static_cast<size_t>(r)].get();
      W3D_REQUIRE(s->sch_.push, "push group: every rank must run the slab LDS passes (deep-tb)");
      if (r > 0) {
        (void)hipStreamDestroy(s->s0_);
        s->s0_ = ranks_[0]->s0_;
        s->own_s0_ = false;
      }
      for (int side = 0; side < 2; ++side) {
        const int peer = neighbor_rank(s->sch_.dims, r, 0, side);
        if (peer < 0) continue;
        GpuSolver* q = ranks_[static_cast<size_t>(peer)].get();
        s->connect_push_peer(side, q->stg_, q->flags_, false);
      }
    }
  }
  if (o.sdma && world > 1) {
    // copy-engine ranks in one process: every link points at the peer rank's own buffers and flag words (no IPC)
    for (auto& sp : ranks_) {
      GpuSolver* s = sp.get();
      W3D_REQUIRE(s->sch_.sdma, "sdma group: every rank must run the LDS multi-step passes (deep-tb)");
      for (GpuSolver::XLink& l : s->xlinks_) {
        GpuSolver* q = ranks_[static_cast<size_t>(l.peer)].get();
        l.flags = q->xflags_;
        for (int b = 0; b < q->sch_.nbuf; ++b) l.u[b] = q->u_[b];
        l.recv = q->recv_buf_;
      }
    }
  }
  // (sdma: the flag waits of one rank's stream are released by other ranks' streams, so the group enqueues eagerly in
  // an order where every wait is issued after the write it waits for — see enqueue)
  graph_ = opt.graph && !opt.timers && !opt.debug_sync && (world == 1 || multistream_capture_safe()) && !o.sdma;
  graph0_ = graph_;
  W3D_HIP(hipStreamCreateWithFlags(&gs_, hipStreamNonBlocking));
  W3D_HIP(hipEventCreateWithFlags(&fork_, hipEventDisableTiming));
  W3D_HIP(hipEventCreateWithFlags(&all_packed_, hipEventDisableTiming));
  W3D_HIP(hipEventCreateWithFlags(&all_pulled_, hipEventDisableTiming));
  join_.resize(2 * static_cast<size_t>(world));
  for (hipEvent_t& e : join_) W3D_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}

GpuGroup::~GpuGroup() {
  if (multi_) {  // (each rank's resources on its own device)
    for (auto& r : ranks_) {
      (void)hipSetDevice(r->device());
      r.reset();
    }
    return;
  }
  if (exec_) (void)hipGraphExecDestroy(exec_);
  for (hipEvent_t e : join_) (void)hipEventDestroy(e);
  for (hipEvent_t e : {fork_, all_packed_, all_pulled_})
    if (e) (void)hipEventDestroy(e);
  if (gs_) (void)hipStreamDestroy(gs_);
}

void GpuGroup::set_state(const double* prev, const double* cur, int n0) {
  for (auto& r : ranks_) r->set_state(prev, cur, n0);
  graph_ = false;  // (the state upload is a pageable host copy: eager runs)
}

void GpuGroup::set_initial(const double* phi, const double* psi) {
  int cur = 0;
  W3D_HIP(hipGetDevice(&cur));
  for (auto& r : ranks_) r->set_initial(phi, psi);
  W3D_HIP(hipSetDevice(cur));
  if (multi_) return;  // (every rank captures its own solve)
  // nothing host-side per solve: the group solve is captured again, with the first-step kernels in it
  if (exec_) W3D_HIP(hipGraphExecDestroy(exec_));
  exec_ = nullptr;
  graph_ = graph0_;
}

std::vector<int> GpuGroup::comm_counts() const {
  std::vector<int> v;
  for (const auto& r : ranks_)
    if (r->comm_) v.push_back(r->comm_->count());
  return v;
}

// Every rank's schedule, interleaved unit by unit exactly as the ranks of a multi-process run would issue them.
void GpuGroup::enqueue() {
  std::vector<GpuSolver*> rs;
  for (auto& p : ranks_) rs.push_back(p.get());
  const bool dbg = std::getenv("W3D_DEBUG") != nullptr;
  auto step = [&](const char* what, int i) {
    if (dbg) std::fprintf(stderr, "[group] unit %d %s\n", i, what);
  };
  for (auto* s : rs) {
    s->xpar_ = static_cast<int>(s->xsolves_ & 1);
    s->phase_init();
    s->tb_region_ = 0;
    s->pending_.clear();
  }
  step("init", -1);
  const int nu = static_cast<int>(rs[0]->units_.size());
  const bool late = rs[0]->sch_.late_exchange();
  if (rs[0]->sch_.sdma) {
    // copy-engine group: each rank runs its own production schedule; the phases are issued rank by rank so that every
    // flag wait reaches its HIP queue after the write that releases it (streams of one process may share a hardware
    // queue, where a wait issued first would block the write behind it): all receives (done(i − 1) writes) of unit i
    // before any exchange i (which waits for them), every exchange i − 1 ("arrived" writes) before the receives of unit i
    for (int i = 0; i < nu; ++i) {
      for (auto* s : rs) s->sdma_receive(i);
      for (auto* s : rs) {
        s->unit_shell(i);
        if (!late) s->unit_exchange_sdma(i);
        s->unit_interior(i);
        if (late) s->unit_exchange_sdma(i);
      }
      step("unit", i);
    }
    for (auto* s : rs) {
      s->flush_reduces();
      s->sdma_finish();
      ++s->xsolves_;
    }
    return;
  }
  for (int i = 0; i < nu; ++i) {
    for (auto* s : rs) s->unit_shell(i);
    step("shell", i);
    if (late)
      for (auto* s : rs) s->unit_interior(i);
    // Cross-rank ordering goes through the group stream: it joins every rank's "packed" event, and every puller
    // waits on the join (likewise "pulled" before anyone overwrites its send regions). Direct waits of one rank's
    // stream on a PEER's side-stream event are avoided on purpose: HIP 7.2 crashes in hipStreamEndCapture on such
    // sibling-to-sibling waits (tools/probes/capture_probe2.hip, flag 1); fork/join through the origin captures fine.
    for (auto* s : rs) s->lb_pack(i);
    step("pack", i);
    bool any = false;
    for (auto* s : rs)
      if (s->needs_exchange(i)) {
        capture::wait(gs_, s->ev_packed_);
        any = true;
      }
    if (any) capture::record(all_packed_, gs_);
    for (auto* s : rs) s->lb_pull(i, rs, all_packed_);
    step("pull", i);
    for (auto* s : rs)
      if (s->needs_exchange(i)) capture::wait(gs_, s->ev_halo_);
    if (any) capture::record(all_pulled_, gs_);
    for (auto* s : rs) s->lb_fence(i, all_pulled_);
    step("fence", i);
    if (!late)
      for (auto* s : rs) s->unit_interior(i);
    step("interior", i);
  }
  for (auto* s : rs) s->flush_reduces();
  for (auto* s : rs)
    if (s->sch_.push) {
      s->push_finish(s->s0_);
      s->push_epoch_ += nu;
    }
  step("flush", nu);
}

// the group stream waits for every stream the ranks used
void GpuGroup::join() {
  for (size_t q = 0; q < ranks_.size(); ++q) {
    GpuSolver* s = ranks_[q].get();
    capture::record(join_[2 * q], s->s0_);
    capture::wait(gs_, join_[2 * q]);
    if (s->xstream() != s->s0_) {
      capture::record(join_[2 * q + 1], s->s1_);
      capture::wait(gs_, join_[2 * q + 1]);
    }
  }
}

RunResult GpuGroup::run() {
  if (multi_) {
    // every rank's production solve on its own thread and device, concurrently (RCCL's collectives and send/recv
    // pairs need every rank's call in flight); each rank's log is the global one (all-gathered), rank 0's is returned
    std::vector<RunResult> out(ranks_.size());
    std::vector<std::string> err(ranks_.size());
    std::vector<std::thread> th;
    const double t0 = now_s();
    for (size_t r = 0; r < ranks_.size(); ++r)
      th.emplace_back([&, r] {
        try {
          W3D_HIP(hipSetDevice(ranks_[r]->device()));
          out[r] = ranks_[r]->run();
        } catch (const std::exception& e) {
          err[r] = e.what();
        }
      });
    for (auto& t : th) t.join();
    for (size_t r = 0; r < ranks_.size(); ++r)
      W3D_REQUIRE(err[r].empty(), "multi-device rank " + std::to_string(r) + ": " + err[r]);
    for (size_t r = 1; r < ranks_.size(); ++r)
      W3D_REQUIRE(out[r].max_err == out[0].max_err, "multi-device: ranks gathered different error logs");
    RunResult r = out[0];
    r.solve_s = now_s() - t0;
    ++runs_;
    return r;
  }
  std::vector<GpuSolver*> rs;
  for (auto& p : ranks_) rs.push_back(p.get());
  const int K = rs[0]->sch_.prob.K;
  // capture on the second run (RCCL connects its peers eagerly on the first send/recv, never inside a capture): the
  // group stream forks into every rank's two streams and joins them back, so the graph holds all ranks' work
  const bool dbg = std::getenv("W3D_DEBUG") != nullptr;
  auto trace = [&](const char* what) {
    if (dbg) {
      (void)hipDeviceSynchronize();
      std::fprintf(stderr, "[group] %s: %s\n", what, hipGetErrorString(hipGetLastError()));
    }
  };
  if (graph_ && !exec_ && runs_ >= 1) {
    hipGraph_t g = nullptr;
    bool ok = hipStreamBeginCapture(gs_, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (dbg) std::fprintf(stderr, "[group] begin capture ok=%d\n", ok ? 1 : 0);
    if (ok) {
      capture::begin(gs_);
      try {
        capture::record(fork_, gs_);
        for (auto* s : rs) {
          capture::wait(s->s0_, fork_);
          if (s->xstream() != s->s0_) capture::wait(s->s1_, fork_);
        }
        enqueue();
        join();
        capture::finish();
      } catch (const std::exception& ex) {
        if (dbg) std::fprintf(stderr, "[group] capture enqueue failed: %s\n", ex.what());
        ok = false;
        capture::close();
      }
      const hipError_t e = hipStreamEndCapture(gs_, &g);
      capture::abandon();
      if (dbg) std::fprintf(stderr, "[group] end capture: %s graph=%p\n", hipGetErrorString(e), (void*)g);
      ok = ok && e == hipSuccess && g != nullptr;
    }
    if (ok) {
      const hipError_t e = hipGraphInstantiate(&exec_, g, nullptr, nullptr, 0);
      if (dbg) std::fprintf(stderr, "[group] instantiate: %s\n", hipGetErrorString(e));
      ok = e == hipSuccess;
      if (ok && hipGraphUpload(exec_, gs_) != hipSuccess) {  // (see GpuSolver::run)
        (void)hipGraphExecDestroy(exec_);
        ok = false;
      }
    }
    if (g) (void)hipGraphDestroy(g);
    (void)hipGetLastError();
    if (!ok) {
      exec_ = nullptr;
      graph_ = false;
    }
  }
  const double t0 = now_s();
  if (exec_ && graph_) {
    W3D_HIP(hipGraphLaunch(exec_, gs_));
    trace("graph launch");
  } else {
    enqueue();
    join();  // the gathers below run on the group stream
  }
  // per-rank error logs to the host: through ncclAllGather on each rank's communicator (rccl-self; one rank each, so
  // the gathered log is the rank's own) or straight from errlog_; combined in rank order as the multi-process
  // all-gather is
  const size_t per = static_cast<size_t>(K + 1);
  std::vector<Partial> all(per * rs.size());
  for (size_t q = 0; q < rs.size(); ++q) {
    GpuSolver* s = rs[q];
    const Partial* src = s->errlog_;
    if (s->comm_) {
      W3D_NCCL(ncclAllGather(s->errlog_, s->errall_, 2 * per, ncclFloat64, static_cast<ncclComm_t>(s->comm_->raw()),
                             gs_));
      src = s->errall_;
    }
    W3D_HIP(hipMemcpyAsync(all.data() + q * per, src, per * sizeof(Partial), hipMemcpyDeviceToHost, gs_));
  }
  trace("gathers");
  wait_stream(gs_, rs[0]->comm_.get(), gpu_timeout_s());
  for (auto* s : rs) {
    if (s->comm_) s->comm_->check_async();
    s->push_check();
  }
  RunResult r;
  for (size_t q = 0; q < rs.size(); ++q)
    W3D_REQUIRE(!rs[q]->sch_.sdma || all[q * per].x == 0.0,
                "sdma transport: a flag wait timed out on rank " + std::to_string(q));
  const double n_int = static_cast<double>(rs[0]->sch_.prob.N - 1);
  for (int n : rs[0]->check_steps()) {
    double m = 0.0, sum = 0.0;
    for (size_t q = 0; q < rs.size(); ++q) {
      const Partial& v = all[q * per + static_cast<size_t>(n)];
      m = v.x > m || std::isnan(v.x) ? v.x : m;
      sum += v.y;
    }
    r.steps.push_back(n);
    r.max_err.push_back(m);
    r.rms_err.push_back(std::sqrt(sum / (n_int * n_int * n_int)));
    if (!std::isfinite(m) || !std::isfinite(sum)) r.finite = false;
  }
  r.solve_s = now_s() - t0;
  rs[0]->collect_phases(r);  // (timers: rank 0's phases, as the CLI reports)
  ++runs_;
  return r;
}

}  // namespace wave3d
