// Push halo transport of the slab LDS passes: peers, IPC, per-solve setup, end of solve. See wave3d/solver.hpp.
//
// Pass j (1-based) of npass forwards its faces into the neighbours' staging of parity j % 2, reads its ghosts from its
// own staging of parity (j − 1) % 2 (pass 1: from the field, filled by the init / the loaded state), waits for both
// neighbours' pass j − 1 and signals its own. Epochs: in-kernel waits (graph-replayable) use the pass index j, every
// pass but the last signals (nobody waits for that one) and the flags are reset at the end of the solve, before its
// closing collective (which every multi-process run with in-kernel waits has: the error all-gather). Without a closing
// collective (push_no_collective) or with command-processor waits the epochs run on over the solves, every pass
// signals and pass 1 waits for the neighbours' last pass of the previous solve (no reset needed).
#include <algorithm>
#include <cstring>

#include "solver_internal.hpp"

namespace wave3d {

void GpuSolver::push_alloc() {
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

void GpuSolver::push_begin_solve() {
  W3D_HIP(hipMemsetAsync(flags_ + 8, 0, sizeof(unsigned), s0_));  // workgroups done (the passes' signal counter)
  // (in-process group only: there every rank's init precedes every pass, so no neighbour has written yet)
  if (sch_.opt.poison_ghosts && loopback_) {
    W3D_HIP(hipMemsetAsync(stg_, 0xFF, static_cast<size_t>(8 * sch_.lay.xg * sch_.lay.plane) * sizeof(double), s0_));
    // ... except each staging plane's zero slot (Layout::zero_off), which positions outside the global interior load
    const size_t pb = static_cast<size_t>(sch_.lay.plane) * sizeof(double);
    W3D_HIP(hipMemset2DAsync(stg_ + sch_.lay.zero_off(), pb, 0, sizeof(double), static_cast<size_t>(8 * sch_.lay.xg), s0_));
  }
}

// every pass's push parameters, in device memory before the first pass reads them
void GpuSolver::push_upload() {
  const int npass = static_cast<int>(units_.size());
  W3D_REQUIRE(npass <= sch_.prob.K, "push: more passes than steps");
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  W3D_HIP(hipStreamIsCapturing(s0_, &cs));
  push_tab_ = push_host_ + (cs == hipStreamCaptureStatusActive ? 0 : sch_.prob.K);
  for (int j = 1; j <= npass; ++j) push_tab_[j - 1] = make_push(j, npass);
  W3D_HIP(hipMemcpyAsync(push_dev_, push_tab_, static_cast<size_t>(npass) * sizeof(TbPush), hipMemcpyHostToDevice,
                         s0_));
}

// this pass's parameters (make_push) from the table push_upload sent; the command-processor waits (push_cp_wait) are
// stream operations issued here, before the launch
void GpuSolver::push_pass_args(PassArgs& a) {
  a.push = push_tab_ + cur_unit_;
  a.push_dev = push_dev_ + cur_unit_;
  if (sch_.opt.push_cp_wait)
    for (int side = 0; side < 2; ++side)
      if (a.push->wait_side[side] && a.push->cp_wait > 0)
        W3D_HIP(hipStreamWaitValue32(s0_, flags_ + side, a.push->cp_wait, hipStreamWaitValueGte, 0xFFFFFFFFu));
}

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

}  // namespace wave3d
