// GpuGroup: the ranks of one decomposition inside one process. See wave3d/solver.hpp.
#include <cstdio>
#include <thread>

#include "solver_internal.hpp"
#include "wave3d/capture_guard.hpp"

namespace wave3d {

GpuGroup::GpuGroup(const Problem& prob, const SolverOptions& opt, int world, const std::string& transport)
    : transport_(transport) {
  W3D_REQUIRE(world >= 1, "world must be >= 1");
  W3D_REQUIRE(prob.order == 2, "order: order = 4 runs on one GPU rank only, not in a GpuGroup (the stencil needs ghosts two "
                               "deep per step)");
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
    if (o.sdma && world > 1) wire_sdma();
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
    for (auto& sp : ranks_)
      W3D_REQUIRE(sp->sch_.sdma, "sdma group: every rank must run the LDS multi-step passes (deep-tb)");
    wire_sdma();
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

// copy-engine ranks in one process: every link points at the peer rank's own buffers and flag words (no IPC)
void GpuGroup::wire_sdma() {
  for (auto& sp : ranks_)
    for (GpuSolver::XLink& l : sp->xlinks_) {
      GpuSolver* q = ranks_[static_cast<size_t>(l.peer)].get();
      l.flags = q->xflags_;
      for (int b = 0; b < q->sch_.nbuf; ++b) l.u[b] = q->u_[b];
      l.recv = q->recv_buf_;
    }
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
  {
    DeviceScope scope(ranks_[0]->device());
    for (auto& r : ranks_) r->set_initial(phi, psi);
  }
  if (multi_) return;  // (every rank captures its own solve)
  // nothing host-side per solve: the group solve is captured again, with the first-step kernels in it
  if (exec_) W3D_HIP(hipGraphExecDestroy(exec_));
  exec_ = nullptr;
  graph_ = graph0_;
}

void GpuGroup::set_receivers(const i64* ijk, int R) {
  for (auto& r : ranks_) {
    DeviceScope scope(r->device());
    r->set_receivers(ijk, R);
  }
  n_recv_ = R;
  if (multi_) return;  // (every rank captures its own solve)
  if (exec_) W3D_HIP(hipGraphExecDestroy(exec_));
  exec_ = nullptr;  // (graph_ stays as it is: the record launches are device work like any other)
}

void GpuGroup::set_sources(const i64* ijk, int Q, const double* w) {
  W3D_REQUIRE(Q == 0 || !multi_, "sources: not on a multi-device group (its ranks solve on their own threads over RCCL; "
                                 "use a loopback or rccl-self group)");
  for (auto& r : ranks_) {
    DeviceScope scope(r->device());
    r->set_sources(ijk, Q, w);
  }
  if (multi_) return;
  if (exec_) W3D_HIP(hipGraphExecDestroy(exec_));
  exec_ = nullptr;  // (graph_ stays as it is: the corrections are device work like any other)
}

std::vector<double> GpuGroup::traces() const {
  W3D_REQUIRE(n_recv_ > 0, "traces: no receivers are set (set_receivers)");
  const size_t rows = static_cast<size_t>(ranks_[0]->sch_.prob.K + 1), R = static_cast<size_t>(n_recv_);
  std::vector<double> all(rows * R);
  std::vector<char> seen(R, 0);
  for (const auto& r : ranks_) {
    const GpuSolver::Traces t = r->traces();
    const size_t own = t.slots.size();
    for (size_t k = 0; k < own; ++k) {
      const size_t slot = static_cast<size_t>(t.slots[k]);
      W3D_REQUIRE(slot < R && !seen[slot], "traces: a receiver is owned by two ranks");
      seen[slot] = 1;
      for (size_t n = 0; n < rows; ++n) all[n * R + slot] = t.values[n * own + k];
    }
  }
  for (char s : seen) W3D_REQUIRE(s, "traces: a receiver is owned by no rank");
  return all;
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
  for (auto* s : rs) s->source_finish();
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
  const bool dbg = std::getenv("W3D_DEBUG") != nullptr;
  auto trace = [&](const char* what) {
    if (dbg) {
      (void)hipDeviceSynchronize();
      std::fprintf(stderr, "[group] %s: %s\n", what, hipGetErrorString(hipGetLastError()));
    }
  };
  // capture on the second run (RCCL connects its peers eagerly on the first send/recv, never inside a capture): the
  // group stream forks into every rank's two streams and joins them back, so the graph holds all ranks' work. Any
  // failure, a throwing schedule included: eager runs from here on
  if (graph_ && !exec_ && runs_ >= 1) {
    auto forked = [&] {
      capture::record(fork_, gs_);
      for (auto* s : rs) {
        capture::wait(s->s0_, fork_);
        if (s->xstream() != s->s0_) capture::wait(s->s1_, fork_);
      }
      enqueue();
      join();
    };
    std::string thrown;
    exec_ = capture::graph(gs_, forked, &thrown);
    if (!exec_) graph_ = false;
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
    s->solve_done();
  }
  RunResult r;
  rs[0]->decode_log(all.data(), static_cast<int>(rs.size()), r);  // (every rank has the same schedule and check steps)
  r.solve_s = now_s() - t0;
  rs[0]->collect_phases(r);  // (timers: rank 0's phases, as the CLI reports)
  ++runs_;
  return r;
}

}  // namespace wave3d
