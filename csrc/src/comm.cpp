// RCCL communicator wrapper and the blocking host collectives over it. See wave3d/solver.hpp.
#include <cstring>

#include "solver_internal.hpp"

namespace wave3d {

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
