// What the GPU runtime's translation units share and nothing outside them needs (comm.cpp, solver_gpu.cpp,
// transport_push.cpp, gpu_group.cpp).
#pragma once

#include <rccl/rccl.h>

#include <chrono>
#include <cstdlib>
#include <string>
#include <thread>

#include "wave3d/solver.hpp"

namespace wave3d {

#define W3D_NCCL(expr)                                                                               \
  do {                                                                                               \
    ncclResult_t _r = (expr);                                                                        \
    if (_r != ncclSuccess) ::wave3d::fail(std::string(#expr) + ": " + ncclGetErrorString(_r));        \
  } while (0)

inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Upper bound for one blocking wait on the GPU (env W3D_TIMEOUT_S, default 300 s): a lost peer or a stuck halo
// exchange turns into an error instead of a hang.
inline double gpu_timeout_s() {
  static const double t = [] {
    const char* v = std::getenv("W3D_TIMEOUT_S");
    const double x = v ? std::atof(v) : 0.0;
    return x > 0.0 ? x : 300.0;
  }();
  return t;
}

// Wait for a stream while polling RCCL for asynchronous failures (a dead peer must not hang the job forever).
inline void wait_stream(hipStream_t s, const Comm* comm, double timeout_s) {
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

// Makes `dev` the current device (sync: and waits for all its work) for the enclosing scope, then puts the caller's
// device back. The restore cannot throw from a destructor: its error is dropped.
class DeviceScope {
 public:
  explicit DeviceScope(int dev, bool sync = false) {
    W3D_HIP(hipGetDevice(&prev_));
    W3D_HIP(hipSetDevice(dev));
    if (sync) W3D_HIP(hipDeviceSynchronize());
  }
  ~DeviceScope() { (void)hipSetDevice(prev_); }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;

 private:
  int prev_ = 0;
};

}  // namespace wave3d
