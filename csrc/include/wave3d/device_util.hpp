// Device helpers that every kernel file used to copy: the 16-byte pair, the wave reduction of an error partial, the block
// error epilogue of the tiled single-step kernels, and the launch-error check of the host launchers.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "wave3d/common.hpp"

#define W3D_HIP_CHECK(expr)                                                                          \
  do {                                                                                               \
    hipError_t _e = (expr);                                                                          \
    if (_e != hipSuccess) ::wave3d::fail(std::string(#expr) + ": " + hipGetErrorString(_e));          \
  } while (0)

namespace wave3d {

using v2d = double __attribute__((ext_vector_type(2)));  // one pair: two consecutive z nodes, 16 bytes

constexpr int kLanes = 64;

__device__ __forceinline__ v2d ld2(const double* p) { return *reinterpret_cast<const v2d*>(p); }

template <bool NT>
__device__ __forceinline__ void st2(double* p, v2d v) {
  if (NT)
    __builtin_nontemporal_store(v, reinterpret_cast<v2d*>(p));
  else
    *reinterpret_cast<v2d*>(p) = v;
}

__device__ __forceinline__ v2d neg2(v2d v) {
  v2d r;
  r.x = -v.x;
  r.y = -v.y;
  return r;
}

// (max, sum) of an error partial over the wave, in every lane
__device__ __forceinline__ void wave_reduce(double& m, double& s) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double om = __shfl_xor(m, o, 64);
    const double os = __shfl_xor(s, o, 64);
    m = om > m ? om : m;
    s = s + os;
  }
}

// The check epilogue of a (TY rows × 64 lanes) workgroup whose waves are its rows: every thread's (emax, esum) is folded
// per wave, then thread 0 folds the TY rows in row order into partials[blockIdx.x] (Partial, kernels.hpp). Every thread
// of the workgroup calls it.
template <int TY>
__device__ __forceinline__ void block_error_store(double emax, double esum, int lane, int row, int tid, double2* partials) {
  __shared__ double red_m[TY], red_s[TY];
  wave_reduce(emax, esum);
  if (lane == 0) {
    red_m[row] = emax;
    red_s[row] = esum;
  }
  __syncthreads();
  if (tid == 0) {
    double m = red_m[0], s = red_s[0];
    for (int r = 1; r < TY; ++r) {
      m = red_m[r] > m ? red_m[r] : m;
      s += red_s[r];
    }
    partials[blockIdx.x] = make_double2(m, s);
  }
}

}  // namespace wave3d
