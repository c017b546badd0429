// rpsf_side_unit.hpp - what the side units of the library (csrc/builder.hip, csrc/stars.hip, csrc/saturation.hip) share: errors
// reported through rpsf.hip, the workgroup context their core headers' drivers run in on the GPU, launch arithmetic and a device
// array that grows.  Everything here has internal linkage: each unit gets its own.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/rpsf.h"

int rpsf_detail_fail(int code, const std::string& msg);  // rpsf.hip: sets rpsf_last_error of the calling thread
static inline int fail(int code, const std::string& msg) { return rpsf_detail_fail(code, msg); }
#define HIP_TRY(expr)                                                                                               \
  do {                                                                                                              \
    hipError_t e_ = (expr);                                                                                         \
    if (e_ != hipSuccess)                                                                                           \
      return fail(e_ == hipErrorOutOfMemory ? RPSF_E_NOMEM : RPSF_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace {
struct GpuCtx {
  template <class F>
  __device__ __forceinline__ void each(F&& f) {
    f((int)threadIdx.x);
    __syncthreads();
  }
};
__device__ __forceinline__ long global_id() { return (long)blockIdx.x * blockDim.x + threadIdx.x; }
inline unsigned blocks_for(long threads) { return (unsigned)((threads + 255) / 256); }

template <class T>
struct Buf {  // a device array that only ever grows
  T* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t count) {
    if (count <= cap) return hipSuccess;
    if (p) {  // (nothing of an earlier call may still be running on the old array)
      (void)hipDeviceSynchronize();
      (void)hipFree(p);
    }
    p = nullptr, cap = 0;
    const hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e == hipSuccess) cap = count;
    return e;
  }
  ~Buf() {
    if (p) (void)hipFree(p);
  }
};
}  // namespace
