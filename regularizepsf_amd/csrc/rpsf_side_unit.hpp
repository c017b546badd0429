// rpsf_side_unit.hpp - what every host-side unit of the library shares: the error plumbing (the one text of fail / HIP_TRY; the
// message itself lives in rpsf.hip), and for the side units (csrc/builder.hip, csrc/stars.hip, csrc/saturation.hip, csrc/convert.hip,
// csrc/scale.hip) the workgroup context their core headers' drivers run in on the GPU, launch arithmetic, a device array that grows
// and the narrowing upload of a host frame.  Everything here but rpsf_detail_fail has internal linkage: each unit gets its own.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/rpsf.h"

// functions that cross unit boundaries inside the library: never exported
#define RPSF_HIDDEN __attribute__((visibility("hidden")))

RPSF_HIDDEN int rpsf_detail_fail(int code, const std::string& msg);  // rpsf.hip: sets rpsf_last_error of the calling thread
static inline int fail(int code, const std::string& msg) { return rpsf_detail_fail(code, msg); }
// stars.hip: what another unit may know of a model handle (builder.hip draws the neighbours of kernel B1n from it); the values stay the model's
RPSF_HIDDEN void rpsf_detail_stars_model_view(const rpsf_stars_model* model, int* device, int* n_cells, int* N, const double** values_dev);
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

// Scratch that is kept between calls and re-sized by the largest one so far (DevBuf, rpsf_plan.hpp: one allocation of an exact size, owned by a handle)
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

// A host frame of `npix` pixels into `frame_dev`: it crosses PCIe once, as float32 - what every apply path of the library uploads
inline int upload_frame_f32(float* frame_dev, const void* image_host, int image_is_f64, size_t npix) {
  if (image_is_f64) {
    std::vector<float> narrow(npix);
    const double* src = static_cast<const double*>(image_host);
    for (size_t i = 0; i < npix; ++i) narrow[i] = (float)src[i];
    HIP_TRY(hipMemcpy(frame_dev, narrow.data(), npix * sizeof(float), hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemcpy(frame_dev, image_host, npix * sizeof(float), hipMemcpyHostToDevice));
  }
  return RPSF_OK;
}
}  // namespace
