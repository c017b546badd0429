// rpsf_kernels_shard.hpp - the plain kernel of the sharded row-band step: K4.  Defined in exactly one unit, the one that launches it:
// csrc/rpsf_shard.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

// ------------------------------------------------------------------------------------------------
// K4: accum[i] += src[i]
// ------------------------------------------------------------------------------------------------
// (grid-stride: a caller that runs it beside a persistent patch launch gives it a handful of workgroups, so that it lives on the CUs that
// launch leaves free instead of spreading a thousand small workgroups over CUs the patch workgroups are waiting for)
// The 16-byte body only where both addresses are multiples of 16 bytes: the sharded step hands over pointers rows x width floats into an
// allocation, which at a width that is no multiple of 4 are aligned to 4 bytes and no more.  Those callers get the same elements one by one.
__global__ void add_rows_kernel(float* __restrict__ accum, const float* __restrict__ src, size_t count) {
  const size_t step = (size_t)gridDim.x * blockDim.x * 4;
  if (((reinterpret_cast<uintptr_t>(accum) | reinterpret_cast<uintptr_t>(src)) & 15) != 0) {
    for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < count; i += step)
      for (size_t j = i; j < i + 4 && j < count; ++j) accum[j] += src[j];
    return;
  }
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < count; i += step) {
    if (i + 3 < count) {
      float4 a = *reinterpret_cast<float4*>(accum + i);
      float4 b = *reinterpret_cast<const float4*>(src + i);
      a.x += b.x, a.y += b.y, a.z += b.z, a.w += b.w;
      *reinterpret_cast<float4*>(accum + i) = a;
    } else {
      for (size_t j = i; j < count; ++j) accum[j] += src[j];
    }
  }
}
