// rpsf_convert.hpp - what csrc/rpsf_saturated.hip sees of csrc/convert.hip: the launches of the two conversion kernels around the plan's own apply
// (rpsf_apply_view, rpsf_apply_batch_view).  `frames` views of v's shape, dtype and strides, frame_stride bytes apart, against dense
// float32 frames dense_frame_stride floats apart; one launch, asynchronous on `st`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/rpsf.h"

__attribute__((visibility("hidden"))) int rpsf_conv_gather(const rpsf_view& v, int frames, int64_t frame_stride, float* dense, int64_t dense_frame_stride,
                                                            hipStream_t st);  // kernel C1
__attribute__((visibility("hidden"))) int rpsf_conv_scatter(const float* dense, int64_t dense_frame_stride, const rpsf_view& v, int frames,
                                                             int64_t frame_stride, hipStream_t st);  // kernel C2
