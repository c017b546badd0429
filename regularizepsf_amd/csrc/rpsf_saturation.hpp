// rpsf_saturation.hpp - what csrc/rpsf_saturated.hip sees of csrc/saturation.hip: the device scratch of a plan's saturation branch (owned by the
// plan, rpsf_plan.hpp) and the two halves of the route around the correction of the padded frames (which is the plan's own launch, rpsf.hip).  The unit of work is the
// frame-group: `frames` frames of one shape; a single frame is a frame-group of one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rpsfsat {
struct MaskView;  // csrc/rpsf_core_saturation.hpp
}
struct SatDevice;  // scratch, events and counters; owned by the plan, made at the first call, grown when a larger frame-group arrives

struct SatCall {
  int H, W, N, pad_mode, dilation, width;
  double threshold;
  int in_row0, out_row0, out_rows;  // rows of the padded frame the correction reads from / writes (SatRun::init's geometry)
};

__attribute__((visibility("hidden"))) SatDevice* rpsf_sat_create();
__attribute__((visibility("hidden"))) void rpsf_sat_destroy(SatDevice* s);  // (the plan's device is current)
__attribute__((visibility("hidden"))) int rpsf_sat_kernel_ms(SatDevice* s, double ms[5]);  // F1 ... F5 of the last frame-group, device time

// `frames` frames of one shape, image_stride floats apart (csrc/rpsf_core_saturation_batch.hpp).  F1 - F4 on `st` with ONE
// synchronisation of it for all frames; F4 is one launch over every frame's groups in `order_mode` (rpsfsatb::ORDER_*).  *padded: the
// filled padded frames, *p_stride floats apart; *corrected: room for out_rows x PW float32 per frame, *c_stride apart.
__attribute__((visibility("hidden"))) int rpsf_sat_fill_batch(SatDevice* s, const SatCall& c, int frames, const float* images_dev, size_t image_stride,
                                                               int order_mode, hipStream_t st, float** padded, size_t* p_stride, float** corrected,
                                                               size_t* c_stride);
// The same with a bad-pixel mask ("Bad-pixel masks"): masks_host[f] is frame f's uint8 view in DEVICE memory (null: no
// frame has one), fill_nonfinite: NaN and +-Inf of the padded frame are masked too.  These pixels are masked as they are, not dilated.
__attribute__((visibility("hidden"))) int rpsf_sat_fill_batch_masked(SatDevice* s, const SatCall& c, int frames, const float* images_dev,
                                                                      size_t image_stride, const rpsfsat::MaskView* masks_host, int fill_nonfinite,
                                                                      int order_mode, hipStream_t st, float** padded, size_t* p_stride,
                                                                      float** corrected, size_t* c_stride);
// F5 of every frame of the last rpsf_sat_fill_batch, one launch
__attribute__((visibility("hidden"))) int rpsf_sat_restore_batch(SatDevice* s, const SatCall& c, const float* images_dev, size_t image_stride,
                                                                  float* outs_dev, size_t out_stride, hipStream_t st);
// every frame's list to the host, one wait for `st`: frame fr's entries start at info_host[FRAME_INFO * fr + I_LIST0] and number
// counters_host[FRAME_COUNTERS * fr + C_LIST]; *list_host stays null, and nothing is waited for, when no frame had a masked pixel
__attribute__((visibility("hidden"))) int rpsf_sat_lists_batch(SatDevice* s, hipStream_t st, const int32_t** list_host, const int** info_host,
                                                                const int** counters_host);
__attribute__((visibility("hidden"))) int rpsf_sat_masks_batch(SatDevice* s, const SatCall& c, hipStream_t st, uint8_t* masks_host);  // frames x PH x PW bytes
__attribute__((visibility("hidden"))) int rpsf_sat_frame_counts(SatDevice* s, int frame, int* n_hot, int* n_mask, int* n_groups);  // of the last frame-group
__attribute__((visibility("hidden"))) void rpsf_sat_batch_totals(SatDevice* s, long* groups, long* masked);  // of the last frame-group
