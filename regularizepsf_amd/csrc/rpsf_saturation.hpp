// rpsf_saturation.hpp - what csrc/rpsf.hip sees of csrc/saturation.hip: the device scratch of a plan's saturation branch and the two
// halves of the route around the correction of the padded frame (which is the plan's own launch, rpsf.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

struct SatDevice;  // scratch, events and counters; owned by the plan, made at the first call, grown when a larger frame arrives

struct SatCall {
  int H, W, N, pad_mode, dilation, width;
  double threshold;
  int in_row0, out_row0, out_rows;  // rows of the padded frame the correction reads from / writes (SatRun::init's geometry)
  bool reverse_groups;              // testing aid: F4's workgroups take the groups last first
};

__attribute__((visibility("hidden"))) SatDevice* rpsf_sat_create();
__attribute__((visibility("hidden"))) void rpsf_sat_destroy(SatDevice* s);  // (the plan's device is current)
// F1 - F4 on `st`, one synchronisation of it in between (hot count, group count, masked count).  *padded: the filled padded frame
// (PH x PW float32), *corrected: room for out_rows x PW float32.
__attribute__((visibility("hidden"))) int rpsf_sat_fill(SatDevice* s, const SatCall& c, const float* image_dev, hipStream_t st, float** padded,
                                                         float** corrected);
// F5 on `st`: raw values on the mask, crop into out_dev (H x W), the list of masked in-frame pixels
__attribute__((visibility("hidden"))) int rpsf_sat_restore(SatDevice* s, const SatCall& c, const float* image_dev, float* out_dev, hipStream_t st);
// copies the list of F5 (row * W + col of every masked in-frame pixel, in no particular order) to the host and waits for `st`;
// *list_host stays null, and nothing is waited for, when nothing was hot
__attribute__((visibility("hidden"))) int rpsf_sat_list(SatDevice* s, hipStream_t st, const int32_t** list_host, size_t* count);
__attribute__((visibility("hidden"))) int rpsf_sat_mask(SatDevice* s, const SatCall& c, hipStream_t st, uint8_t* mask_host);  // PH x PW bytes (zeros when nothing was hot)
__attribute__((visibility("hidden"))) int rpsf_sat_counts(SatDevice* s, int* n_hot, int* n_mask, int* n_groups);  // of the last fill
__attribute__((visibility("hidden"))) int rpsf_sat_kernel_ms(SatDevice* s, double ms[5]);
