// rpsf_scale.hpp - what csrc/scale.hip offers the other units of the library (csrc/builder.hip): the frame upscale and the block mean on
// arrays that are already on the device.  Everything runs on the null stream of the current device.
#pragma once
#include <cstdint>

struct rpsf_scale_scratch;  // intermediates of the upscale, pivot table and events; grows, never shrinks
rpsf_scale_scratch* rpsf_detail_scale_scratch_new();
void rpsf_detail_scale_scratch_free(rpsf_scale_scratch* scratch);

// The host frame (float32 or float64, height x width) uploaded as it is into the scratch.
int rpsf_detail_scale_upload(rpsf_scale_scratch* scratch, const void* image_host, int image_is_f64, int height, int width);
// U1 and U2 on the uploaded frame: out_dev receives scaled(height) x scaled(width) values, float32 if out_is_f32, else float64.
// The device times of the two passes are kept for rpsf_scale_kernel_ms.  scale >= 2, height and width >= 4.
int rpsf_detail_scale_run(rpsf_scale_scratch* scratch, int image_is_f64, int height, int width, int scale, void* out_dev, int out_is_f32);
// B4: n_cells cells of (N scale)^2 float64 -> n_cells cells of N^2 float64 (launch only).
int rpsf_detail_downscale(const double* cells_dev, int n_cells, int N, int scale, double* out_dev);
