// scale.hip - interpolation_scale of ArrayPSFBuilder.build: the frame upscale of regularizepsf/image_processing.py:49-59 and the block
// mean of regularizepsf/builder.py:234-235.  The per-thread work is in rpsf_core_scale.hpp, with the mathematics.
//
//   U1  scale_line_kernel       axis 0: one lane per column of the H x W frame (float32 or float64 as it came), the whole column solved
//                               and evaluated by that lane, loads and stores coalesced along the row.  Writes Hs x W float64.
//   U2  scale_transpose_kernel  axis 1: the Hs x W intermediate transposed through LDS in 32 x 32 tiles, scale_line_kernel again with one
//       scale_line_kernel       lane per row, and the transpose back, which writes float64 (rpsf_scale_image) or float32 straight into
//       scale_transpose_kernel  the builder's frame buffer (rpsf_builder_add_frame_scaled).
//   B4  scale_block_mean_kernel one lane per pixel of an N x N cell: the s x s block of the P x P averaged cell, row-major, float64.
//
// No atomics: every output has one writer and every sum a fixed order, so two runs of one input agree bit for bit.
#include <hip/hip_runtime.h>

#include <climits>
#include <string>
#include <vector>

#include "rpsf_core_scale.hpp"
#include "rpsf_scale.hpp"
#include "rpsf_side_unit.hpp"

using namespace rpsfs;

template <class T>
__global__ __launch_bounds__(LINE_THREADS) void scale_line_kernel(long lanes, int m, int s, const T* y, const double* ip, double* work,
                                                                  double* out) {
  u_line(global_id(), lanes, m, s, y, ip, work, out);
}

template <class Tout>
__global__ __launch_bounds__(TILE* TILE_ROWS) void scale_transpose_kernel(long rows, long cols, const double* in, Tout* out) {
  __shared__ double tile[TILE * TILE_LD];
  t_load((int)threadIdx.x, blockIdx.y, blockIdx.x, rows, cols, in, tile);
  __syncthreads();
  t_store((int)threadIdx.x, blockIdx.y, blockIdx.x, rows, cols, tile, out);
}

__global__ __launch_bounds__(256) void scale_block_mean_kernel(const double* cells, int N, int s, double* out) {
  const int pixel = blockIdx.y * 256 + threadIdx.x;
  if (pixel >= N * N) return;
  const size_t cell = blockIdx.x;
  out[cell * N * N + pixel] = b4_pixel(cells + cell * (size_t)(N * s) * (N * s), N, s, pixel);
}

struct rpsf_scale_scratch {
  Buf<char> input;                 // the frame as uploaded
  Buf<double> rows, turned, cols;  // Hs x W, W x Hs, Ws x Hs
  Buf<double> work, pivots;
  std::vector<double> pivots_host;  // of the longest line so far: a shorter line's table is its prefix
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  ~rpsf_scale_scratch() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

static thread_local double last_u1_ms = 0, last_u2_ms = 0;

rpsf_scale_scratch* rpsf_detail_scale_scratch_new() { return new rpsf_scale_scratch; }
void rpsf_detail_scale_scratch_free(rpsf_scale_scratch* scratch) { delete scratch; }

int rpsf_detail_scale_upload(rpsf_scale_scratch* q, const void* image_host, int image_is_f64, int height, int width) {
  const size_t bytes = (size_t)height * width * (image_is_f64 ? sizeof(double) : sizeof(float));
  HIP_TRY(q->input.reserve(bytes));
  HIP_TRY(hipMemcpy(q->input.p, image_host, bytes, hipMemcpyHostToDevice));
  return RPSF_OK;
}

template <class T>
static void launch_line(long lanes, int m, int s, const T* y, const double* ip, double* work, double* out) {
  hipLaunchKernelGGL(scale_line_kernel<T>, dim3((unsigned)((lanes + LINE_THREADS - 1) / LINE_THREADS)), dim3(LINE_THREADS), 0, nullptr, lanes,
                     m, s, y, ip, work, out);
}

template <class Tout>
static void launch_transpose(long rows, long cols, const double* in, Tout* out) {
  hipLaunchKernelGGL(scale_transpose_kernel<Tout>, dim3((unsigned)((cols + TILE - 1) / TILE), (unsigned)((rows + TILE - 1) / TILE)),
                     dim3(TILE * TILE_ROWS), 0, nullptr, rows, cols, in, out);
}

int rpsf_detail_scale_run(rpsf_scale_scratch* q, int image_is_f64, int height, int width, int scale, void* out_dev, int out_is_f32) {
  if (height < MIN_LINE || width < MIN_LINE) return fail(RPSF_E_BADARG, "the spline of the upscale needs at least 4 x 4 pixels");
  if (scale < 2) return fail(RPSF_E_BADARG, "scale must be at least 2 here");
  const long hs = scaled(height, scale), ws = scaled(width, scale);
  if (hs > INT_MAX || ws > INT_MAX || hs * ws > (1L << 40)) return fail(RPSF_E_UNSUPPORTED, "the scaled frame is too large");
  const int longest = height > width ? height : width;
  for (auto& e : q->ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  if ((int)q->pivots_host.size() < longest - 4) {
    q->pivots_host.resize((size_t)longest - 4);
    pivot_table(longest, q->pivots_host.data());
    HIP_TRY(q->pivots.reserve(q->pivots_host.size()));
    HIP_TRY(hipMemcpy(q->pivots.p, q->pivots_host.data(), q->pivots_host.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  HIP_TRY(q->pivots.reserve(1));  // 4 x 4: no unknowns, but a pointer the kernel may hold
  HIP_TRY(q->rows.reserve((size_t)hs * width));
  HIP_TRY(q->turned.reserve((size_t)hs * width));
  HIP_TRY(q->cols.reserve((size_t)hs * ws));
  HIP_TRY(q->work.reserve((size_t)(height > hs ? height : hs) * width));  // axis 0: (H - 4) x W, axis 1: (W - 4) x Hs
  HIP_TRY(hipEventRecord(q->ev[0], nullptr));
  if (image_is_f64) {
    launch_line<double>(width, height, scale, reinterpret_cast<const double*>(q->input.p), q->pivots.p, q->work.p, q->rows.p);
  } else {
    launch_line<float>(width, height, scale, reinterpret_cast<const float*>(q->input.p), q->pivots.p, q->work.p, q->rows.p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(q->ev[1], nullptr));
  launch_transpose<double>(hs, width, q->rows.p, q->turned.p);  // -> W x Hs
  HIP_TRY(hipGetLastError());
  launch_line<double>(hs, width, scale, q->turned.p, q->pivots.p, q->work.p, q->cols.p);  // -> Ws x Hs
  HIP_TRY(hipGetLastError());
  if (out_is_f32) {
    launch_transpose<float>(ws, hs, q->cols.p, static_cast<float*>(out_dev));  // -> Hs x Ws
  } else {
    launch_transpose<double>(ws, hs, q->cols.p, static_cast<double*>(out_dev));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(q->ev[2], nullptr));
  HIP_TRY(hipEventSynchronize(q->ev[2]));
  float u1 = 0, u2 = 0;
  HIP_TRY(hipEventElapsedTime(&u1, q->ev[0], q->ev[1]));
  HIP_TRY(hipEventElapsedTime(&u2, q->ev[1], q->ev[2]));
  last_u1_ms = u1, last_u2_ms = u2;
  return RPSF_OK;
}

int rpsf_detail_downscale(const double* cells_dev, int n_cells, int N, int scale, double* out_dev) {
  hipLaunchKernelGGL(scale_block_mean_kernel, dim3((unsigned)n_cells, blocks_for((long)N * N)), dim3(256), 0, nullptr, cells_dev, N, scale,
                     out_dev);
  HIP_TRY(hipGetLastError());
  return RPSF_OK;
}

extern "C" int rpsf_scale_image(int device, const void* image_host, int image_is_f64, int height, int width, int scale,
                                double* out_f64_host) {
  if (!image_host || !out_f64_host) return fail(RPSF_E_BADARG, "null argument");
  if (height < MIN_LINE || width < MIN_LINE) return fail(RPSF_E_BADARG, "the spline of the upscale needs at least 4 x 4 pixels");
  if (scale < 1) return fail(RPSF_E_BADARG, "scale must be at least 1");
  if (scale == 1) {  // the reference does not resample at all
    const size_t count = (size_t)height * width;
    for (size_t i = 0; i < count; ++i)
      out_f64_host[i] = image_is_f64 ? static_cast<const double*>(image_host)[i] : (double)static_cast<const float*>(image_host)[i];
    return RPSF_OK;
  }
  HIP_TRY(hipSetDevice(device));
  rpsf_scale_scratch q;
  Buf<double> out;
  const size_t count = (size_t)scaled(height, scale) * (size_t)scaled(width, scale);
  if (const int rc = rpsf_detail_scale_upload(&q, image_host, image_is_f64, height, width)) return rc;
  HIP_TRY(out.reserve(count));
  if (const int rc = rpsf_detail_scale_run(&q, image_is_f64, height, width, scale, out.p, 0)) return rc;
  HIP_TRY(hipMemcpy(out_f64_host, out.p, count * sizeof(double), hipMemcpyDeviceToHost));
  return RPSF_OK;
}

extern "C" int rpsf_scale_kernel_ms(double* u1_ms, double* u2_ms) {
  if (!u1_ms && !u2_ms) return fail(RPSF_E_BADARG, "null argument");
  if (u1_ms) *u1_ms = last_u1_ms;
  if (u2_ms) *u2_ms = last_u2_ms;
  return RPSF_OK;
}
