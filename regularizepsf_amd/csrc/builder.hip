// builder.hip - the PSF builder: ArrayPSFBuilder.build of the reference downstream of the star list
// (regularizepsf/image_processing.py:76-121 per star, regularizepsf/builder.py:53-125 per lattice cell).
//
//   B1  builder_patch_kernel    one workgroup per star, the N x N patch in LDS as float64 (N = 128: 141 KiB of the 160 KiB),
//                               phases of rpsf_core_builder.hpp separated by barriers; writes the float32 patch to a staging
//                               slot and one flag byte.  A small copy kernel appends the accepted patches to the stack.
//   B2  builder_average_kernel  one lane per pixel of a cell, the cell's member list walked in CSR order.
//   B3  builder_clean_kernel    one workgroup per averaged cell, the driver of rpsf_core_cleanup.hpp: the cell's values in registers,
//                               byte masks and union-find parents in LDS (N = 128: 96 KiB); writes the cleaned float64 cell and one
//                               flag byte.
//   B1w builder_patch_wide_kernel, B3w builder_clean_wide_kernel: B1 and B3 at the wide sizes 129 <= N <= 256 (a handle of
//                               rpsf_builder_create_wide), the drivers of rpsf_core_builder_wide.hpp and rpsf_core_cleanup_wide.hpp.  A
//                               float64 patch of that size does not fit LDS: a launch is min(items, slots) workgroups of 1024 threads,
//                               workgroup b works on items b, b + slots, ... in its own slot of a workspace in global memory that
//                               belongs to the handle.  B2 and the append kernel are size-generic and serve both.
//   B1n builder_patch_sub_kernel  rpsf_builder_add_frame_subtracted / _device_subtracted, and only then: B1 with its gather replaced by phase 1n
//                               of rpsf_core_builder_sub.hpp - every pixel of the patch takes out the fitted stars on the patch's own
//                               neighbour list (built on the host, one list per patch) while it is gathered; everything after the gather is
//                               B1's own functions.  B1's launch shape and LDS block, one chunk of star records behind it.
//   rpsf_builder_add_frame_device runs B1 on a dense float32 frame that is already on the device (a finder's, DESIGN.md 3.11, or the caller's).
//   A scaled builder (rpsf_builder_create_scaled, interpolation_scale = s of the reference) runs B1 and B2 at P = N s on frames that
//   csrc/scale.hip upscales on the device, brings every averaged P x P cell back to N x N with its kernel B4, and runs B3 at N.
//
// INVARIANT: every patch in the stack is finite and has a non-zero centre.  B1 accepts nothing else (a zero or non-finite
// pixel, or a value outside float32, rejects the patch), rpsf_builder_load_patches refuses anything else - so every sample
// (double)p / (double)centre B2 sees is finite and the order-preserving key of rpsf_core_builder.hpp is total.
// B2's cells are finite in turn, and rpsf_builder_clean refuses anything else: B3 relies on it.
// No float atomics anywhere, and the only integer ones are the atomicMin of B3's union-find, whose result (the smallest index of a
// component) does not depend on their order: flags are plain stores of one value, sums run in a fixed order - two builds of one
// input agree bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "rpsf_core_builder.hpp"
#include "rpsf_core_builder_sub.hpp"
#include "rpsf_core_builder_wide.hpp"
#include "rpsf_core_cleanup.hpp"
#include "rpsf_core_cleanup_wide.hpp"
#include "rpsf_scale.hpp"
#include "rpsf_side_unit.hpp"

using namespace rpsfb;

struct B1Params {
  const float* image;
  int height, width, N;
  const int32_t* corners;  // n x 2 rounded corners (row, col)
  const double* frac;      // n x 2 shift amounts
  double saturation, star_minimum, star_maximum;
  float* staging;  // n x N x N
  uint8_t* flags;  // n
};

template <int THREADS>
__global__ __launch_bounds__(THREADS) void builder_patch_kernel(B1Params q) {
  extern __shared__ double builder_lds[];
  const int N = q.N, tid = threadIdx.x, star = blockIdx.x;
  const Lds s = carve(builder_lds, N);
  b1_tables(tid, N, q.frac[2 * star], q.frac[2 * star + 1], s);
  b1_gather(tid, THREADS, N, q.image, q.height, q.width, q.corners[2 * star], q.corners[2 * star + 1], s);
  __syncthreads();
  b1_prefilter(tid, N, 0, s);
  __syncthreads();
  b1_prefilter(tid, N, 1, s);
  __syncthreads();
  double v[MAX_PPT];
  for (int axis = 0; axis < 2; ++axis) {
    b1_taps_read(tid, THREADS, N, axis, s, v);
    __syncthreads();
    b1_taps_write(tid, THREADS, N, s, v);
    __syncthreads();
  }
  b1_scan(tid, THREADS, N, s);
  __syncthreads();
  b1_plane(tid, N, s);
  __syncthreads();
  b1_finish(tid, THREADS, N, q.saturation, s, q.staging + (size_t)star * N * N);
  __syncthreads();
  if (tid == 0) q.flags[star] = b1_verdict(N, q.star_minimum, q.star_maximum, s);
}

// B1n: B1 with phase 1 replaced (rpsf_core_builder_sub.hpp).  The trip count of the chunk loop is the patch's, the same for every thread of the
// workgroup: every thread takes part in every barrier.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void builder_patch_sub_kernel(B1Params q, rpsfbn::Sub sub) {
  extern __shared__ double builder_lds[];
  const int N = q.N, tid = threadIdx.x, star = blockIdx.x;
  const Lds s = carve(builder_lds, N);
  const rpsfbn::Chunk chunk = rpsfbn::carve_chunk(builder_lds, N);
  const int rr = q.corners[2 * star], rc = q.corners[2 * star + 1];
  b1_tables(tid, N, q.frac[2 * star], q.frac[2 * star + 1], s);
  const long long begin = sub.offsets[star], end = sub.offsets[star + 1];
  if (begin == end) {  // (the same for every thread of the workgroup) nothing to take out: B1's own gather, whose values phase 1n's are when s = 0.0
    b1_gather(tid, THREADS, N, q.image, q.height, q.width, rr, rc, s);
  } else {
    rpsfbn::b1n_begin(tid, THREADS, N, s);
    for (long long at = begin; at < end; at += rpsfbn::CHUNK) {
      const int len = end - at < rpsfbn::CHUNK ? (int)(end - at) : rpsfbn::CHUNK;
      rpsfbn::b1n_stage(tid, sub, at, len, chunk);
      __syncthreads();
      rpsfbn::b1n_add(tid, THREADS, N, q.height, q.width, rr, rc, sub, len, chunk, s);
      __syncthreads();
    }
    rpsfbn::b1n_gather(tid, THREADS, N, q.image, q.height, q.width, rr, rc, s);
  }
  __syncthreads();
  b1_prefilter(tid, N, 0, s);
  __syncthreads();
  b1_prefilter(tid, N, 1, s);
  __syncthreads();
  double v[MAX_PPT];
  for (int axis = 0; axis < 2; ++axis) {
    b1_taps_read(tid, THREADS, N, axis, s, v);
    __syncthreads();
    b1_taps_write(tid, THREADS, N, s, v);
    __syncthreads();
  }
  b1_scan(tid, THREADS, N, s);
  __syncthreads();
  b1_plane(tid, N, s);
  __syncthreads();
  b1_finish(tid, THREADS, N, q.saturation, s, q.staging + (size_t)star * N * N);
  __syncthreads();
  if (tid == 0) q.flags[star] = b1_verdict(N, q.star_minimum, q.star_maximum, s);
}

// B1w: workgroup b owns slot b of `workspace` (rpsfbw::slot_doubles(N) doubles each) and takes stars b, b + gridDim.x, ...
__global__ __launch_bounds__(rpsfbw::THREADS) void builder_patch_wide_kernel(B1Params q, int n_stars, double* workspace) {
  extern __shared__ double builder_lds[];
  const int N = q.N;
  const rpsfbw::Wide w = rpsfbw::carve(builder_lds, workspace + (size_t)blockIdx.x * rpsfbw::slot_doubles(N), N);
  const auto each = [](auto&& f) {
    f((int)threadIdx.x);
    __syncthreads();
  };
  for (int star = blockIdx.x; star < n_stars; star += gridDim.x) {
    const uint8_t verdict = rpsfbw::b1w_star(each, N, q.image, q.height, q.width, q.corners[2 * star], q.corners[2 * star + 1],
                                             q.frac[2 * star], q.frac[2 * star + 1], q.saturation, q.star_minimum, q.star_maximum, w,
                                             q.staging + (size_t)star * N * N);
    if (threadIdx.x == 0) q.flags[star] = verdict;
    __syncthreads();  // the verdict reads the flags and the centre: the next star's first phase writes them
  }
}

// accepted patch i of the frame: staging slot source[i] -> stack slot first + i
__global__ __launch_bounds__(256) void builder_append_kernel(const float* staging, const int32_t* source, float* stack, int npix) {
  const float* from = staging + (size_t)source[blockIdx.x] * npix;
  float* to = stack + (size_t)blockIdx.x * npix;
  for (int p = threadIdx.x; p < npix; p += 256) to[p] = from[p];
}

__global__ __launch_bounds__(256) void builder_average_kernel(const float* stack, const int64_t* offsets, const int32_t* members, int N,
                                                              int method, double quantile, double* cells) {
  const int cell = blockIdx.x, pixel = blockIdx.y * 256 + threadIdx.x;
  if (pixel >= N * N) return;
  const int64_t first = offsets[cell];
  cells[(size_t)cell * N * N + pixel] = b2_pixel(stack, members + first, (long)(offsets[cell + 1] - first), N, pixel, method, quantile);
}

namespace {
struct CleanCtx {
  rpsfc::Regs mine;
  template <class F>
  __device__ __forceinline__ void each(F&& f) {
    f((int)threadIdx.x);
    __syncthreads();
  }
  __device__ __forceinline__ rpsfc::Regs& regs(int) { return mine; }
};
}  // namespace

template <int THREADS>
__global__ __launch_bounds__(THREADS) void builder_clean_kernel(int N, const double* cells, double* cleaned, uint8_t* flags) {
  extern __shared__ double builder_lds[];
  CleanCtx ctx;
  const size_t at = (size_t)blockIdx.x * N * N;
  rpsfc::clean_cell(ctx, N, THREADS, cells + at, cleaned + at, flags + blockIdx.x, builder_lds);
}

namespace {
struct CleanWideCtx {
  template <class F>
  __device__ __forceinline__ void each(F&& f) {
    f((int)threadIdx.x);
    __syncthreads();
  }
};
}  // namespace

// B3w: workgroup b owns slot b of `workspace` (rpsfcw::slot_bytes(N) bytes each) and takes cells b, b + gridDim.x, ...
__global__ __launch_bounds__(rpsfcw::THREADS) void builder_clean_wide_kernel(int N, int n_cells, const double* cells, double* cleaned,
                                                                             uint8_t* flags, char* workspace) {
  extern __shared__ double builder_lds[];
  CleanWideCtx ctx;
  for (int cell = blockIdx.x; cell < n_cells; cell += gridDim.x) {
    const size_t at = (size_t)cell * N * N;
    rpsfcw::clean_cell_wide(ctx, N, cells + at, cleaned + at, flags + cell, builder_lds, workspace + (size_t)blockIdx.x * rpsfcw::slot_bytes(N));
  }
}

struct rpsf_builder {
  int device = 0, N = 0;  // N: the size of the patches in the stack (B1, B2)
  int model = 0, scale = 1;  // model: the size of a cell of the model (B3); N = model * scale
  rpsf_scale_scratch* upscale = nullptr;
  bool wide = false;  // a handle of rpsf_builder_create_wide: N above MAX_N, B1w and B3w
  Buf<double> workspace;  // wide: the slots of B1w, which those of B3w fit into; allocated by the first launch that needs it
  Buf<double> small;  // scaled builder: the averaged cells after B4, model x model
  size_t count = 0;
  float* stack = nullptr;
  size_t capacity = 0;
  Buf<float> frame, staging;
  Buf<int32_t> corners, source, members;
  Buf<double> frac, cells, cleaned;
  Buf<uint8_t> flags, clean_flags;
  Buf<int64_t> offsets;
  // B1n: the subtraction set of the frame and the patches' neighbour lists
  Buf<double> sub_pos, sub_flux;
  Buf<int> sub_cell, sub_index;
  Buf<long long> sub_offsets;
  hipEvent_t ev[2] = {nullptr, nullptr};
  double patch_ms = 0, average_ms = 0, clean_ms = 0;
  ~rpsf_builder() {
    if (stack) (void)hipFree(stack);
    rpsf_detail_scale_scratch_free(upscale);
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

static int grow_stack(rpsf_builder* b, size_t need) {
  if (need <= b->capacity) return RPSF_OK;
  size_t cap = b->capacity ? b->capacity : 1;
  while (cap < need) cap *= 2;
  const size_t npix = (size_t)b->N * b->N;
  float* bigger = nullptr;
  HIP_TRY(hipMalloc(&bigger, cap * npix * sizeof(float)));
  if (b->count) {
    const hipError_t e = hipMemcpy(bigger, b->stack, b->count * npix * sizeof(float), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) {
      (void)hipFree(bigger);
      HIP_TRY(e);
    }
  }
  if (b->stack) (void)hipFree(b->stack);
  b->stack = bigger, b->capacity = cap;
  return RPSF_OK;
}

static int elapsed(rpsf_builder* b, double* ms) {
  float t = 0;
  HIP_TRY(hipEventSynchronize(b->ev[1]));
  HIP_TRY(hipEventElapsedTime(&t, b->ev[0], b->ev[1]));
  *ms = t;
  return RPSF_OK;
}

// B1 and B2 at patch_size * scale, B3 at patch_size
static int create(rpsf_builder** out, int device, int patch_size, int scale, size_t capacity) {
  if (!out) return fail(RPSF_E_BADARG, "null argument");
  if (patch_size < MIN_N || patch_size > MAX_N)
    return fail(RPSF_E_UNSUPPORTED, "builder patch size " + std::to_string(patch_size) + " is outside 4..128");
  if (scale < 1) return fail(RPSF_E_BADARG, "scale must be at least 1");
  if (scale > MAX_N / patch_size)
    return fail(RPSF_E_UNSUPPORTED, "builder patch size " + std::to_string(patch_size) + " times scale " + std::to_string(scale) +
                                        " is outside 4..128");
  const int P = patch_size * scale;
  HIP_TRY(hipSetDevice(device));
  rpsf_builder* b = new rpsf_builder;
  b->device = device, b->N = P, b->model = patch_size, b->scale = scale;
  auto made = [&]() -> int {
    for (auto& e : b->ev) HIP_TRY(hipEventCreate(&e));
    if (scale > 1) b->upscale = rpsf_detail_scale_scratch_new();
    // the two kernels take their sizes apart on a scaled builder: B1's LDS follows P, B3's the model's size
    if (P > 64) {
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&builder_patch_kernel<1024>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes(MAX_N)));
    } else {
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&builder_patch_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes(64)));
    }
    if (patch_size > 64)
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&builder_clean_kernel<1024>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)rpsfc::lds_bytes(MAX_N)));
    return grow_stack(b, capacity ? capacity : 1);
  }();
  if (made != RPSF_OK) {
    delete b;
    return made;
  }
  *out = b;
  return RPSF_OK;
}

extern "C" int rpsf_builder_create(rpsf_builder** out, int device, int patch_size, size_t capacity) {
  return create(out, device, patch_size, 1, capacity);
}

extern "C" int rpsf_builder_create_scaled(rpsf_builder** out, int device, int patch_size, int scale, size_t capacity) {
  return create(out, device, patch_size, scale, capacity);
}

extern "C" int rpsf_builder_create_wide(rpsf_builder** out, int device, int patch_size, size_t capacity) {
  if (!out) return fail(RPSF_E_BADARG, "null argument");
  if (patch_size < rpsfbw::MIN_N || patch_size > rpsfbw::MAX_N)
    return fail(RPSF_E_UNSUPPORTED, "wide builder patch size " + std::to_string(patch_size) + " is outside 129..256");
  HIP_TRY(hipSetDevice(device));
  rpsf_builder* b = new rpsf_builder;
  b->device = device, b->N = patch_size, b->model = patch_size, b->scale = 1, b->wide = true;
  auto made = [&]() -> int {
    for (auto& e : b->ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&builder_clean_wide_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)rpsfcw::lds_bytes(rpsfcw::MAX_N)));
    return grow_stack(b, capacity ? capacity : 1);
  }();
  if (made != RPSF_OK) {
    delete b;
    return made;
  }
  *out = b;
  return RPSF_OK;
}

extern "C" int rpsf_builder_wide_slots(const rpsf_builder* b, int* slots) {
  if (!b || !slots) return fail(RPSF_E_BADARG, "null argument");
  if (!b->wide) return fail(RPSF_E_UNSUPPORTED, "not a wide builder");
  *slots = rpsfbw::slots_for(b->N);
  return RPSF_OK;
}

// the workspace of a wide handle: slots_for(N) slots of B1w (at most 256 MiB), each of which is large enough for a slot of B3w
static int wide_workspace(rpsf_builder* b) {
  // (a slot of B1w is 16 N (N | 1) bytes, one of B3w 4 N^2 + 44160: the first is the larger from N = 61 on)
  if (rpsfcw::slot_bytes(b->N) > rpsfbw::slot_doubles(b->N) * sizeof(double)) return fail(RPSF_E_STATE, "wide workspace slots");
  HIP_TRY(b->workspace.reserve((size_t)rpsfbw::slots_for(b->N) * rpsfbw::slot_doubles(b->N)));
  return RPSF_OK;
}

extern "C" void rpsf_builder_destroy(rpsf_builder* b) {
  if (!b) return;
  (void)hipSetDevice(b->device);
  delete b;
}

// the star list of a frame of height x width, checked before anything is uploaded
static int check_stars(const rpsf_builder* b, int height, int width, int n_stars, const int32_t* corners_i32, const double* frac_f64) {
  const int N = b->N;
  for (int i = 0; i < 2 * n_stars; ++i) {
    // the reference's corner is round(position - N / 2) of a position inside the frame; anything within one frame of it is gathered
    // through the mirror map, anything farther is a caller's mistake
    const long limit = i % 2 ? width : height;
    if (corners_i32[i] < -N - limit || corners_i32[i] > 2 * limit) return fail(RPSF_E_BADARG, "a star's corner lies far outside the frame");
    if (!(std::fabs(frac_f64[i]) <= 2.0)) return fail(RPSF_E_BADARG, "a shift amount is not within two pixels");
  }
  return RPSF_OK;
}

static int patches_of_frame(rpsf_builder* b, const float* frame_dev, int height, int width, int n_stars, const int32_t* corners_i32,
                            const double* frac_f64, double saturation_threshold, double star_minimum, double star_maximum,
                            uint8_t* accepted_u8_host, const rpsfbn::Sub* sub = nullptr);

extern "C" int rpsf_builder_add_frame(rpsf_builder* b, const void* image_host, int image_is_f64, int height, int width, int n_stars,
                                      const int32_t* corners_i32, const double* frac_f64, double saturation_threshold,
                                      double star_minimum, double star_maximum, uint8_t* accepted_u8_host) {
  if (!b || !image_host) return fail(RPSF_E_BADARG, "null argument");
  if (height < 2 || width < 2) return fail(RPSF_E_BADARG, "a frame needs at least 2 x 2 pixels");
  if (n_stars < 0) return fail(RPSF_E_BADARG, "n_stars is negative");
  if (n_stars == 0) return RPSF_OK;
  if (!corners_i32 || !frac_f64 || !accepted_u8_host) return fail(RPSF_E_BADARG, "null argument");
  if (const int rc = check_stars(b, height, width, n_stars, corners_i32, frac_f64)) return rc;
  const size_t fpix = (size_t)height * width;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(b->frame.reserve(fpix));
  if (const int rc = upload_frame_f32(b->frame.p, image_host, image_is_f64, fpix)) return rc;
  return patches_of_frame(b, b->frame.p, height, width, n_stars, corners_i32, frac_f64, saturation_threshold, star_minimum, star_maximum,
                          accepted_u8_host);
}

extern "C" int rpsf_builder_add_frame_scaled(rpsf_builder* b, const void* image_host, int image_is_f64, int height, int width, int scale,
                                             int n_stars, const int32_t* corners_i32, const double* frac_f64,
                                             double saturation_threshold, double star_minimum, double star_maximum,
                                             uint8_t* accepted_u8_host) {
  if (!b || !image_host) return fail(RPSF_E_BADARG, "null argument");
  if (b->wide) return fail(RPSF_E_UNSUPPORTED, "a wide builder takes no scaled frames");
  if (scale != b->scale) return fail(RPSF_E_BADARG, "scale " + std::to_string(scale) + " is not the builder's " + std::to_string(b->scale));
  if (scale == 1)
    return rpsf_builder_add_frame(b, image_host, image_is_f64, height, width, n_stars, corners_i32, frac_f64, saturation_threshold,
                                  star_minimum, star_maximum, accepted_u8_host);
  if (height < 4 || width < 4) return fail(RPSF_E_BADARG, "the spline of the upscale needs at least 4 x 4 pixels");
  if (n_stars < 0) return fail(RPSF_E_BADARG, "n_stars is negative");
  if (n_stars == 0) return RPSF_OK;
  if (!corners_i32 || !frac_f64 || !accepted_u8_host) return fail(RPSF_E_BADARG, "null argument");
  const long hs = 1 + (long)(height - 1) * scale, ws = 1 + (long)(width - 1) * scale;
  if (hs > (1L << 30) || ws > (1L << 30)) return fail(RPSF_E_UNSUPPORTED, "the scaled frame is too large");
  if (const int rc = check_stars(b, (int)hs, (int)ws, n_stars, corners_i32, frac_f64)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  // the frame crosses PCIe once, unscaled and in its own type; the scaled frame is born in the buffer B1 reads
  if (const int rc = rpsf_detail_scale_upload(b->upscale, image_host, image_is_f64, height, width)) return rc;
  HIP_TRY(b->frame.reserve((size_t)hs * ws));
  if (const int rc = rpsf_detail_scale_run(b->upscale, image_is_f64, height, width, scale, b->frame.p, 1)) return rc;
  return patches_of_frame(b, b->frame.p, (int)hs, (int)ws, n_stars, corners_i32, frac_f64, saturation_threshold, star_minimum, star_maximum,
                          accepted_u8_host);
}

extern "C" int rpsf_builder_add_frame_device(rpsf_builder* b, const float* frame_dev, int height, int width, int n_stars,
                                             const int32_t* corners_i32, const double* frac_f64, double saturation_threshold,
                                             double star_minimum, double star_maximum, uint8_t* accepted_u8_host) {
  if (!b || !frame_dev) return fail(RPSF_E_BADARG, "null argument");
  if (height < 2 || width < 2) return fail(RPSF_E_BADARG, "a frame needs at least 2 x 2 pixels");
  if (n_stars < 0) return fail(RPSF_E_BADARG, "n_stars is negative");
  if (n_stars == 0) return RPSF_OK;
  if (!corners_i32 || !frac_f64 || !accepted_u8_host) return fail(RPSF_E_BADARG, "null argument");
  if (const int rc = check_stars(b, height, width, n_stars, corners_i32, frac_f64)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  // the frame is read where it lies - a finder's frame buffer or the caller's own array; on a scaled builder it is the scaled frame
  return patches_of_frame(b, frame_dev, height, width, n_stars, corners_i32, frac_f64, saturation_threshold, star_minimum, star_maximum,
                          accepted_u8_host);
}

// B1 - or, with `sub`, B1n - on frame_dev (height x width float32, dense, on the builder's device) and the append of what it accepts
static int patches_of_frame(rpsf_builder* b, const float* frame_dev, int height, int width, int n_stars, const int32_t* corners_i32,
                            const double* frac_f64, double saturation_threshold, double star_minimum, double star_maximum,
                            uint8_t* accepted_u8_host, const rpsfbn::Sub* sub) {
  const int N = b->N;
  const size_t npix = (size_t)N * N;
  HIP_TRY(b->corners.reserve(2 * (size_t)n_stars));
  HIP_TRY(b->frac.reserve(2 * (size_t)n_stars));
  HIP_TRY(b->flags.reserve(n_stars));
  HIP_TRY(b->staging.reserve((size_t)n_stars * npix));
  HIP_TRY(hipMemcpy(b->corners.p, corners_i32, 2 * (size_t)n_stars * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->frac.p, frac_f64, 2 * (size_t)n_stars * sizeof(double), hipMemcpyHostToDevice));
  const B1Params q{frame_dev, height, width, N, b->corners.p, b->frac.p, saturation_threshold, star_minimum, star_maximum,
                   b->staging.p, b->flags.p};
  if (b->wide)
    if (const int rc = wide_workspace(b)) return rc;
  HIP_TRY(hipEventRecord(b->ev[0], nullptr));
  if (sub && N > 64) {  // (never a wide handle: the entry points refuse it)
    hipLaunchKernelGGL(builder_patch_sub_kernel<1024>, dim3(n_stars), dim3(1024), rpsfbn::lds_bytes(N), nullptr, q, *sub);
  } else if (sub) {
    hipLaunchKernelGGL(builder_patch_sub_kernel<256>, dim3(n_stars), dim3(256), rpsfbn::lds_bytes(N), nullptr, q, *sub);
  } else if (b->wide) {
    const int grid = n_stars < rpsfbw::slots_for(N) ? n_stars : rpsfbw::slots_for(N);
    hipLaunchKernelGGL(builder_patch_wide_kernel, dim3(grid), dim3(rpsfbw::THREADS), rpsfbw::lds_bytes(N), nullptr, q, n_stars,
                       b->workspace.p);
  } else if (N > 64) {
    hipLaunchKernelGGL(builder_patch_kernel<1024>, dim3(n_stars), dim3(1024), lds_bytes(N), nullptr, q);
  } else {
    hipLaunchKernelGGL(builder_patch_kernel<256>, dim3(n_stars), dim3(256), lds_bytes(N), nullptr, q);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(b->ev[1], nullptr));
  HIP_TRY(hipMemcpy(accepted_u8_host, b->flags.p, n_stars, hipMemcpyDeviceToHost));
  if (const int rc = elapsed(b, &b->patch_ms)) return rc;
  std::vector<int32_t> source;
  for (int i = 0; i < n_stars; ++i)
    if (accepted_u8_host[i] == ACCEPTED) source.push_back(i);
  if (source.empty()) return RPSF_OK;
  if (const int rc = grow_stack(b, b->count + source.size())) return rc;
  HIP_TRY(b->source.reserve(source.size()));
  HIP_TRY(hipMemcpy(b->source.p, source.data(), source.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(builder_append_kernel, dim3((unsigned)source.size()), dim3(256), 0, nullptr, b->staging.p, b->source.p,
                     b->stack + b->count * npix, (int)npix);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  b->count += source.size();
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------ B1n (Neighbour-subtracted patches)
// what both entry points check and do: `frame_dev` is the device frame, or null for the host frame `image_host`
static int add_frame_subtracted(rpsf_builder* b, const float* frame_dev, const void* image_host, int image_is_f64, int height, int width,
                                const rpsf_stars_model* model, size_t n_all, const double* positions_host, const double* flux_host,
                                const int32_t* cells_host, double radius, int n_stars, const int32_t* own_i32, const int32_t* corners_i32,
                                const double* frac_f64, double saturation_threshold, double star_minimum, double star_maximum,
                                uint8_t* accepted_u8_host) {
  const char* name = frame_dev ? "rpsf_builder_add_frame_device_subtracted: " : "rpsf_builder_add_frame_subtracted: ";
  if (!b || (!frame_dev && !image_host)) return fail(RPSF_E_BADARG, std::string(name) + "null argument");
  if (n_all && (!model || !positions_host || !flux_host || !cells_host)) return fail(RPSF_E_BADARG, std::string(name) + "null argument");
  if (n_stars > 0 && (!own_i32 || !corners_i32 || !frac_f64 || !accepted_u8_host)) return fail(RPSF_E_BADARG, std::string(name) + "null argument");
  if (height < 2 || width < 2) return fail(RPSF_E_BADARG, std::string(name) + "a frame needs at least 2 x 2 pixels");
  if (n_stars < 0) return fail(RPSF_E_BADARG, std::string(name) + "n_stars is negative");
  if (const char* why = rpsfn::render_problem(radius, rpsfn::MODE_MODEL)) return fail(RPSF_E_BADARG, std::string(name) + why);
  if (n_all > ((size_t)1 << 30)) return fail(RPSF_E_UNSUPPORTED, std::string(name) + "more than 2^30 stars in one call");
  for (size_t i = 0; i < n_all; ++i)
    if (!rpsfp::position_ok(positions_host[2 * i], positions_host[2 * i + 1]))
      return fail(RPSF_E_BADARG, std::string(name) + "position " + std::to_string(i) + " is not finite or not inside |y|, |x| < 2^20");
  for (int k = 0; k < n_stars; ++k)
    if (own_i32[k] < -1 || (own_i32[k] >= 0 && (size_t)own_i32[k] >= n_all))
      return fail(RPSF_E_BADARG, std::string(name) + "own[" + std::to_string(k) + "] is neither -1 nor a star of the set");
  // the handles are looked at from here on: what the builder cannot do at all comes before what is wrong with the model
  if (b->wide) return fail(RPSF_E_UNSUPPORTED, std::string(name) + "a wide builder (129 to 256 pixels) cuts no neighbour-subtracted patches");
  if (b->scale > 1) return fail(RPSF_E_UNSUPPORTED, std::string(name) + "a scaled builder cuts no neighbour-subtracted patches");
  int model_device = 0, n_cells = 0, model_n = 0;
  const double* cube = nullptr;
  if (n_all) {
    rpsf_detail_stars_model_view(model, &model_device, &n_cells, &model_n, &cube);
    if (!(radius <= rpsff::max_fit_radius(model_n)))
      return fail(RPSF_E_BADARG, std::string(name) + "radius " + std::to_string(radius) + " is above min(64, N / 2 - 1) of the model's N = " +
                                     std::to_string(model_n));
  }
  if (n_all && model_device != b->device) return fail(RPSF_E_BADARG, std::string(name) + "the model is on another device than the builder");
  if (n_stars == 0) return RPSF_OK;
  if (const int rc = check_stars(b, height, width, n_stars, corners_i32, frac_f64)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  if (!frame_dev) {
    const size_t fpix = (size_t)height * width;
    HIP_TRY(b->frame.reserve(fpix));
    if (const int rc = upload_frame_f32(b->frame.p, image_host, image_is_f64, fpix)) return rc;
    frame_dev = b->frame.p;
  }
  if (n_all == 0)  // nothing to take out: B1 itself
    return patches_of_frame(b, frame_dev, height, width, n_stars, corners_i32, frac_f64, saturation_threshold, star_minimum, star_maximum,
                            accepted_u8_host);
  std::vector<long long> offsets;
  std::vector<int> index;
  rpsfbn::neighbour_lists(height, width, b->N, (size_t)n_stars, corners_i32, own_i32, n_all, positions_host, flux_host, cells_host, n_cells,
                          radius, offsets, index);
  HIP_TRY(b->sub_pos.reserve(2 * n_all));
  HIP_TRY(b->sub_flux.reserve(n_all));
  HIP_TRY(b->sub_cell.reserve(n_all));
  HIP_TRY(b->sub_offsets.reserve(offsets.size()));
  HIP_TRY(b->sub_index.reserve(index.empty() ? 1 : index.size()));
  HIP_TRY(hipMemcpy(b->sub_pos.p, positions_host, 2 * n_all * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->sub_flux.p, flux_host, n_all * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->sub_cell.p, cells_host, n_all * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->sub_offsets.p, offsets.data(), offsets.size() * sizeof(long long), hipMemcpyHostToDevice));
  if (!index.empty()) HIP_TRY(hipMemcpy(b->sub_index.p, index.data(), index.size() * sizeof(int), hipMemcpyHostToDevice));
  if (b->N > 64) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&builder_patch_sub_kernel<1024>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)rpsfbn::lds_bytes(MAX_N)));
  } else {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&builder_patch_sub_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)rpsfbn::lds_bytes(64)));
  }
  const rpsfbn::Sub sub{cube, model_n, radius * radius, model_n / 2.0 - 0.5, b->sub_pos.p, b->sub_flux.p, b->sub_cell.p, b->sub_offsets.p,
                        b->sub_index.p};
  return patches_of_frame(b, frame_dev, height, width, n_stars, corners_i32, frac_f64, saturation_threshold, star_minimum, star_maximum,
                          accepted_u8_host, &sub);
}

extern "C" int rpsf_builder_add_frame_subtracted(rpsf_builder* b, const void* image_host, int image_is_f64, int height, int width,
                                                 const rpsf_stars_model* model, size_t n_all, const double* positions_host,
                                                 const double* flux_host, const int32_t* cells_host, double radius, int n_stars,
                                                 const int32_t* own_i32, const int32_t* corners_i32, const double* frac_f64,
                                                 double saturation_threshold, double star_minimum, double star_maximum,
                                                 uint8_t* accepted_u8_host) {
  return add_frame_subtracted(b, nullptr, image_host, image_is_f64, height, width, model, n_all, positions_host, flux_host, cells_host, radius,
                              n_stars, own_i32, corners_i32, frac_f64, saturation_threshold, star_minimum, star_maximum, accepted_u8_host);
}

extern "C" int rpsf_builder_add_frame_device_subtracted(rpsf_builder* b, const float* frame_dev, int height, int width,
                                                        const rpsf_stars_model* model, size_t n_all, const double* positions_host,
                                                        const double* flux_host, const int32_t* cells_host, double radius, int n_stars,
                                                        const int32_t* own_i32, const int32_t* corners_i32, const double* frac_f64,
                                                        double saturation_threshold, double star_minimum, double star_maximum,
                                                        uint8_t* accepted_u8_host) {
  if (!frame_dev) return fail(RPSF_E_BADARG, "rpsf_builder_add_frame_device_subtracted: null argument");
  return add_frame_subtracted(b, frame_dev, nullptr, 0, height, width, model, n_all, positions_host, flux_host, cells_host, radius, n_stars,
                              own_i32, corners_i32, frac_f64, saturation_threshold, star_minimum, star_maximum, accepted_u8_host);
}

extern "C" int rpsf_builder_subtract_info(int* chunk, int* bucket, size_t* lds_bytes_128) {
  if (chunk) *chunk = rpsfbn::CHUNK;
  if (bucket) *bucket = rpsfbn::BUCKET;
  if (lds_bytes_128) *lds_bytes_128 = rpsfbn::lds_bytes(MAX_N);
  return RPSF_OK;
}

extern "C" int rpsf_builder_count(const rpsf_builder* b, size_t* count) {
  if (!b || !count) return fail(RPSF_E_BADARG, "null argument");
  *count = b->count;
  return RPSF_OK;
}

extern "C" int rpsf_builder_patches(rpsf_builder* b, size_t first, size_t count, float* host) {
  if (!b || (!host && count)) return fail(RPSF_E_BADARG, "null argument");
  if (first > b->count || count > b->count - first) return fail(RPSF_E_BADARG, "patch range outside the stack");
  if (!count) return RPSF_OK;
  const size_t npix = (size_t)b->N * b->N;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipMemcpy(host, b->stack + first * npix, count * npix * sizeof(float), hipMemcpyDeviceToHost));
  return RPSF_OK;
}

extern "C" int rpsf_builder_load_patches(rpsf_builder* b, size_t count, const float* host) {
  if (!b || (!host && count)) return fail(RPSF_E_BADARG, "null argument");
  if (!count) return RPSF_OK;
  const size_t npix = (size_t)b->N * b->N, centre = (size_t)(b->N / 2) * b->N + b->N / 2;
  for (size_t i = 0; i < count * npix; ++i)
    if (!std::isfinite(host[i])) return fail(RPSF_E_BADARG, "patch " + std::to_string(i / npix) + " has a non-finite pixel");
  for (size_t i = 0; i < count; ++i)
    if (host[i * npix + centre] == 0.0f) return fail(RPSF_E_BADARG, "patch " + std::to_string(i) + " has a zero centre pixel");
  HIP_TRY(hipSetDevice(b->device));
  if (const int rc = grow_stack(b, b->count + count)) return rc;
  HIP_TRY(hipMemcpy(b->stack + b->count * npix, host, count * npix * sizeof(float), hipMemcpyHostToDevice));
  b->count += count;
  return RPSF_OK;
}

// B2 into builder->cells, which stay on the device
static int average_on_device(rpsf_builder* b, int method, double percentile, int n_cells, const int64_t* cell_offsets_i64,
                             const int32_t* members_i32) {
  if (!b || !cell_offsets_i64) return fail(RPSF_E_BADARG, "null argument");
  if (method != RPSF_AVERAGE_MEAN && method != RPSF_AVERAGE_MEDIAN && method != RPSF_AVERAGE_PERCENTILE)
    return fail(RPSF_E_BADARG, "unknown averaging method " + std::to_string(method));
  if (method == RPSF_AVERAGE_PERCENTILE && !(percentile >= 0.0 && percentile <= 100.0))
    return fail(RPSF_E_BADARG, "percentile outside 0..100");
  if (n_cells <= 0) return fail(RPSF_E_BADARG, "n_cells must be positive");
  if (cell_offsets_i64[0] != 0) return fail(RPSF_E_BADARG, "cell_offsets[0] must be 0");
  for (int c = 0; c < n_cells; ++c)
    if (cell_offsets_i64[c + 1] < cell_offsets_i64[c]) return fail(RPSF_E_BADARG, "cell_offsets must not decrease");
  const size_t total = (size_t)cell_offsets_i64[n_cells];
  if (total && !members_i32) return fail(RPSF_E_BADARG, "null argument");
  for (size_t i = 0; i < total; ++i)
    if (members_i32[i] < 0 || (size_t)members_i32[i] >= b->count)
      return fail(RPSF_E_BADARG, "member " + std::to_string(i) + " is not a patch of the stack");
  const size_t npix = (size_t)b->N * b->N;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(b->offsets.reserve((size_t)n_cells + 1));
  HIP_TRY(b->members.reserve(total ? total : 1));
  HIP_TRY(b->cells.reserve((size_t)n_cells * npix));
  HIP_TRY(hipMemcpy(b->offsets.p, cell_offsets_i64, ((size_t)n_cells + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (total) HIP_TRY(hipMemcpy(b->members.p, members_i32, total * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipEventRecord(b->ev[0], nullptr));
  hipLaunchKernelGGL(builder_average_kernel, dim3(n_cells, (unsigned)((npix + 255) / 256)), dim3(256), 0, nullptr, b->stack, b->offsets.p,
                     b->members.p, b->N, method, percentile / 100.0, b->cells.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(b->ev[1], nullptr));
  if (b->scale > 1) {  // B4: the reference's downscale_local_mean of every averaged cell (builder.py:234-235)
    HIP_TRY(b->small.reserve((size_t)n_cells * b->model * b->model));
    if (const int rc = rpsf_detail_downscale(b->cells.p, n_cells, b->model, b->scale, b->small.p)) return rc;
  }
  return RPSF_OK;
}

// the averaged cells at the model's size, on the device: B2's own, or B4's on a scaled builder
static double* model_cells(rpsf_builder* b) { return b->scale > 1 ? b->small.p : b->cells.p; }

extern "C" int rpsf_builder_downscale(rpsf_builder* b, int n_cells, const double* cells_f64_host, double* out_f64_host) {
  if (!b || !cells_f64_host || !out_f64_host) return fail(RPSF_E_BADARG, "null argument");
  if (n_cells <= 0) return fail(RPSF_E_BADARG, "n_cells must be positive");
  if (b->wide) return fail(RPSF_E_UNSUPPORTED, "a wide builder has no scaled cells to bring down");
  const size_t big = (size_t)n_cells * b->N * b->N, little = (size_t)n_cells * b->model * b->model;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(b->cells.reserve(big));
  HIP_TRY(b->small.reserve(little));
  HIP_TRY(hipMemcpy(b->cells.p, cells_f64_host, big * sizeof(double), hipMemcpyHostToDevice));
  if (const int rc = rpsf_detail_downscale(b->cells.p, n_cells, b->model, b->scale, b->small.p)) return rc;
  HIP_TRY(hipMemcpy(out_f64_host, b->small.p, little * sizeof(double), hipMemcpyDeviceToHost));
  return RPSF_OK;
}

extern "C" int rpsf_builder_average(rpsf_builder* b, int method, double percentile, int n_cells, const int64_t* cell_offsets_i64,
                                    const int32_t* members_i32, double* cells_f64_host) {
  if (!cells_f64_host) return fail(RPSF_E_BADARG, "null argument");
  if (const int rc = average_on_device(b, method, percentile, n_cells, cell_offsets_i64, members_i32)) return rc;
  HIP_TRY(hipMemcpy(cells_f64_host, model_cells(b), (size_t)n_cells * b->model * b->model * sizeof(double), hipMemcpyDeviceToHost));
  return elapsed(b, &b->average_ms);
}

// B3 on builder->cells; the cleaned cells and the flags come back in one download each
static int clean_on_device(rpsf_builder* b, int n_cells, double* out_f64_host, uint8_t* flags_u8_host) {
  const int N = b->model;
  const size_t npix = (size_t)N * N;
  const double* cells = model_cells(b);
  HIP_TRY(b->cleaned.reserve((size_t)n_cells * npix));
  HIP_TRY(b->clean_flags.reserve((size_t)n_cells));
  if (b->wide)
    if (const int rc = wide_workspace(b)) return rc;
  HIP_TRY(hipEventRecord(b->ev[0], nullptr));
  if (b->wide) {
    const int grid = n_cells < rpsfcw::slots_for(N) ? n_cells : rpsfcw::slots_for(N);
    hipLaunchKernelGGL(builder_clean_wide_kernel, dim3(grid), dim3(rpsfcw::THREADS), rpsfcw::lds_bytes(N), nullptr, N, n_cells, cells,
                       b->cleaned.p, b->clean_flags.p, reinterpret_cast<char*>(b->workspace.p));
  } else if (N > 64) {
    hipLaunchKernelGGL(builder_clean_kernel<1024>, dim3(n_cells), dim3(1024), rpsfc::lds_bytes(N), nullptr, N, cells, b->cleaned.p,
                       b->clean_flags.p);
  } else {
    hipLaunchKernelGGL(builder_clean_kernel<256>, dim3(n_cells), dim3(256), rpsfc::lds_bytes(N), nullptr, N, cells, b->cleaned.p,
                       b->clean_flags.p);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(b->ev[1], nullptr));
  HIP_TRY(hipMemcpy(out_f64_host, b->cleaned.p, (size_t)n_cells * npix * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(flags_u8_host, b->clean_flags.p, (size_t)n_cells, hipMemcpyDeviceToHost));
  return elapsed(b, &b->clean_ms);
}

extern "C" int rpsf_builder_clean(rpsf_builder* b, int n_cells, const double* cells_f64_host, double* out_f64_host,
                                  uint8_t* flags_u8_host) {
  if (!b || !cells_f64_host || !out_f64_host || !flags_u8_host) return fail(RPSF_E_BADARG, "null argument");
  if (n_cells <= 0) return fail(RPSF_E_BADARG, "n_cells must be positive");
  const size_t npix = (size_t)b->model * b->model;
  for (size_t i = 0; i < (size_t)n_cells * npix; ++i)
    if (!std::isfinite(cells_f64_host[i])) return fail(RPSF_E_BADARG, "cell " + std::to_string(i / npix) + " has a non-finite pixel");
  HIP_TRY(hipSetDevice(b->device));
  Buf<double>& cells = b->scale > 1 ? b->small : b->cells;
  HIP_TRY(cells.reserve((size_t)n_cells * npix));
  HIP_TRY(hipMemcpy(cells.p, cells_f64_host, (size_t)n_cells * npix * sizeof(double), hipMemcpyHostToDevice));
  return clean_on_device(b, n_cells, out_f64_host, flags_u8_host);
}

extern "C" int rpsf_builder_model(rpsf_builder* b, int method, double percentile, int n_cells, const int64_t* cell_offsets_i64,
                                  const int32_t* members_i32, double* out_f64_host, uint8_t* flags_u8_host) {
  if (!out_f64_host || !flags_u8_host) return fail(RPSF_E_BADARG, "null argument");
  if (const int rc = average_on_device(b, method, percentile, n_cells, cell_offsets_i64, members_i32)) return rc;
  if (const int rc = elapsed(b, &b->average_ms)) return rc;
  return clean_on_device(b, n_cells, out_f64_host, flags_u8_host);
}

extern "C" int rpsf_builder_clean_ms(const rpsf_builder* b, double* ms) {
  if (!b || !ms) return fail(RPSF_E_BADARG, "null argument");
  *ms = b->clean_ms;
  return RPSF_OK;
}

extern "C" int rpsf_builder_kernel_ms(const rpsf_builder* b, double* patch_ms, double* average_ms) {
  if (!b) return fail(RPSF_E_BADARG, "null argument");
  if (patch_ms) *patch_ms = b->patch_ms;
  if (average_ms) *average_ms = b->average_ms;
  return RPSF_OK;
}
