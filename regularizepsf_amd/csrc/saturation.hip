// saturation.hip - the saturation branch of ArrayPSFTransform.apply on the device: what SatRun::prepare / finish of
// rpsf.hip do on the host, for a float32 frame that is already on the GPU.
//
//   F1  sat_pad_kernel                     2N-padded float32 frame and one hot byte per pixel (value > threshold), hot count
//   F2  sat_cross_kernel x dilation        mask = hot dilated with the cross element (two byte planes in turn), masked count
//   F3  sat_rows / sat_cols_kernel         mask grown by a box of reach h / 2, then the star finder's labeller (S3) and root list (S4)
//       sat_group_init / accumulate        per group: masked pixels and their bounding box
//   F4  sat_fill_kernel                    one wave per group: the sequential nan-mean fill of the group's pixels in raster order
//   F5  sat_restore_kernel                 raw values on the mask, crop, list of the masked in-frame pixels
//
// A group of frames of one shape goes through the same phases with the frame as a grid index (sat_*_batch_kernel, the drivers of
// rpsf_core_saturation_batch.hpp): F1 - F3 once for all frames, ONE host wait, one F4 launch over all frames' groups, longest first.
//
// The phases are the drivers of rpsf_core_saturation.hpp.  Every launch goes to the caller's stream; the host waits for it once, between
// the root count and the root list, to size the group table.  When nothing is hot every kernel after F1 returns at its first
// instruction and F4 is not launched.  The only atomics are integer adds / min / max.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/rpsf.h"
#include "rpsf_core_saturation.hpp"
#include "rpsf_core_saturation_batch.hpp"
#include "rpsf_saturation.hpp"

using namespace rpsfs;
using namespace rpsfsat;
using rpsfsatb::Stack;
using rpsfsatb::Tables;

int rpsf_detail_fail(int code, const std::string& msg);  // rpsf.hip: sets rpsf_last_error of the calling thread
static int fail(int code, const std::string& msg) { return rpsf_detail_fail(code, msg); }
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
enum { N_HOT, N_MASK, N_GROUPS, CURSOR, N_LIST, N_COUNTERS };
}  // namespace

extern __shared__ __attribute__((aligned(16))) char sat_lds[];

__global__ __launch_bounds__(256) void sat_pad_kernel(Padded f, const float* image, double threshold, float* padded, uint8_t* hot, int* counters) {
  f1_pad(global_id(), f, image, threshold, padded, hot, counters + N_HOT);
}
// (every kernel from here to F4 leaves at once when F1 found nothing: counters[N_HOT] is the same word for all threads)
__global__ __launch_bounds__(256) void sat_cross_kernel(int PH, int PW, const uint8_t* src, uint8_t* dst, int* counters, int last) {
  if (counters[N_HOT] == 0) return;
  f2_cross(global_id(), PH, PW, src, dst, last ? counters + N_MASK : nullptr);
}
__global__ __launch_bounds__(256) void sat_rows_kernel(int PH, int PW, int reach, const uint8_t* mask, uint8_t* tmp, const int* counters) {
  if (counters[N_HOT] == 0) return;
  f3_rows(global_id(), PH, PW, reach, mask, tmp);
}
__global__ __launch_bounds__(256) void sat_cols_kernel(int PH, int PW, int reach, const uint8_t* tmp, uint8_t* grown, const int* counters) {
  if (counters[N_HOT] == 0) return;
  f3_cols(global_id(), PH, PW, reach, tmp, grown);
}
__global__ __launch_bounds__(TILE_THREADS) void sat_label_tile_kernel(const uint8_t* grown, int PH, int PW, int32_t* labels, const int* counters) {
  if (counters[N_HOT] == 0) return;
  GpuCtx ctx;
  s3_tile(ctx, grown, PH, PW, (int)blockIdx.y, (int)blockIdx.x, reinterpret_cast<int*>(sat_lds), labels);
}
__global__ __launch_bounds__(256) void sat_label_seam_kernel(int PH, int PW, int32_t* labels, const int* counters) {
  if (counters[N_HOT] == 0) return;
  s3_seam(global_id(), PH, PW, labels);
}
__global__ __launch_bounds__(256) void sat_label_flatten_kernel(long npix, int32_t* labels, const int* counters) {
  if (counters[N_HOT] == 0) return;
  s3_flatten(global_id(), npix, labels);
}
__global__ __launch_bounds__(256) void sat_count_kernel(int PH, int PW, const int32_t* labels, int* segcnt, const int* counters) {
  if (counters[N_HOT] == 0) return;
  s4_count(global_id(), PH, PW, labels, segcnt);
}
__global__ __launch_bounds__(SCAN_THREADS) void sat_scan_kernel(long nseg, const int* segcnt, int* segoff, int* counters) {
  if (counters[N_HOT] == 0) return;
  GpuCtx ctx;
  s4_scan(ctx, nseg, segcnt, segoff, counters + N_GROUPS, reinterpret_cast<int*>(sat_lds));
}
__global__ __launch_bounds__(256) void sat_roots_kernel(int PH, int PW, const int32_t* labels, const int* segoff, int* roots) {
  s4_roots(global_id(), PH, PW, labels, segoff, roots);
}
__global__ __launch_bounds__(256) void sat_group_init_kernel(long count, int* stats) { f3_init(global_id(), count, stats); }
__global__ __launch_bounds__(256) void sat_group_accumulate_kernel(long npix, int PW, const uint8_t* mask, const int32_t* labels, const int* roots,
                                                                   long count, int* stats) {
  f3_accumulate(global_id(), npix, PW, mask, labels, roots, count, stats);
}
__global__ __launch_bounds__(FILL_LANES) void sat_fill_kernel(long count, int reverse, int PH, int PW, int h, const uint8_t* mask, const int* roots,
                                                              const int* stats, float* padded, int32_t* labels, double* fills, int* counters) {
  GpuCtx ctx;
  const long g = reverse ? count - 1 - (long)blockIdx.x : (long)blockIdx.x;
  f4_group(ctx, g, PH, PW, h, mask, roots, stats, padded, labels, fills, counters + CURSOR, reinterpret_cast<FillLds*>(sat_lds));
}
__global__ __launch_bounds__(256) void sat_restore_kernel(Padded f, const float* image, const uint8_t* mask, const float* corrected, int out_row0,
                                                          float* out, int32_t* list, int* counters) {
  f5_restore(global_id(), f, image, mask, corrected, out_row0, out, list, counters + N_LIST);
}

// ---- the same for a group of frames: blockIdx.y (the labeller's tiles: blockIdx.z) is the frame
__global__ __launch_bounds__(256) void sat_pad_batch_kernel(Stack s, const float* images, size_t image_stride, double threshold) {
  rpsfsatb::b1_pad(global_id(), (int)blockIdx.y, s, images, image_stride, threshold);
}
__global__ __launch_bounds__(256) void sat_cross_batch_kernel(Stack s, int from, int last) {
  rpsfsatb::b2_cross(global_id(), (int)blockIdx.y, s, from, last);
}
__global__ __launch_bounds__(256) void sat_rows_batch_kernel(Stack s, int reach, int at) { rpsfsatb::b3_rows(global_id(), (int)blockIdx.y, s, reach, at); }
__global__ __launch_bounds__(256) void sat_cols_batch_kernel(Stack s, int reach, int at) { rpsfsatb::b3_cols(global_id(), (int)blockIdx.y, s, reach, at); }
__global__ __launch_bounds__(TILE_THREADS) void sat_label_tile_batch_kernel(Stack s, int grown) {
  GpuCtx ctx;
  rpsfsatb::b3_tile(ctx, (int)blockIdx.z, s, grown, (int)blockIdx.y, (int)blockIdx.x, reinterpret_cast<int*>(sat_lds));
}
__global__ __launch_bounds__(256) void sat_label_seam_batch_kernel(Stack s) { rpsfsatb::b3_seam(global_id(), (int)blockIdx.y, s); }
__global__ __launch_bounds__(256) void sat_label_flatten_batch_kernel(Stack s) { rpsfsatb::b3_flatten(global_id(), (int)blockIdx.y, s); }
__global__ __launch_bounds__(256) void sat_count_batch_kernel(Stack s) { rpsfsatb::b3_count(global_id(), (int)blockIdx.y, s); }
__global__ __launch_bounds__(SCAN_THREADS) void sat_scan_batch_kernel(Stack s) {
  GpuCtx ctx;
  rpsfsatb::b3_scan(ctx, (int)blockIdx.x, s, reinterpret_cast<int*>(sat_lds));
}
__global__ __launch_bounds__(256) void sat_roots_batch_kernel(Stack s, Tables t) { rpsfsatb::b3_roots(global_id(), (int)blockIdx.y, s, t); }
__global__ __launch_bounds__(256) void sat_group_init_batch_kernel(Tables t) { rpsfsatb::b3_init(global_id(), (int)blockIdx.y, t); }
__global__ __launch_bounds__(256) void sat_group_accumulate_batch_kernel(Stack s, Tables t, int at) {
  rpsfsatb::b3_accumulate(global_id(), (int)blockIdx.y, s, t, at);
}
__global__ __launch_bounds__(256) void sat_order_hist_kernel(Tables t) { rpsfsatb::o_hist(global_id(), t); }
__global__ __launch_bounds__(256) void sat_order_scatter_kernel(Tables t) { rpsfsatb::o_scatter(global_id(), t); }
__global__ __launch_bounds__(FILL_LANES) void sat_fill_batch_kernel(Stack s, Tables t, int order_mode, int at, int h) {
  GpuCtx ctx;
  rpsfsatb::b4_group(ctx, (long)blockIdx.x, order_mode, s, t, at, h, reinterpret_cast<FillLds*>(sat_lds));
}
__global__ __launch_bounds__(256) void sat_restore_batch_kernel(Stack s, const int* info, int at, const float* images, size_t image_stride,
                                                                const float* corrected, size_t c_stride, int out_row0, float* outs,
                                                                size_t out_stride, int32_t* lists) {
  rpsfsatb::b5_restore(global_id(), (int)blockIdx.y, s, info, at, images, image_stride, corrected, c_stride, out_row0, outs, out_stride, lists);
}

namespace {
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
template <class T>
struct PinnedBuf {  // the same in page-locked host memory
  T* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t count) {
    if (count <= cap) return hipSuccess;
    if (p) {
      (void)hipDeviceSynchronize();
      (void)hipHostFree(p);
    }
    p = nullptr, cap = 0;
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), count * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) cap = count;
    return e;
  }
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
};
unsigned blocks_for(long threads) { return (unsigned)((threads + 255) / 256); }
}  // namespace

struct SatDevice {
  Buf<float> padded, corrected;
  Buf<uint8_t> bytes[3];  // hot / mask in turn, the row-grown and the grown mask
  Buf<int32_t> labels, list;
  Buf<int> segcnt, segoff, roots, stats, counters;
  Buf<double> fills;
  PinnedBuf<int> h_counters;
  PinnedBuf<int32_t> h_list;
  const uint8_t* mask = nullptr;  // of the last fill; null: nothing was hot
  size_t list_cap = 0;
  int n_hot = 0, n_mask = 0, n_groups = 0;
  enum { E_START, E_F1, E_F2, E_F3, E_F4, E_F5A, E_F5B, N_EVENTS };
  hipEvent_t ev[N_EVENTS] = {};
  bool timed = false, restored = false;
  // a group of frames (rpsf_sat_fill_batch): the arrays above hold `b_frames` frames b_stride apart, counters and tables are these
  Buf<int> b_counters, b_info, b_gframe, b_order;  // FRAME_COUNTERS per frame + SHARED_COUNTERS; FRAME_INFO per frame; per group
  PinnedBuf<int> h_b_counters, h_b_info;
  int b_frames = 0, b_at = 0;
  size_t b_stride = 0, b_cstride = 0, b_nseg = 0;
  long b_groups = 0, b_masked = 0, b_listed = 0;
  ~SatDevice() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

SatDevice* rpsf_sat_create() { return new SatDevice; }
void rpsf_sat_destroy(SatDevice* s) { delete s; }

int rpsf_sat_fill(SatDevice* s, const SatCall& c, const float* image_dev, hipStream_t st, float** padded, float** corrected) {
  const Padded f{c.H, c.W, c.N, c.H + 4 * c.N, c.W + 4 * c.N, c.pad_mode};
  const long npix = f.npix(), nseg = (long)f.PH * segs_per_row(f.PW);
  const int PH = f.PH, PW = f.PW, h = c.width / 2;
  const size_t np = (size_t)npix;
  s->timed = s->restored = false;
  s->mask = nullptr;
  s->n_hot = s->n_mask = s->n_groups = 0;
  // (growing frees the old array: nothing of an earlier call may still be running on it)
  if (np > s->padded.cap || (size_t)c.out_rows * PW > s->corrected.cap) HIP_TRY(hipDeviceSynchronize());
  for (auto& e : s->ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  HIP_TRY(s->padded.reserve(np));
  HIP_TRY(s->corrected.reserve((size_t)c.out_rows * PW));
  for (auto& b : s->bytes) HIP_TRY(b.reserve(np));
  HIP_TRY(s->labels.reserve(np));
  HIP_TRY(s->segcnt.reserve((size_t)nseg));
  HIP_TRY(s->segoff.reserve((size_t)nseg));
  HIP_TRY(s->counters.reserve(N_COUNTERS));
  HIP_TRY(s->h_counters.reserve(N_COUNTERS));
  *padded = s->padded.p, *corrected = s->corrected.p;
  int* const cnt = s->counters.p;
  const unsigned quads = blocks_for((npix + 3) / 4), pixels = blocks_for(npix);

  HIP_TRY(hipMemsetAsync(cnt, 0, N_COUNTERS * sizeof(int), st));
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_START], st));
  hipLaunchKernelGGL(sat_pad_kernel, dim3(quads), dim3(256), 0, st, f, image_dev, c.threshold, s->padded.p, s->bytes[0].p, cnt);
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F1], st));
  int at = 0;  // bytes[at]: the mask so far
  for (int pass = 0; pass < c.dilation; ++pass, at ^= 1)
    hipLaunchKernelGGL(sat_cross_kernel, dim3(quads), dim3(256), 0, st, PH, PW, s->bytes[at].p, s->bytes[at ^ 1].p, cnt, pass == c.dilation - 1);
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F2], st));
  const uint8_t* mask = s->bytes[at].p;
  const uint8_t* grown = mask;
  if (const int reach = box_reach(h); reach > 0) {
    hipLaunchKernelGGL(sat_rows_kernel, dim3(pixels), dim3(256), 0, st, PH, PW, reach, mask, s->bytes[at ^ 1].p, cnt);
    hipLaunchKernelGGL(sat_cols_kernel, dim3(pixels), dim3(256), 0, st, PH, PW, reach, s->bytes[at ^ 1].p, s->bytes[2].p, cnt);
    grown = s->bytes[2].p;
  }
  const dim3 tiles((PW + TILE_C - 1) / TILE_C, (PH + TILE_R - 1) / TILE_R);
  hipLaunchKernelGGL(sat_label_tile_kernel, tiles, dim3(TILE_THREADS), TILE_R * TILE_C * sizeof(int), st, grown, PH, PW, s->labels.p, cnt);
  hipLaunchKernelGGL(sat_label_seam_kernel, dim3(blocks_for((long)tiles.x * tiles.y * SEAM_SLOTS)), dim3(256), 0, st, PH, PW, s->labels.p, cnt);
  hipLaunchKernelGGL(sat_label_flatten_kernel, dim3(pixels), dim3(256), 0, st, npix, s->labels.p, cnt);
  hipLaunchKernelGGL(sat_count_kernel, dim3(blocks_for(nseg)), dim3(256), 0, st, PH, PW, s->labels.p, s->segcnt.p, cnt);
  hipLaunchKernelGGL(sat_scan_kernel, dim3(1), dim3(SCAN_THREADS), (SCAN_THREADS + 32) * sizeof(int), st, nseg, s->segcnt.p, s->segoff.p, cnt);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->h_counters.p, cnt, N_COUNTERS * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // the one wait of the route
  s->n_hot = s->h_counters.p[N_HOT], s->n_mask = s->h_counters.p[N_MASK], s->n_groups = s->h_counters.p[N_GROUPS];
  if (s->n_hot == 0) return RPSF_OK;
  if (s->n_groups <= 0 || s->n_mask <= 0) return fail(RPSF_E_HIP, "saturation: hot pixels without a group (internal error)");
  s->mask = mask;
  const long n = s->n_groups;
  s->list_cap = std::min<size_t>((size_t)s->n_mask, (size_t)c.H * c.W);
  HIP_TRY(s->roots.reserve((size_t)n));
  HIP_TRY(s->stats.reserve(GROUP_STATS * (size_t)n));
  HIP_TRY(s->fills.reserve((size_t)s->n_mask));
  HIP_TRY(s->list.reserve(s->list_cap));
  HIP_TRY(s->h_list.reserve(s->list_cap));
  hipLaunchKernelGGL(sat_roots_kernel, dim3(blocks_for(nseg)), dim3(256), 0, st, PH, PW, s->labels.p, s->segoff.p, s->roots.p);
  hipLaunchKernelGGL(sat_group_init_kernel, dim3(blocks_for(n)), dim3(256), 0, st, n, s->stats.p);
  hipLaunchKernelGGL(sat_group_accumulate_kernel, dim3(pixels), dim3(256), 0, st, npix, PW, mask, s->labels.p, s->roots.p, n, s->stats.p);
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F3], st));
  hipLaunchKernelGGL(sat_fill_kernel, dim3((unsigned)n), dim3(FILL_LANES), sizeof(FillLds), st, n, c.reverse_groups ? 1 : 0, PH, PW, h, mask,
                     s->roots.p, s->stats.p, s->padded.p, s->labels.p, s->fills.p, cnt);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F4], st));
  s->timed = true;
  return RPSF_OK;
}

int rpsf_sat_restore(SatDevice* s, const SatCall& c, const float* image_dev, float* out_dev, hipStream_t st) {
  const Padded f{c.H, c.W, c.N, c.H + 4 * c.N, c.W + 4 * c.N, c.pad_mode};
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F5A], st));
  hipLaunchKernelGGL(sat_restore_kernel, dim3(blocks_for((long)c.H * c.W)), dim3(256), 0, st, f, image_dev, s->mask, s->corrected.p, c.out_row0,
                     out_dev, s->list.p, s->counters.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F5B], st));
  s->restored = true;
  return RPSF_OK;
}

int rpsf_sat_list(SatDevice* s, hipStream_t st, const int32_t** list_host, size_t* count) {
  *list_host = nullptr, *count = 0;
  if (!s->mask) return RPSF_OK;
  HIP_TRY(hipMemcpyAsync(s->h_counters.p, s->counters.p, N_COUNTERS * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(s->h_list.p, s->list.p, s->list_cap * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const int n = s->h_counters.p[N_LIST];
  if (n < 0 || (size_t)n > s->list_cap) return fail(RPSF_E_HIP, "saturation: the list of masked pixels is longer than the mask (internal error)");
  *list_host = s->h_list.p, *count = (size_t)n;
  return RPSF_OK;
}

int rpsf_sat_mask(SatDevice* s, const SatCall& c, hipStream_t st, uint8_t* mask_host) {
  const size_t np = (size_t)(c.H + 4 * c.N) * (c.W + 4 * c.N);
  HIP_TRY(hipStreamSynchronize(st));
  if (!s->mask) std::fill(mask_host, mask_host + np, (uint8_t)0);
  else HIP_TRY(hipMemcpy(mask_host, s->mask, np, hipMemcpyDeviceToHost));
  return RPSF_OK;
}

int rpsf_sat_kernel_ms(SatDevice* s, double ms[5]) {
  for (int i = 0; i < 5; ++i) ms[i] = 0.0;
  auto between = [&](int a, int b, double* out) -> int {
    float t = 0;
    HIP_TRY(hipEventSynchronize(s->ev[b]));
    HIP_TRY(hipEventElapsedTime(&t, s->ev[a], s->ev[b]));
    *out = t;
    return RPSF_OK;
  };
  if (!s->ev[SatDevice::E_START]) return RPSF_OK;
  if (const int rc = between(SatDevice::E_START, SatDevice::E_F1, &ms[0])) return rc;
  if (s->timed)
    for (int i = 1; i < 4; ++i)
      if (const int rc = between(SatDevice::E_START + i, SatDevice::E_F1 + i, &ms[i])) return rc;
  if (s->restored)
    if (const int rc = between(SatDevice::E_F5A, SatDevice::E_F5B, &ms[4])) return rc;
  return RPSF_OK;
}

int rpsf_sat_counts(SatDevice* s, int* n_hot, int* n_mask, int* n_groups) {
  *n_hot = s->n_hot, *n_mask = s->n_mask, *n_groups = s->n_groups;
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------ a group of frames
namespace {
Stack stack_of(const SatDevice* s, const SatCall& c) {
  Stack k;
  k.f = Padded{c.H, c.W, c.N, c.H + 4 * c.N, c.W + 4 * c.N, c.pad_mode};
  k.stride = s->b_stride, k.nseg = s->b_nseg;
  k.padded = s->padded.p, k.labels = s->labels.p, k.segcnt = s->segcnt.p, k.segoff = s->segoff.p, k.counters = s->b_counters.p;
  for (int i = 0; i < 3; ++i) k.bytes[i] = s->bytes[i].p;
  return k;
}
}  // namespace

int rpsf_sat_fill_batch(SatDevice* s, const SatCall& c, int frames, const float* images_dev, size_t image_stride, int order_mode, hipStream_t st,
                        float** padded, size_t* p_stride, float** corrected, size_t* c_stride) {
  using namespace rpsfsatb;
  if (frames < 1 || frames > MAX_GROUP_FRAMES) return fail(RPSF_E_BADARG, "saturation: frames per frame-group out of range");
  const int PH = c.H + 4 * c.N, PW = c.W + 4 * c.N, h = c.width / 2;
  const long npix = (long)PH * PW, nseg = (long)PH * segs_per_row(PW);
  const size_t F = (size_t)frames, stride = frame_stride((size_t)npix), cstride = frame_stride((size_t)c.out_rows * PW);
  const size_t n_counters = F * FRAME_COUNTERS + SHARED_COUNTERS;
  s->timed = s->restored = false;
  s->b_frames = 0, s->b_groups = s->b_masked = s->b_listed = 0;
  for (auto& e : s->ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  HIP_TRY(s->padded.reserve(F * stride));
  HIP_TRY(s->corrected.reserve(F * cstride));
  for (auto& b : s->bytes) HIP_TRY(b.reserve(F * stride));
  HIP_TRY(s->labels.reserve(F * stride));
  HIP_TRY(s->segcnt.reserve(F * (size_t)nseg));
  HIP_TRY(s->segoff.reserve(F * (size_t)nseg));
  HIP_TRY(s->b_counters.reserve(n_counters));
  HIP_TRY(s->h_b_counters.reserve(F * FRAME_COUNTERS));
  HIP_TRY(s->b_info.reserve(F * FRAME_INFO));
  HIP_TRY(s->h_b_info.reserve(F * FRAME_INFO));
  s->b_stride = stride, s->b_cstride = cstride, s->b_nseg = (size_t)nseg;
  *padded = s->padded.p, *p_stride = stride, *corrected = s->corrected.p, *c_stride = cstride;
  const Stack k = stack_of(s, c);
  const unsigned fy = (unsigned)frames;
  const dim3 quads(blocks_for((npix + 3) / 4), fy), pixels(blocks_for(npix), fy), segs(blocks_for(nseg), fy);

  HIP_TRY(hipMemsetAsync(s->b_counters.p, 0, n_counters * sizeof(int), st));
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_START], st));
  hipLaunchKernelGGL(sat_pad_batch_kernel, quads, dim3(256), 0, st, k, images_dev, image_stride, c.threshold);
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F1], st));
  int at = 0;
  for (int pass = 0; pass < c.dilation; ++pass, at ^= 1)
    hipLaunchKernelGGL(sat_cross_batch_kernel, quads, dim3(256), 0, st, k, at, pass == c.dilation - 1);
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F2], st));
  int grown = at;
  if (const int reach = box_reach(h); reach > 0) {
    hipLaunchKernelGGL(sat_rows_batch_kernel, pixels, dim3(256), 0, st, k, reach, at);
    hipLaunchKernelGGL(sat_cols_batch_kernel, pixels, dim3(256), 0, st, k, reach, at);
    grown = 2;
  }
  const dim3 tiles((PW + TILE_C - 1) / TILE_C, (PH + TILE_R - 1) / TILE_R, fy);
  hipLaunchKernelGGL(sat_label_tile_batch_kernel, tiles, dim3(TILE_THREADS), TILE_R * TILE_C * sizeof(int), st, k, grown);
  hipLaunchKernelGGL(sat_label_seam_batch_kernel, dim3(blocks_for((long)tiles.x * tiles.y * SEAM_SLOTS), fy), dim3(256), 0, st, k);
  hipLaunchKernelGGL(sat_label_flatten_batch_kernel, pixels, dim3(256), 0, st, k);
  hipLaunchKernelGGL(sat_count_batch_kernel, segs, dim3(256), 0, st, k);
  hipLaunchKernelGGL(sat_scan_batch_kernel, dim3(fy), dim3(SCAN_THREADS), (SCAN_THREADS + 32) * sizeof(int), st, k);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->h_b_counters.p, s->b_counters.p, F * FRAME_COUNTERS * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // the one wait of the frame-group
  if (!plan_tables(s->h_b_counters.p, frames, (size_t)c.H * c.W, s->h_b_info.p, &s->b_groups, &s->b_masked, &s->b_listed))
    return fail(RPSF_E_UNSUPPORTED, "saturation: hot pixels without a group, or 2^31 masked pixels in one frame-group (cut it with RPSF_OPT_SAT_GROUP)");
  s->b_frames = frames, s->b_at = at;
  HIP_TRY(hipMemcpyAsync(s->b_info.p, s->h_b_info.p, F * FRAME_INFO * sizeof(int), hipMemcpyHostToDevice, st));
  if (s->b_groups == 0) return RPSF_OK;  // nothing hot in any frame
  const size_t n = (size_t)s->b_groups;
  HIP_TRY(s->roots.reserve(n));
  HIP_TRY(s->stats.reserve(GROUP_STATS * n));
  HIP_TRY(s->b_gframe.reserve(n));
  HIP_TRY(s->b_order.reserve(n));
  HIP_TRY(s->fills.reserve((size_t)s->b_masked));
  HIP_TRY(s->list.reserve((size_t)s->b_listed));
  HIP_TRY(s->h_list.reserve((size_t)s->b_listed));
  int most = 0;  // groups of one frame
  for (int fr = 0; fr < frames; ++fr) most = std::max(most, s->h_b_info.p[FRAME_INFO * fr + I_GROUPS]);
  const Tables t{s->b_info.p, s->roots.p, s->stats.p, s->b_gframe.p, s->b_order.p, s->b_counters.p + F * FRAME_COUNTERS, s->fills.p, s->b_groups};
  hipLaunchKernelGGL(sat_roots_batch_kernel, segs, dim3(256), 0, st, k, t);
  hipLaunchKernelGGL(sat_group_init_batch_kernel, dim3(blocks_for(most), fy), dim3(256), 0, st, t);
  hipLaunchKernelGGL(sat_group_accumulate_batch_kernel, pixels, dim3(256), 0, st, k, t, at);
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F3], st));
  if (order_mode != ORDER_FRAMES) {
    hipLaunchKernelGGL(sat_order_hist_kernel, dim3(blocks_for(s->b_groups)), dim3(256), 0, st, t);
    hipLaunchKernelGGL(sat_order_scatter_kernel, dim3(blocks_for(s->b_groups)), dim3(256), 0, st, t);
  }
  hipLaunchKernelGGL(sat_fill_batch_kernel, dim3((unsigned)n), dim3(FILL_LANES), sizeof(FillLds), st, k, t, order_mode, at, h);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F4], st));
  s->timed = true;
  return RPSF_OK;
}

int rpsf_sat_restore_batch(SatDevice* s, const SatCall& c, const float* images_dev, size_t image_stride, float* outs_dev, size_t out_stride,
                           hipStream_t st) {
  if (s->b_frames < 1) return fail(RPSF_E_STATE, "saturation: no filled frame-group to restore");
  const Stack k = stack_of(s, c);
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F5A], st));
  hipLaunchKernelGGL(sat_restore_batch_kernel, dim3(blocks_for((long)c.H * c.W), (unsigned)s->b_frames), dim3(256), 0, st, k, s->b_info.p, s->b_at,
                     images_dev, image_stride, s->corrected.p, s->b_cstride, c.out_row0, outs_dev, out_stride, s->list.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F5B], st));
  s->restored = true;
  return RPSF_OK;
}

int rpsf_sat_lists_batch(SatDevice* s, hipStream_t st, const int32_t** list_host, const int** info_host, const int** counters_host) {
  using namespace rpsfsatb;
  *list_host = nullptr, *info_host = s->h_b_info.p, *counters_host = s->h_b_counters.p;
  if (s->b_listed == 0) return RPSF_OK;
  HIP_TRY(hipMemcpyAsync(s->h_b_counters.p, s->b_counters.p, (size_t)s->b_frames * FRAME_COUNTERS * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(s->h_list.p, s->list.p, (size_t)s->b_listed * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int fr = 0; fr < s->b_frames; ++fr) {
    const long n = s->h_b_counters.p[FRAME_COUNTERS * fr + C_LIST];
    const long room = (fr + 1 < s->b_frames ? s->h_b_info.p[FRAME_INFO * (fr + 1) + I_LIST0] : s->b_listed) - s->h_b_info.p[FRAME_INFO * fr + I_LIST0];
    if (n < 0 || n > room) return fail(RPSF_E_HIP, "saturation: a list of masked pixels is longer than its mask (internal error)");
  }
  *list_host = s->h_list.p;
  return RPSF_OK;
}

int rpsf_sat_masks_batch(SatDevice* s, const SatCall& c, hipStream_t st, uint8_t* masks_host) {
  const size_t np = (size_t)(c.H + 4 * c.N) * (c.W + 4 * c.N);
  HIP_TRY(hipStreamSynchronize(st));
  for (int fr = 0; fr < s->b_frames; ++fr) {
    uint8_t* dst = masks_host + fr * np;
    if (s->h_b_counters.p[rpsfsatb::FRAME_COUNTERS * fr + rpsfsatb::C_HOT] == 0) std::fill(dst, dst + np, (uint8_t)0);
    else HIP_TRY(hipMemcpy(dst, s->bytes[s->b_at].p + fr * s->b_stride, np, hipMemcpyDeviceToHost));
  }
  return RPSF_OK;
}

int rpsf_sat_frame_counts(SatDevice* s, int fr, int* n_hot, int* n_mask, int* n_groups) {
  const int* c = s->h_b_counters.p + rpsfsatb::FRAME_COUNTERS * fr;
  const bool hot = c[rpsfsatb::C_HOT] != 0;
  *n_hot = c[rpsfsatb::C_HOT], *n_mask = hot ? c[rpsfsatb::C_MASK] : 0, *n_groups = hot ? c[rpsfsatb::C_GROUPS] : 0;
  return RPSF_OK;
}

void rpsf_sat_batch_totals(SatDevice* s, long* groups, long* masked) { *groups = s->b_groups, *masked = s->b_masked; }
