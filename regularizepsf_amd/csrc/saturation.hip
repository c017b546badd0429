// saturation.hip - the saturation branch of ArrayPSFTransform.apply on the device: what SatRun::prepare / finish of
// rpsf_saturated.hip do on the host, for a frame-group: float32 frames of one shape that are already on the GPU.  A single frame is a
// frame-group of one.  The frame is a grid index (blockIdx.y; the labeller's tiles: blockIdx.z).
//
//   F1  sat_pad_batch_kernel                  2N-padded float32 frames and one hot byte per pixel (value > threshold), hot counts
//       sat_pad_masked_batch_kernel           the masked route's F1: the exact plane as well (the caller's mask through the pad map, non-finite values)
//   F2  sat_cross_batch_kernel x dilation     mask = hot dilated with the cross element (two byte planes in turn), masked counts
//       sat_cross_merge_batch_kernel          the masked route's last pass: mask = dilated | exact
//   F3  sat_rows / sat_cols_batch_kernel      mask grown by a box of reach h / 2, then the star finder's labeller (S3) and root list (S4)
//       sat_group_init / accumulate_batch     per group: masked pixels and their bounding box
//   F4  sat_order_hist / scatter_kernel       the groups of all frames longest first (not run when the table's own order is asked for)
//       sat_fill_batch_kernel                 one wave per group: the sequential nan-mean fill of the group's pixels in raster order
//   F5  sat_restore_batch_kernel              raw values on the mask, crop, list of the masked in-frame pixels per frame
//
// The phases are the drivers of rpsf_core_saturation_batch.hpp, which call the per-thread functions of rpsf_core_saturation.hpp.  Every
// launch goes to the caller's stream; the host waits for it ONCE per frame-group, between the root count and the root list, to size the
// group table.  A frame in which nothing is hot (masked route: and nothing exact) leaves every kernel after F1 at its first instruction,
// and when no frame has such a pixel F4 is not launched.  The only atomics are integer adds / min / max.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "rpsf_core_saturation.hpp"
#include "rpsf_core_saturation_batch.hpp"
#include "rpsf_saturation.hpp"
#include "rpsf_side_unit.hpp"

using namespace rpsfs;
using namespace rpsfsat;
using rpsfsatb::Stack;
using rpsfsatb::Tables;

extern __shared__ __attribute__((aligned(16))) char sat_lds[];

__global__ __launch_bounds__(256) void sat_pad_batch_kernel(Stack s, const float* images, size_t image_stride, double threshold) {
  rpsfsatb::b1_pad(global_id(), (int)blockIdx.y, s, images, image_stride, threshold);
}
__global__ __launch_bounds__(256) void sat_cross_batch_kernel(Stack s, int from, int last) {
  rpsfsatb::b2_cross(global_id(), (int)blockIdx.y, s, from, last);
}
__global__ __launch_bounds__(256) void sat_pad_masked_batch_kernel(Stack s, const float* images, size_t image_stride, double threshold,
                                                                   const MaskView* masks, int fill_nonfinite) {
  rpsfsatb::b1_pad_masked(global_id(), (int)blockIdx.y, s, images, image_stride, threshold, masks, fill_nonfinite);
}
__global__ __launch_bounds__(256) void sat_cross_merge_batch_kernel(Stack s, int from) { rpsfsatb::b2_cross_merge(global_id(), (int)blockIdx.y, s, from); }
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
struct PinnedBuf {  // Buf in page-locked host memory
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
}  // namespace

struct SatDevice {  // the arrays hold the `frames` frames of the last fill, `stride` (corrected: `cstride`) elements apart
  Buf<float> padded, corrected;
  Buf<uint8_t> bytes[3];  // hot / mask in turn, the row-grown and the grown mask
  Buf<uint8_t> exact;     // the masked route: the pixels masked as they are (the caller's mask through the pad map, non-finite values)
  Buf<MaskView> mask_views;  // the masked route: one per frame
  PinnedBuf<MaskView> h_mask_views;
  Buf<int32_t> labels, list;
  Buf<int> segcnt, segoff, roots, stats;
  Buf<int> counters, info, gframe, order;  // FRAME_COUNTERS per frame + SHARED_COUNTERS; FRAME_INFO per frame; per group
  Buf<double> fills;
  PinnedBuf<int> h_counters, h_info;
  PinnedBuf<int32_t> h_list;
  int frames = 0, at = 0;  // bytes[at]: the masks
  size_t stride = 0, cstride = 0, nseg = 0;
  long groups = 0, masked = 0, listed = 0;
  enum { E_START, E_F1, E_F2, E_F3, E_F4, E_F5A, E_F5B, N_EVENTS };
  hipEvent_t ev[N_EVENTS] = {};
  bool timed = false, restored = false;
  ~SatDevice() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

SatDevice* rpsf_sat_create() { return new SatDevice; }
void rpsf_sat_destroy(SatDevice* s) { delete s; }

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

namespace {
Stack stack_of(const SatDevice* s, const SatCall& c) {
  Stack k;
  k.f = Padded{c.H, c.W, c.N, c.H + 4 * c.N, c.W + 4 * c.N, c.pad_mode};
  k.stride = s->stride, k.nseg = s->nseg;
  k.padded = s->padded.p, k.labels = s->labels.p, k.segcnt = s->segcnt.p, k.segoff = s->segoff.p, k.counters = s->counters.p;
  for (int i = 0; i < 3; ++i) k.bytes[i] = s->bytes[i].p;
  return k;
}
}  // namespace

// masked: the route of rpsf_sat_fill_batch_masked (F1's and F2's last pass's variants); masks_host: `frames` views or null
static int fill_batch(SatDevice* s, const SatCall& c, int frames, const float* images_dev, size_t image_stride, bool masked,
                      const MaskView* masks_host, int fill_nonfinite, int order_mode, hipStream_t st, float** padded, size_t* p_stride,
                      float** corrected, size_t* c_stride) {
  using namespace rpsfsatb;
  if (frames < 1 || frames > MAX_GROUP_FRAMES) return fail(RPSF_E_BADARG, "saturation: frames per frame-group out of range");
  const int PH = c.H + 4 * c.N, PW = c.W + 4 * c.N, h = c.width / 2;
  const long npix = (long)PH * PW, nseg = (long)PH * segs_per_row(PW);
  const size_t F = (size_t)frames, stride = frame_stride((size_t)npix), cstride = frame_stride((size_t)c.out_rows * PW);
  const size_t n_counters = F * FRAME_COUNTERS + SHARED_COUNTERS;
  s->timed = s->restored = false;
  s->frames = 0, s->groups = s->masked = s->listed = 0;
  for (auto& e : s->ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  HIP_TRY(s->padded.reserve(F * stride));
  HIP_TRY(s->corrected.reserve(F * cstride));
  for (auto& b : s->bytes) HIP_TRY(b.reserve(F * stride));
  HIP_TRY(s->labels.reserve(F * stride));
  HIP_TRY(s->segcnt.reserve(F * (size_t)nseg));
  HIP_TRY(s->segoff.reserve(F * (size_t)nseg));
  HIP_TRY(s->counters.reserve(n_counters));
  HIP_TRY(s->h_counters.reserve(F * FRAME_COUNTERS));
  HIP_TRY(s->info.reserve(F * FRAME_INFO));
  HIP_TRY(s->h_info.reserve(F * FRAME_INFO));
  if (masked) {
    HIP_TRY(s->exact.reserve(F * stride));
    if (masks_host) {
      HIP_TRY(s->mask_views.reserve(F));
      HIP_TRY(s->h_mask_views.reserve(F));
    }
  }
  s->stride = stride, s->cstride = cstride, s->nseg = (size_t)nseg;
  *padded = s->padded.p, *p_stride = stride, *corrected = s->corrected.p, *c_stride = cstride;
  Stack k = stack_of(s, c);
  k.exact = masked ? s->exact.p : nullptr;
  const unsigned fy = (unsigned)frames;
  const dim3 quads(blocks_for((npix + 3) / 4), fy), pixels(blocks_for(npix), fy), segs(blocks_for(nseg), fy);

  HIP_TRY(hipMemsetAsync(s->counters.p, 0, n_counters * sizeof(int), st));
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_START], st));
  if (masked) {
    if (masks_host) {  // (the pinned copy is free again: every earlier fill waited for its stream after this copy)
      std::copy(masks_host, masks_host + F, s->h_mask_views.p);
      HIP_TRY(hipMemcpyAsync(s->mask_views.p, s->h_mask_views.p, F * sizeof(MaskView), hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(sat_pad_masked_batch_kernel, quads, dim3(256), 0, st, k, images_dev, image_stride, c.threshold,
                       masks_host ? s->mask_views.p : nullptr, fill_nonfinite);
  } else {
    hipLaunchKernelGGL(sat_pad_batch_kernel, quads, dim3(256), 0, st, k, images_dev, image_stride, c.threshold);
  }
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F1], st));
  int at = 0;
  for (int pass = 0; pass < c.dilation; ++pass, at ^= 1) {
    if (masked && pass == c.dilation - 1) hipLaunchKernelGGL(sat_cross_merge_batch_kernel, quads, dim3(256), 0, st, k, at);
    else hipLaunchKernelGGL(sat_cross_batch_kernel, quads, dim3(256), 0, st, k, at, pass == c.dilation - 1);
  }
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
  HIP_TRY(hipMemcpyAsync(s->h_counters.p, s->counters.p, F * FRAME_COUNTERS * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));  // the one wait of the frame-group
  if (!plan_tables(s->h_counters.p, frames, (size_t)c.H * c.W, s->h_info.p, &s->groups, &s->masked, &s->listed))
    return fail(RPSF_E_UNSUPPORTED, "saturation: hot pixels without a group, or 2^31 masked pixels in one frame-group (cut it with RPSF_OPT_SAT_GROUP)");
  s->frames = frames, s->at = at;
  HIP_TRY(hipMemcpyAsync(s->info.p, s->h_info.p, F * FRAME_INFO * sizeof(int), hipMemcpyHostToDevice, st));
  if (s->groups == 0) return RPSF_OK;  // nothing hot in any frame
  const size_t n = (size_t)s->groups;
  HIP_TRY(s->roots.reserve(n));
  HIP_TRY(s->stats.reserve(GROUP_STATS * n));
  HIP_TRY(s->gframe.reserve(n));
  HIP_TRY(s->order.reserve(n));
  HIP_TRY(s->fills.reserve((size_t)s->masked));
  HIP_TRY(s->list.reserve((size_t)s->listed));
  HIP_TRY(s->h_list.reserve((size_t)s->listed));
  int most = 0;  // groups of one frame
  for (int fr = 0; fr < frames; ++fr) most = std::max(most, s->h_info.p[FRAME_INFO * fr + I_GROUPS]);
  const Tables t{s->info.p, s->roots.p, s->stats.p, s->gframe.p, s->order.p, s->counters.p + F * FRAME_COUNTERS, s->fills.p, s->groups};
  hipLaunchKernelGGL(sat_roots_batch_kernel, segs, dim3(256), 0, st, k, t);
  hipLaunchKernelGGL(sat_group_init_batch_kernel, dim3(blocks_for(most), fy), dim3(256), 0, st, t);
  hipLaunchKernelGGL(sat_group_accumulate_batch_kernel, pixels, dim3(256), 0, st, k, t, at);
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F3], st));
  if (order_mode != ORDER_FRAMES) {
    hipLaunchKernelGGL(sat_order_hist_kernel, dim3(blocks_for(s->groups)), dim3(256), 0, st, t);
    hipLaunchKernelGGL(sat_order_scatter_kernel, dim3(blocks_for(s->groups)), dim3(256), 0, st, t);
  }
  hipLaunchKernelGGL(sat_fill_batch_kernel, dim3((unsigned)n), dim3(FILL_LANES), sizeof(FillLds), st, k, t, order_mode, at, h);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F4], st));
  s->timed = true;
  return RPSF_OK;
}

int rpsf_sat_fill_batch(SatDevice* s, const SatCall& c, int frames, const float* images_dev, size_t image_stride, int order_mode, hipStream_t st,
                        float** padded, size_t* p_stride, float** corrected, size_t* c_stride) {
  return fill_batch(s, c, frames, images_dev, image_stride, false, nullptr, 0, order_mode, st, padded, p_stride, corrected, c_stride);
}

int rpsf_sat_fill_batch_masked(SatDevice* s, const SatCall& c, int frames, const float* images_dev, size_t image_stride, const MaskView* masks_host,
                               int fill_nonfinite, int order_mode, hipStream_t st, float** padded, size_t* p_stride, float** corrected,
                               size_t* c_stride) {
  return fill_batch(s, c, frames, images_dev, image_stride, true, masks_host, fill_nonfinite, order_mode, st, padded, p_stride, corrected, c_stride);
}

int rpsf_sat_restore_batch(SatDevice* s, const SatCall& c, const float* images_dev, size_t image_stride, float* outs_dev, size_t out_stride,
                           hipStream_t st) {
  if (s->frames < 1) return fail(RPSF_E_STATE, "saturation: no filled frame-group to restore");
  const Stack k = stack_of(s, c);
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F5A], st));
  hipLaunchKernelGGL(sat_restore_batch_kernel, dim3(blocks_for((long)c.H * c.W), (unsigned)s->frames), dim3(256), 0, st, k, s->info.p, s->at,
                     images_dev, image_stride, s->corrected.p, s->cstride, c.out_row0, outs_dev, out_stride, s->list.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev[SatDevice::E_F5B], st));
  s->restored = true;
  return RPSF_OK;
}

int rpsf_sat_lists_batch(SatDevice* s, hipStream_t st, const int32_t** list_host, const int** info_host, const int** counters_host) {
  using namespace rpsfsatb;
  *list_host = nullptr, *info_host = s->h_info.p, *counters_host = s->h_counters.p;
  if (s->listed == 0) return RPSF_OK;
  HIP_TRY(hipMemcpyAsync(s->h_counters.p, s->counters.p, (size_t)s->frames * FRAME_COUNTERS * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(s->h_list.p, s->list.p, (size_t)s->listed * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (int fr = 0; fr < s->frames; ++fr) {
    const long n = s->h_counters.p[FRAME_COUNTERS * fr + C_LIST];
    const long room = (fr + 1 < s->frames ? s->h_info.p[FRAME_INFO * (fr + 1) + I_LIST0] : s->listed) - s->h_info.p[FRAME_INFO * fr + I_LIST0];
    if (n < 0 || n > room) return fail(RPSF_E_HIP, "saturation: a list of masked pixels is longer than its mask (internal error)");
  }
  *list_host = s->h_list.p;
  return RPSF_OK;
}

int rpsf_sat_masks_batch(SatDevice* s, const SatCall& c, hipStream_t st, uint8_t* masks_host) {
  const size_t np = (size_t)(c.H + 4 * c.N) * (c.W + 4 * c.N);
  HIP_TRY(hipStreamSynchronize(st));
  for (int fr = 0; fr < s->frames; ++fr) {
    uint8_t* dst = masks_host + fr * np;
    if (!Stack::busy(s->h_counters.p + rpsfsatb::FRAME_COUNTERS * fr)) std::fill(dst, dst + np, (uint8_t)0);
    else HIP_TRY(hipMemcpy(dst, s->bytes[s->at].p + fr * s->stride, np, hipMemcpyDeviceToHost));
  }
  return RPSF_OK;
}

int rpsf_sat_frame_counts(SatDevice* s, int fr, int* n_hot, int* n_mask, int* n_groups) {
  const int* c = s->h_counters.p + rpsfsatb::FRAME_COUNTERS * fr;
  const bool hot = Stack::busy(c);
  *n_hot = c[rpsfsatb::C_HOT], *n_mask = hot ? c[rpsfsatb::C_MASK] : 0, *n_groups = hot ? c[rpsfsatb::C_GROUPS] : 0;
  return RPSF_OK;
}

void rpsf_sat_batch_totals(SatDevice* s, long* groups, long* masked) { *groups = s->groups, *masked = s->masked; }
