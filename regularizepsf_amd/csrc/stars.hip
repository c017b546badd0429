// stars.hip - find_stars: star positions for the PSF builder.  The detector is this project's own definition,
// modelled on sep.Background + sep.extract without deblending; it is NOT sep.
//
//   S1  stars_mesh_kernel      one workgroup per background box: sigma-clipped level and rms (exact median, fixed-order sums)
//   S2  stars_detect_kernel    one workgroup per 32 x 32 tile: residual against the bilinear background surface (mesh window and
//                              the tile with a one-pixel halo in LDS), 3 x 3 filter, test against T -> one mask byte per pixel
//   S3  stars_label_*          union-find per tile in LDS, integer atomicMin across tile seams, flatten:
//                              every detected pixel ends with the smallest linear index of its component, the rest with -1
//   S4  stars_count/scan/roots the roots in index order; stars_init/accumulate: area and bounding box by integer atomics;
//       stars_walk_kernel      one wave per component of an accepted area: float64 moments over its bounding box, fixed tree
//
// The phases are the drivers of rpsf_core_stars.hpp.  Launches follow one another on the null stream; no workgroup ever waits for
// another one, and the only atomics are integer min / max / add - labels and moments are the same on every run.
#include <hip/hip_runtime.h>

#include <climits>
#include <string>
#include <vector>

#include "rpsf_core_stars.hpp"
#include "rpsf_side_unit.hpp"

using namespace rpsfs;

extern __shared__ __attribute__((aligned(16))) char stars_lds[];

__global__ __launch_bounds__(S1_THREADS) void stars_mesh_kernel(Frame fr, double* level, double* rms) {
  GpuCtx ctx;
  s1_box(ctx, fr, (int)blockIdx.y, (int)blockIdx.x, stars_lds, level, rms);
}
__global__ __launch_bounds__(TILE_THREADS) void stars_detect_kernel(Frame fr, const double* L, double T, uint8_t* det) {
  GpuCtx ctx;
  s2_tile(ctx, fr, L, T, (int)blockIdx.y, (int)blockIdx.x, stars_lds, det);
}
__global__ __launch_bounds__(TILE_THREADS) void stars_label_tile_kernel(const uint8_t* det, int H, int W, int32_t* labels) {
  GpuCtx ctx;
  s3_tile(ctx, det, H, W, (int)blockIdx.y, (int)blockIdx.x, reinterpret_cast<int*>(stars_lds), labels);
}
__global__ __launch_bounds__(256) void stars_label_seam_kernel(int H, int W, int32_t* labels) { s3_seam(global_id(), H, W, labels); }
__global__ __launch_bounds__(256) void stars_label_flatten_kernel(long npix, int32_t* labels) { s3_flatten(global_id(), npix, labels); }
__global__ __launch_bounds__(256) void stars_count_kernel(int H, int W, const int32_t* labels, int* segcnt) {
  s4_count(global_id(), H, W, labels, segcnt);
}
__global__ __launch_bounds__(SCAN_THREADS) void stars_scan_kernel(long nseg, const int* segcnt, int* segoff, int* total) {
  GpuCtx ctx;
  s4_scan(ctx, nseg, segcnt, segoff, total, reinterpret_cast<int*>(stars_lds));
}
__global__ __launch_bounds__(256) void stars_roots_kernel(int H, int W, const int32_t* labels, const int* segoff, int* roots) {
  s4_roots(global_id(), H, W, labels, segoff, roots);
}
__global__ __launch_bounds__(256) void stars_init_kernel(long count, int W, const int* roots, int* stats) {
  s4_init(global_id(), count, W, roots, stats);
}
__global__ __launch_bounds__(256) void stars_accumulate_kernel(long npix, int W, const int32_t* labels, const int* roots, long count,
                                                               int* stats) {
  s4_accumulate(global_id(), npix, W, labels, roots, count, stats);
}
__global__ __launch_bounds__(WALK_THREADS) void stars_walk_kernel(Frame fr, const double* L, const int32_t* labels, const int* roots,
                                                                  const int* stats, long count, long min_area, long max_area,
                                                                  double* moments) {
  GpuCtx ctx;
  s4_walk(ctx, fr, L, labels, roots, stats, count, min_area, max_area, (long)blockIdx.x * WALK_WAVES, reinterpret_cast<double*>(stars_lds),
          moments);
}

struct rpsf_stars {
  int device = 0, H = 0, W = 0, box = 0, nby = 0, nbx = 0;
  bool have_frame = false;
  Buf<float> frame;
  Buf<uint8_t> mask, det;
  Buf<int32_t> labels;
  Buf<double> level, rms, moments;
  Buf<int> segcnt, segoff, total, roots, stats;
  std::vector<double> found;  // rows (row, col, flux, area) of the last detect
  hipEvent_t ev[2] = {nullptr, nullptr};
  double ms[4] = {0, 0, 0, 0};
  long npix() const { return (long)H * W; }
  long nseg() const { return (long)H * segs_per_row(W); }
  Frame view() const { return Frame{frame.p, mask.p, H, W, box, nby, nbx}; }
  ~rpsf_stars() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// device time of what `launches` enqueues, added to *ms
template <class F>
static int timed(rpsf_stars* s, double* ms, F&& launches) {
  HIP_TRY(hipEventRecord(s->ev[0], nullptr));
  launches();
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev[1], nullptr));
  HIP_TRY(hipEventSynchronize(s->ev[1]));
  float t = 0;
  HIP_TRY(hipEventElapsedTime(&t, s->ev[0], s->ev[1]));
  *ms += t;
  return RPSF_OK;
}

static void launch_label(rpsf_stars* s) {
  const dim3 tiles((s->W + TILE_C - 1) / TILE_C, (s->H + TILE_R - 1) / TILE_R);
  hipLaunchKernelGGL(stars_label_tile_kernel, tiles, dim3(TILE_THREADS), TILE_R * TILE_C * sizeof(int), nullptr, s->det.p, s->H, s->W,
                     s->labels.p);
  hipLaunchKernelGGL(stars_label_seam_kernel, dim3(blocks_for((long)tiles.x * tiles.y * SEAM_SLOTS)), dim3(256), 0, nullptr, s->H, s->W,
                     s->labels.p);
  hipLaunchKernelGGL(stars_label_flatten_kernel, dim3(blocks_for(s->npix())), dim3(256), 0, nullptr, s->npix(), s->labels.p);
}

extern "C" int rpsf_stars_create(rpsf_stars** out, int device, int height, int width, int box) {
  if (!out) return fail(RPSF_E_BADARG, "null argument");
  if (height <= 0 || width <= 0) return fail(RPSF_E_BADARG, "a frame needs positive height and width");
  if (box < MIN_BOX || box > MAX_BOX)
    return fail(RPSF_E_UNSUPPORTED, "background box " + std::to_string(box) + " is outside 8..128");
  if ((long)height * width > INT_MAX) return fail(RPSF_E_UNSUPPORTED, "frames of more than 2^31 - 1 pixels are not supported");
  HIP_TRY(hipSetDevice(device));
  rpsf_stars* s = new rpsf_stars;
  s->device = device, s->H = height, s->W = width, s->box = box;
  s->nby = (height + box - 1) / box, s->nbx = (width + box - 1) / box;
  auto made = [&]() -> int {
    for (auto& e : s->ev) HIP_TRY(hipEventCreate(&e));
    const size_t npix = (size_t)s->npix(), nmesh = (size_t)s->nby * s->nbx;
    HIP_TRY(s->frame.reserve(npix));
    HIP_TRY(s->mask.reserve(npix));
    HIP_TRY(s->det.reserve(npix));
    HIP_TRY(s->labels.reserve(npix));
    HIP_TRY(s->level.reserve(nmesh));
    HIP_TRY(s->rms.reserve(nmesh));
    HIP_TRY(s->segcnt.reserve((size_t)s->nseg()));
    HIP_TRY(s->segoff.reserve((size_t)s->nseg()));
    HIP_TRY(s->total.reserve(1));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&stars_mesh_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)s1_lds_bytes(MAX_BOX)));  // 70 KiB at box = 128
    return RPSF_OK;
  }();
  if (made != RPSF_OK) {
    delete s;
    return made;
  }
  *out = s;
  return RPSF_OK;
}

extern "C" void rpsf_stars_destroy(rpsf_stars* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  delete s;
}

extern "C" int rpsf_stars_background(rpsf_stars* s, const void* image_host, int image_is_f64, const uint8_t* mask_host_or_null,
                                     double* level_host, double* rms_host) {
  if (!s || !image_host || !level_host || !rms_host) return fail(RPSF_E_BADARG, "null argument");
  const size_t npix = (size_t)s->npix(), nmesh = (size_t)s->nby * s->nbx;
  HIP_TRY(hipSetDevice(s->device));
  s->have_frame = false;
  if (image_is_f64) {  // the frame crosses PCIe once, as float32 - what every other path of the library uploads
    std::vector<float> narrow(npix);
    const double* src = static_cast<const double*>(image_host);
    for (size_t i = 0; i < npix; ++i) narrow[i] = (float)src[i];
    HIP_TRY(hipMemcpy(s->frame.p, narrow.data(), npix * sizeof(float), hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemcpy(s->frame.p, image_host, npix * sizeof(float), hipMemcpyHostToDevice));
  }
  if (mask_host_or_null) {
    std::vector<uint8_t> flags(npix);
    for (size_t i = 0; i < npix; ++i) flags[i] = mask_host_or_null[i] != 0;
    HIP_TRY(hipMemcpy(s->mask.p, flags.data(), npix, hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemset(s->mask.p, 0, npix));
  }
  s->ms[0] = 0;
  if (const int rc = timed(s, &s->ms[0], [&] {
        hipLaunchKernelGGL(stars_mesh_kernel, dim3(s->nbx, s->nby), dim3(S1_THREADS), s1_lds_bytes(s->box), nullptr, s->view(), s->level.p,
                           s->rms.p);
      }))
    return rc;
  HIP_TRY(hipMemcpy(level_host, s->level.p, nmesh * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rms_host, s->rms.p, nmesh * sizeof(double), hipMemcpyDeviceToHost));
  s->have_frame = true;
  return RPSF_OK;
}

extern "C" int rpsf_stars_detect(rpsf_stars* s, const double* level_host, double threshold_abs, long min_area, long max_area,
                                 size_t* count) {
  if (!s || !level_host || !count) return fail(RPSF_E_BADARG, "null argument");
  if (!s->have_frame) return fail(RPSF_E_STATE, "rpsf_stars_detect before rpsf_stars_background uploaded a frame");
  const size_t nmesh = (size_t)s->nby * s->nbx;
  for (size_t i = 0; i < nmesh; ++i)
    if (!std::isfinite(level_host[i])) return fail(RPSF_E_BADARG, "the background mesh has a non-finite node");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipMemcpy(s->level.p, level_host, nmesh * sizeof(double), hipMemcpyHostToDevice));
  s->found.clear();
  *count = 0;
  s->ms[1] = s->ms[2] = s->ms[3] = 0;
  const dim3 tiles((s->W + TILE_C - 1) / TILE_C, (s->H + TILE_R - 1) / TILE_R);
  if (const int rc = timed(s, &s->ms[1], [&] {
        hipLaunchKernelGGL(stars_detect_kernel, tiles, dim3(TILE_THREADS), s2_lds_bytes(), nullptr, s->view(), s->level.p, threshold_abs,
                           s->det.p);
      }))
    return rc;
  if (const int rc = timed(s, &s->ms[2], [&] { launch_label(s); })) return rc;
  if (const int rc = timed(s, &s->ms[3], [&] {
        hipLaunchKernelGGL(stars_count_kernel, dim3(blocks_for(s->nseg())), dim3(256), 0, nullptr, s->H, s->W, s->labels.p, s->segcnt.p);
        hipLaunchKernelGGL(stars_scan_kernel, dim3(1), dim3(SCAN_THREADS), (SCAN_THREADS + 32) * sizeof(int), nullptr, s->nseg(),
                           s->segcnt.p, s->segoff.p, s->total.p);
      }))
    return rc;
  int total = 0;
  HIP_TRY(hipMemcpy(&total, s->total.p, sizeof(int), hipMemcpyDeviceToHost));
  if (total <= 0) return RPSF_OK;
  const long n = total;
  HIP_TRY(s->roots.reserve((size_t)n));
  HIP_TRY(s->stats.reserve(4 * (size_t)n));
  HIP_TRY(s->moments.reserve(4 * (size_t)n));
  if (const int rc = timed(s, &s->ms[3], [&] {
        hipLaunchKernelGGL(stars_roots_kernel, dim3(blocks_for(s->nseg())), dim3(256), 0, nullptr, s->H, s->W, s->labels.p, s->segoff.p,
                           s->roots.p);
        hipLaunchKernelGGL(stars_init_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, n, s->W, s->roots.p, s->stats.p);
        hipLaunchKernelGGL(stars_accumulate_kernel, dim3(blocks_for(s->npix())), dim3(256), 0, nullptr, s->npix(), s->W, s->labels.p,
                           s->roots.p, n, s->stats.p);
        hipLaunchKernelGGL(stars_walk_kernel, dim3((unsigned)((n + WALK_WAVES - 1) / WALK_WAVES)), dim3(WALK_THREADS), s4_walk_lds_bytes(),
                           nullptr, s->view(), s->level.p, s->labels.p, s->roots.p, s->stats.p, n, min_area, max_area, s->moments.p);
      }))
    return rc;
  std::vector<double> m(4 * (size_t)n);
  HIP_TRY(hipMemcpy(m.data(), s->moments.p, m.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (long k = 0; k < n; ++k) {  // roots ascend: this is the raster order of each component's first pixel
    const double flux = m[4 * k], area = m[4 * k + 3];
    if (area < (double)min_area || (max_area >= 0 && area > (double)max_area) || !(flux > 0.0)) continue;
    s->found.insert(s->found.end(), {m[4 * k + 1] / flux, m[4 * k + 2] / flux, flux, area});
  }
  *count = s->found.size() / 4;
  return RPSF_OK;
}

extern "C" int rpsf_stars_positions(rpsf_stars* s, size_t first, size_t count, double* out) {
  if (!s || (!out && count)) return fail(RPSF_E_BADARG, "null argument");
  const size_t have = s->found.size() / 4;
  if (first > have || count > have - first) return fail(RPSF_E_BADARG, "range outside the detections of the last rpsf_stars_detect");
  for (size_t i = 0; i < 4 * count; ++i) out[i] = s->found[4 * first + i];
  return RPSF_OK;
}

extern "C" int rpsf_stars_label(rpsf_stars* s, const uint8_t* detected_host, int32_t* labels_host) {
  if (!s || !detected_host || !labels_host) return fail(RPSF_E_BADARG, "null argument");
  const size_t npix = (size_t)s->npix();
  HIP_TRY(hipSetDevice(s->device));
  std::vector<uint8_t> flags(npix);
  for (size_t i = 0; i < npix; ++i) flags[i] = detected_host[i] != 0;
  HIP_TRY(hipMemcpy(s->det.p, flags.data(), npix, hipMemcpyHostToDevice));
  s->ms[2] = 0;
  if (const int rc = timed(s, &s->ms[2], [&] { launch_label(s); })) return rc;
  HIP_TRY(hipMemcpy(labels_host, s->labels.p, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
  return RPSF_OK;
}

extern "C" int rpsf_stars_info(const rpsf_stars* s, int* tile_rows, int* tile_cols) {
  if (!s) return fail(RPSF_E_BADARG, "null argument");
  if (tile_rows) *tile_rows = TILE_R;
  if (tile_cols) *tile_cols = TILE_C;
  return RPSF_OK;
}

extern "C" int rpsf_stars_kernel_ms(const rpsf_stars* s, double ms[4]) {
  if (!s || !ms) return fail(RPSF_E_BADARG, "null argument");
  for (int i = 0; i < 4; ++i) ms[i] = s->ms[i];
  return RPSF_OK;
}
