// rpsf_saturated.hip - the drivers of the saturation branch of apply (regularizepsf/transform.py:117-138,171-177) and the device-array
// views: the host route (every step of the reference on the host, the correction of the padded frame on the GPU), the drivers of the
// device route around csrc/saturation.hip (frame-groups: fill, the plan's shared-K launch, restore) with their test entries, the view entry
// points, which share those drivers, and the sequential host fill (transform.py:135-138).  Launches no kernel of its own: the correction
// is the plan's launch (rpsf.hip: rpsf_detail_launch_apply / rpsf_detail_launch_batch), F1 - F5 are launched by csrc/saturation.hip and C1 / C2 by
// csrc/convert.hip; staging and the worker pool are those of rpsf_host.hip (rpsf_detail_pipe_ensure).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "rpsf_plan.hpp"
#include "rpsf_core_saturation_batch.hpp"
#include "rpsf_convert.hpp"
#include "rpsf_core_convert.hpp"

using rpsf_host::HostPipe;
using rpsf_host::HostPool;

// Python's slice arithmetic for [start, stop) over a length-n axis (a negative bound wraps once): the window rule of the saturation fill
static void py_slice(long start, long stop, long n, long* lo, long* hi) {
  if (start < 0) start = std::max(start + n, 0L);
  if (stop < 0) stop = std::max(stop + n, 0L);
  *lo = std::min(start, n);
  *hi = std::min(stop, n);
}

// ------------------------------------------------------------------------------------------------
// ArrayPSFTransform.apply with a finite saturation threshold, whole (regularizepsf/transform.py:117-138,171-177): float64 copy, np.pad by 2N
// (the mode's index map, evaluated here on the host), mask = padded > threshold, binary dilation with the cross element (`dilation` >= 1
// iterations = a diamond of that radius; scipy treats the outside as background), NaN, the sequential row-major nanmean fill, the correction of
// the PADDED frame on the GPU (corners shifted by 2N, constant padding: exactly what the reference's slices see), raw values restored on the mask,
// crop.  Everything the reference does on the host stays on the host and in its order; what changed against the NumPy / SciPy route of rounds 1-4
// is the cost: no np.pad / astype / copy temporaries (three passes over a (H + 4N)^2 float64 frame), no scipy.ndimage pass over the whole mask for
// a handful of pixels, no device allocation per call, only the rows the patches read and the rows the caller gets cross PCIe.
// A sequence of frames (rpsf_apply_frames_host_saturated - the reference's example corrects a list of frames this way, docs/source/example.ipynb
// cell 25) alternates between two staging slots: the host steps of frame i + 1 run while the GPU corrects frame i.
// ------------------------------------------------------------------------------------------------
// The correction of the 2N-padded frame of an H x W image: rows [r_lo, r_hi) of it are read, rows [o_lo, o_lo + o_rows) written
static int padded_geometry(const rpsf_plan* p, int H, int W, int* r_lo, int* r_hi, int* o_lo, int* o_rows, rpsf_geometry* g) {
  const int N = p->N;
  const long PH = (long)H + 4L * N, PW = (long)W + 4L * N;
  if (PH * PW >= ((long)1 << 31)) return fail(RPSF_E_UNSUPPORTED, "padded frame too large for this entry point");
  // rows of the padded frame the patches read, and the geometry of the correction on it (the hipFFT fallback takes whole frames only)
  *r_lo = p->generic ? 0 : (int)std::max<long>(0, 2L * N + std::min(0, p->corner_min[0]));
  *r_hi = p->generic ? (int)PH : (int)std::min<long>(PH, 2L * N + p->corner_max[0] + N);
  *o_lo = p->generic ? 0 : 2 * N, *o_rows = p->generic ? (int)PH : H;  // output rows the device hands back
  *g = rpsf_geometry{(int)PH, (int)PW, RPSF_PAD_CONSTANT, 0.f, 2 * N, 2 * N, *r_lo, *r_hi - *r_lo, (int)PW, *o_lo, *o_rows, (int)PW};
  return rpsf_detail_check_geometry(p, g);
}

struct SatRun {
  rpsf_plan* p;
  int H, W, N, pad_mode, dilation, width, in_f64, out_f64;
  double threshold;
  long PH, PW;
  int r_lo, r_hi, o_lo, o_rows;
  rpsf_geometry g;
  std::vector<int> colmap;

  int init(rpsf_plan* plan, int height, int w, int mode, double thr, int dil, int nbw, int image_is_f64, int out_is_f64, int slots) {
    p = plan, H = height, W = w, N = plan->N, pad_mode = mode, dilation = dil, width = nbw, in_f64 = image_is_f64, out_f64 = out_is_f64, threshold = thr;
    PH = (long)H + 4L * N, PW = (long)W + 4L * N;
    int rc = padded_geometry(p, H, W, &r_lo, &r_hi, &o_lo, &o_rows, &g);
    if (rc != RPSF_OK) return rc;
    HIP_TRY(hipSetDevice(p->device));
    rc = rpsf_detail_pipe_ensure(p, (size_t)PH * PW, slots);
    if (rc != RPSF_OK) return rc;
    if ((int)p->sat.size() < slots) p->sat.resize(slots);
    colmap.resize(PW);
    for (long c = 0; c < PW; ++c) colmap[c] = pad_index((int)(c - 2L * N), W, pad_mode);
    return RPSF_OK;
  }

  // host steps of one frame into slot s (pad, threshold, dilation, raw values, NaN, sequential fill, narrowing into the pinned staging)
  void prepare(int s, const void* image_host) {
    HostPipe& q = *p->pipe;
    HostPool& pool = HostPool::get(p->device);
    SatScratch& sc = p->sat[s];
    sc.padded.resize((size_t)PH * PW);
    sc.mask.assign((size_t)PH * PW, 0);
    sc.raw.clear();
    double* const padded = sc.padded.data();
    uint8_t* const mask = sc.mask.data();
    const int parts = (int)std::min<long>(PH, (long)pool.width() * 4);
    std::vector<std::vector<int64_t>> hot(parts);  // per part: flat indices of the pixels above the threshold
    // ---- pad (:119-123) + threshold (:129), row blocks in parallel
    pool.run(parts, [&](int part) {
      const long ra = PH * part / parts, rb = PH * (part + 1) / parts;
      for (long r = ra; r < rb; ++r) {
        const int sr = pad_index((int)(r - 2L * N), H, pad_mode);
        double* dst = padded + r * PW;
        if (sr < 0) {
          for (long c = 0; c < PW; ++c) dst[c] = 0.0;  // np.pad(mode="constant") pads with 0
        } else if (in_f64) {
          const double* src = static_cast<const double*>(image_host) + (size_t)sr * W;
          for (long c = 0; c < PW; ++c) dst[c] = colmap[c] < 0 ? 0.0 : src[colmap[c]];
        } else {
          const float* src = static_cast<const float*>(image_host) + (size_t)sr * W;
          for (long c = 0; c < PW; ++c) dst[c] = colmap[c] < 0 ? 0.0 : (double)src[colmap[c]];
        }
        for (long c = 0; c < PW; ++c)
          if (dst[c] > threshold) hot[part].push_back(r * PW + c);
      }
    });
    // ---- dilation (:133): every pixel within `dilation` city-block steps of a saturated one
    std::vector<uint8_t> row_has(PH, 0);
    size_t n_hot = 0;
    for (const auto& list : hot) {
      n_hot += list.size();
      for (const int64_t idx : list) {
        const long r = idx / PW, c = idx % PW;
        for (long dr = -dilation; dr <= dilation; ++dr) {
          const long rr = r + dr;
          if (rr < 0 || rr >= PH) continue;
          const long span = dilation - std::labs(dr);
          const long c0 = std::max<long>(0, c - span), c1 = std::min<long>(PW - 1, c + span);
          std::memset(mask + rr * PW + c0, 1, (size_t)(c1 - c0 + 1));
          row_has[rr] = 1;
        }
      }
    }
    // ---- raw values of the masked pixels the caller will see (:126, :172), NaN (:134), sequential fill (:135-138)
    if (n_hot) {
      for (long r = 0; r < PH; ++r) {
        if (!row_has[r]) continue;
        for (long c = 0; c < PW; ++c)
          if (mask[r * PW + c]) {
            if (r >= 2L * N && r < 2L * N + H && c >= 2L * N && c < 2L * N + W) sc.raw.push_back({r * PW + c, padded[r * PW + c]});
            padded[r * PW + c] = std::nan("");
          }
      }
      const long hw = width / 2;
      for (long i = 0; i < PH; ++i) {
        if (!row_has[i]) continue;
        for (long j = 0; j < PW; ++j) {
          if (!mask[i * PW + j]) continue;
          long r0, r1, c0, c1;
          py_slice(i - hw, i + hw, PH, &r0, &r1);
          py_slice(j - hw, j + hw, PW, &c0, &c1);
          double sum = 0.0;
          long cnt = 0;
          for (long r = r0; r < r1; ++r)
            for (long c = c0; c < c1; ++c) {
              const double v = padded[r * PW + c];
              if (v == v) sum += v, ++cnt;
            }
          padded[i * PW + j] = cnt ? sum / (double)cnt : std::nan("");
        }
      }
    }
    const size_t in_lo = (size_t)r_lo * PW, in_hi = (size_t)r_hi * PW;
    const int T = rpsf_detail_host_parts_for((in_hi - in_lo) * sizeof(float));
    pool.run(T, [&](int t) {
      size_t a, b;
      rpsf_host::split_range(in_lo, in_hi, t, T, a, b);
      rpsf_host::narrow_or_copy(q.h_in[s], padded, true, a, b);
    });
  }

  // the correction of the padded frame of slot s: rows the patches read in, the caller's rows out; asynchronous on the plan's stream
  hipError_t enqueue(int s) {
    HostPipe& q = *p->pipe;
    const size_t in_lo = (size_t)r_lo * PW, in_hi = (size_t)r_hi * PW, out_lo = (size_t)o_lo * PW, out_hi = out_lo + (size_t)o_rows * PW;
    hipError_t err = hipMemcpyAsync(q.d_in[s], q.h_in[s] + in_lo, (in_hi - in_lo) * sizeof(float), hipMemcpyHostToDevice, p->stream);
    if (err == hipSuccess && rpsf_detail_launch_apply(p, q.d_in[s], q.d_out[s], g, p->stream, nullptr) != RPSF_OK) err = hipErrorUnknown;
    if (err == hipSuccess) err = hipMemcpyAsync(q.h_out[s] + out_lo, q.d_out[s], (out_hi - out_lo) * sizeof(float), hipMemcpyDeviceToHost, p->stream);
    if (err == hipSuccess) err = hipEventRecord(q.ev_out[s], p->stream);
    return err;
  }

  // wait for slot s, then the crop (:174-177) with the raw values back on the mask (:172)
  hipError_t finish(int s, void* out_host) {
    HostPipe& q = *p->pipe;
    HostPool& pool = HostPool::get(p->device);
    hipError_t err = hipEventSynchronize(q.ev_out[s]);
    if (err != hipSuccess) return err;
    const int rows_parts = std::min(H, pool.width() * 4);
    pool.run(rows_parts, [&](int part) {
      const long ra = (long)H * part / rows_parts, rb = (long)H * (part + 1) / rows_parts;
      for (long r = ra; r < rb; ++r) {
        const float* src = q.h_out[s] + (size_t)(2 * N + r) * PW + 2 * N;  // (h_out is indexed by rows of the padded frame)
        if (out_f64) {
          double* dst = static_cast<double*>(out_host) + (size_t)r * W;
          for (long c = 0; c < W; ++c) dst[c] = (double)src[c];
        } else {
          std::memcpy(static_cast<float*>(out_host) + (size_t)r * W, src, (size_t)W * sizeof(float));
        }
      }
    });
    for (const SatScratch::Raw& x : p->sat[s].raw) {
      const long r = x.idx / PW - 2L * N, c = x.idx % PW - 2L * N;
      if (out_f64) static_cast<double*>(out_host)[(size_t)r * W + c] = x.value;
      else static_cast<float*>(out_host)[(size_t)r * W + c] = (float)x.value;
    }
    return hipSuccess;
  }
};

static int check_saturated_call(rpsf_plan* p, const void* a, const void* b, int height, int width, int pad_mode, int dilation, int neighborhood_width) {
  if (!p || !a || !b) return fail(RPSF_E_BADARG, "null argument");
  if (height <= 0 || width <= 0) return fail(RPSF_E_BADARG, "image shape must be positive");
  if (pad_mode < 0 || pad_mode > RPSF_PAD_WRAP) return fail(RPSF_E_BADARG, "unknown pad mode");
  if (dilation < 1 || neighborhood_width < 0) return fail(RPSF_E_BADARG, "dilation must be >= 1 and the neighbourhood width >= 0 (other values: the NumPy route)");
  if (!p->have_k) return fail(RPSF_E_STATE, "no transfer kernel installed (call rpsf_plan_set_transfer first)");
  // every saturation and mask entry point: the plan's launch lanes are joined first (rpsf_lanes.hpp), and an error word nobody collected is not
  // this call's
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;
  rpsf_detail_clear_error(p);
  return RPSF_OK;
}

extern "C" int rpsf_apply_host_saturated(rpsf_plan* p, const void* image_host, int image_is_f64, int height, int width, int pad_mode,
                                         double threshold, int dilation, int neighborhood_width, void* out_host, int out_is_f64) {
  int rc = check_saturated_call(p, image_host, out_host, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  SatRun run;
  rc = run.init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, image_is_f64, out_is_f64, 1);
  if (rc != RPSF_OK) return rc;
  run.prepare(0, image_host);
  hipError_t err = run.enqueue(0);
  if (err == hipSuccess) err = run.finish(0, out_host);
  if (err != hipSuccess) return rpsf_detail_drain_after_error(p, err, "saturated host frame");
  return rpsf_detail_sweep_check(p);
}

extern "C" int rpsf_apply_frames_host_saturated(rpsf_plan* p, const void* const* images_host, int image_is_f64, int n_frames, int height, int width,
                                                int pad_mode, double threshold, int dilation, int neighborhood_width, void* const* outs_host,
                                                int out_is_f64) {
  int rc = check_saturated_call(p, images_host, outs_host, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  if (n_frames <= 0) return fail(RPSF_E_BADARG, "n_frames must be positive");
  for (int f = 0; f < n_frames; ++f)
    if (!images_host[f] || !outs_host[f]) return fail(RPSF_E_BADARG, "null frame pointer");
  SatRun run;
  rc = run.init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, image_is_f64, out_is_f64, std::min(2, n_frames));
  if (rc != RPSF_OK) return rc;
  hipError_t err = hipSuccess;
  for (int f = 0; f < n_frames && err == hipSuccess; ++f) {
    run.prepare(f & 1, images_host[f]);  // (the slot's previous frame, f - 2, was finished in the iteration before)
    err = run.enqueue(f & 1);
    if (err == hipSuccess && f > 0) err = run.finish((f - 1) & 1, outs_host[f - 1]);  // the GPU has had the host steps of frame f to correct frame f - 1
  }
  if (err == hipSuccess) err = run.finish((n_frames - 1) & 1, outs_host[n_frames - 1]);
  if (err != hipSuccess) return rpsf_detail_drain_after_error(p, err, "saturated host frames");
  return rpsf_detail_sweep_check(p);
}

// ------------------------------------------------------------------------------------------------
// The same branch with every step on the device (csrc/saturation.hip, csrc/rpsf_core_saturation_batch.hpp): frames of one
// shape are cut into frame-groups; per frame-group F1 - F3 with the frame as a grid index build the filled padded frames from the
// resident H x W frames, one wait, one F4 launch, the shared-K batch launch corrects the padded frames with the geometry above, one F5
// launch restores and crops.  A single frame is a frame-group of one whose F4 takes the groups in the table's own order.
// ------------------------------------------------------------------------------------------------
struct SatDeviceRun {
  SatCall call;
  rpsf_geometry g;
  int r_lo, r_hi;
};

static int sat_device_init(rpsf_plan* p, int height, int width, int pad_mode, double threshold, int dilation, int neighborhood_width,
                           SatDeviceRun* run) {
  if (neighborhood_width / 2 < 1) return fail(RPSF_E_BADARG, "the device route needs neighborhood_width // 2 >= 1 (an always-empty window: the host route)");
  int o_lo, o_rows;
  const int rc = padded_geometry(p, height, width, &run->r_lo, &run->r_hi, &o_lo, &o_rows, &run->g);
  if (rc != RPSF_OK) return rc;
  run->call = SatCall{height, width, p->N, pad_mode, dilation, neighborhood_width, threshold, run->r_lo, o_lo, o_rows};
  HIP_TRY(hipSetDevice(p->device));
  if (!p->sat_dev) p->sat_dev.reset(rpsf_sat_create());
  return RPSF_OK;
}

// What rpsf_saturation_batch_info reports: the frames entry points store it, a single-frame call keeps its own and stores nothing
struct SatBatchStats {
  long frames = 0, frame_groups = 0, groups = 0, masked = 0;
  void store(rpsf_plan* p) const {
    const long v[4] = {frames, frame_groups, groups, masked};
    for (int i = 0; i < 4; ++i) p->sat_batch_info[i] = (int)std::min<long>(v[i], 0x7FFFFFFF);
  }
};

// The bad-pixel masks of a masked call ("Bad-pixel masks"): uint8 views in device memory - none, one for every frame or
// one per frame - and whether the non-finite values of the padded frame are masked too
struct SatMasks {
  const rpsf_view* views = nullptr;
  int n = 0;
  int fill_nonfinite = 0;
};

static int check_masks(const SatMasks& m, int n_frames, int height, int width) {
  if (m.n < 0 || (m.n > 0 && !m.views)) return fail(RPSF_E_BADARG, "mask: null views");
  if (m.n > 1 && m.n != n_frames) return fail(RPSF_E_BADARG, "mask: no mask, one mask or one mask per frame");
  for (int f = 0; f < m.n; ++f) {
    const rpsf_view& v = m.views[f];
    if (v.dtype != RPSF_DTYPE_UINT8) return fail(RPSF_E_BADARG, "mask: views must be uint8");
    if (v.rows != height || v.cols != width) return fail(RPSF_E_BADARG, "mask: every mask must have the frame's shape");
    if (!v.data || v.row_stride <= 0 || v.col_stride <= 0) return fail(RPSF_E_BADARG, "mask: null data or a stride that is not positive");
  }
  return RPSF_OK;
}

// the kernel's views of frames f0 ... f0 + frames - 1 (empty: the call has no mask)
static std::vector<rpsfsat::MaskView> group_views(const SatMasks& m, int f0, int frames) {
  std::vector<rpsfsat::MaskView> views(m.n ? (size_t)frames : 0);
  for (int f = 0; f < (int)views.size(); ++f) {
    const rpsf_view& v = m.views[m.n == 1 ? 0 : f0 + f];
    views[f] = rpsfsat::MaskView{static_cast<const uint8_t*>(v.data), (long)v.row_stride, (long)v.col_stride};
  }
  return views;
}

static int sat_group_frames(const rpsf_plan* p, const SatDeviceRun& run, bool masked = false) {
  if (p->sat_group_opt > 0) return p->sat_group_opt;
  return rpsfsatb::auto_group_frames((size_t)run.g.height * run.g.width, (size_t)run.call.out_rows * run.g.width, masked);
}

// one frame-group, resident; asynchronous on st but for the one wait inside rpsf_sat_fill_batch.  masks: null on the unmasked route,
// else the call's masks and f0, the group's first frame among the call's
static int sat_device_apply_group(rpsf_plan* p, const SatDeviceRun& run, int frames, const float* images_dev, size_t image_stride, float* outs_dev,
                                  size_t out_stride, int order, hipStream_t st, SatBatchStats* stats, size_t* n_masked_or_null,
                                  const SatMasks* masks = nullptr, int f0 = 0) {
  float *padded = nullptr, *corrected = nullptr;
  size_t p_stride = 0, c_stride = 0;
  SatDevice* sd = p->sat_dev.get();
  int rc;
  if (!masks) {
    rc = rpsf_sat_fill_batch(sd, run.call, frames, images_dev, image_stride, order, st, &padded, &p_stride, &corrected, &c_stride);
  } else {
    const std::vector<rpsfsat::MaskView> views = group_views(*masks, f0, frames);
    rc = rpsf_sat_fill_batch_masked(sd, run.call, frames, images_dev, image_stride, views.empty() ? nullptr : views.data(), masks->fill_nonfinite,
                                    order, st, &padded, &p_stride, &corrected, &c_stride);
  }
  if (rc != RPSF_OK) return rc;
  rc = rpsf_detail_launch_batch(p, padded + (size_t)run.r_lo * run.g.width, corrected, frames, p_stride, c_stride, run.g, st);
  if (rc != RPSF_OK) return rc;
  rc = rpsf_sat_restore_batch(sd, run.call, images_dev, image_stride, outs_dev, out_stride, st);
  if (rc != RPSF_OK) return rc;
  long groups = 0, masked = 0;
  rpsf_sat_batch_totals(sd, &groups, &masked);
  stats->frame_groups += 1, stats->groups += groups, stats->masked += masked;
  for (int f = 0; n_masked_or_null && f < frames; ++f) {
    int n_hot, n_mask, n_groups;
    rpsf_sat_frame_counts(sd, f, &n_hot, &n_mask, &n_groups);
    n_masked_or_null[f] = (size_t)n_mask;
  }
  return RPSF_OK;
}

// one frame-group of host arrays through the plan's staging slot 0 (room for `frames` frames: pipe_ensure): staged as float32, uploaded,
// sat_device_apply_group, downloaded, widened; T: parts of the host pool's copies
static int sat_host_group(rpsf_plan* p, const SatDeviceRun& run, int frames, const void* const* images_host, int image_is_f64, void* const* outs_host,
                          int out_is_f64, int order, int T, SatBatchStats* stats, const SatMasks* group_masks = nullptr) {
  const size_t npix = (size_t)run.call.H * run.call.W, total = npix * frames;
  HostPipe& q = *p->pipe;
  HostPool& pool = HostPool::get(p->device);
  pool.run(T, [&](int t) {  // the group's frames laid end to end, cut into T parts
    size_t a, b;
    rpsf_host::split_range(0, total, t, T, a, b);
    while (a < b) {
      const size_t f = a / npix, lo = a % npix, hi = std::min(npix, lo + (b - a));
      rpsf_host::narrow_or_copy(q.h_in[0] + f * npix, images_host[f], image_is_f64 != 0, lo, hi);
      a += hi - lo;
    }
  });
  hipError_t err = hipMemcpyAsync(q.d_in[0], q.h_in[0], total * sizeof(float), hipMemcpyHostToDevice, p->stream);
  if (err != hipSuccess) return rpsf_detail_drain_after_error(p, err, "saturated host frames, device route");
  int rc = sat_device_apply_group(p, run, frames, q.d_in[0], npix, q.d_out[0], npix, order, p->stream, stats, nullptr, group_masks, 0);
  if (rc != RPSF_OK) {
    (void)hipStreamSynchronize(p->stream);
    return rc;
  }
  err = hipMemcpyAsync(q.h_out[0], q.d_out[0], total * sizeof(float), hipMemcpyDeviceToHost, p->stream);
  if (err != hipSuccess) return rpsf_detail_drain_after_error(p, err, "saturated host frames, device route");
  const int32_t* list = nullptr;
  const int *info = nullptr, *counters = nullptr;
  rc = rpsf_sat_lists_batch(p->sat_dev.get(), p->stream, &list, &info, &counters);  // waits for the stream when there is a list
  if (rc != RPSF_OK) {
    (void)hipStreamSynchronize(p->stream);
    return rc;
  }
  if (!list) {
    err = hipStreamSynchronize(p->stream);
    if (err != hipSuccess) return rpsf_detail_drain_after_error(p, err, "saturated host frames, device route");
  }
  pool.run(T, [&](int t) {
    size_t a, b;
    rpsf_host::split_range(0, total, t, T, a, b);
    while (a < b) {
      const size_t f = a / npix, lo = a % npix, hi = std::min(npix, lo + (b - a));
      rpsf_host::widen_or_copy(outs_host[f], out_is_f64 != 0, q.h_out[0] + f * npix, lo, hi);
      a += hi - lo;
    }
  });
  if (image_is_f64 && list) {  // the caller's own values on the mask, not their float32 roundings
    for (int f = 0; f < frames; ++f) {
      const double* src = static_cast<const double*>(images_host[f]);
      const int32_t* mine = list + info[rpsfsatb::FRAME_INFO * f + rpsfsatb::I_LIST0];
      const int n = rpsfsatb::Stack::busy(counters + rpsfsatb::FRAME_COUNTERS * f) ? counters[rpsfsatb::FRAME_COUNTERS * f + rpsfsatb::C_LIST] : 0;
      for (int k = 0; k < n; ++k) {
        if (out_is_f64) static_cast<double*>(outs_host[f])[mine[k]] = src[mine[k]];
        else static_cast<float*>(outs_host[f])[mine[k]] = (float)src[mine[k]];
      }
    }
  }
  return RPSF_OK;
}

extern "C" int rpsf_apply_device_saturated(rpsf_plan* p, const void* image_dev, void* out_dev, int height, int width, int pad_mode, double threshold,
                                           int dilation, int neighborhood_width, void* stream, size_t* n_masked_or_null) {
  int rc = check_saturated_call(p, image_dev, out_dev, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  SatDeviceRun run;
  rc = sat_device_init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, &run);
  if (rc != RPSF_OK) return rc;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : p->stream;
  const size_t npix = (size_t)height * width;
  SatBatchStats stats;
  return sat_device_apply_group(p, run, 1, static_cast<const float*>(image_dev), npix, static_cast<float*>(out_dev), npix, rpsfsatb::ORDER_FRAMES, st,
                                &stats, n_masked_or_null);
}

extern "C" int rpsf_apply_host_saturated_device(rpsf_plan* p, const void* image_host, int image_is_f64, int height, int width, int pad_mode,
                                                double threshold, int dilation, int neighborhood_width, void* out_host, int out_is_f64) {
  int rc = check_saturated_call(p, image_host, out_host, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  SatDeviceRun run;
  rc = sat_device_init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, &run);
  if (rc != RPSF_OK) return rc;
  const size_t npix = (size_t)height * width;
  rc = rpsf_detail_pipe_ensure(p, npix, 1);
  if (rc != RPSF_OK) return rc;
  SatBatchStats stats;
  rc = sat_host_group(p, run, 1, &image_host, image_is_f64, &out_host, out_is_f64, rpsfsatb::ORDER_FRAMES, rpsf_detail_host_parts_for(npix * sizeof(float)), &stats);
  return rc != RPSF_OK ? rc : rpsf_detail_sweep_check(p);
}

extern "C" int rpsf_apply_batch_device_saturated(rpsf_plan* p, const void* images_dev, void* outs_dev, int n_frames, size_t image_stride,
                                                 size_t out_stride, int height, int width, int pad_mode, double threshold, int dilation,
                                                 int neighborhood_width, void* stream, size_t* n_masked_per_frame_or_null) {
  if (p && n_frames == 0) {
    SatBatchStats().store(p);
    return RPSF_OK;
  }
  int rc = check_saturated_call(p, images_dev, outs_dev, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  if (n_frames < 0) return fail(RPSF_E_BADARG, "n_frames must not be negative");
  if (n_frames > 1 && (image_stride < (size_t)height * width || out_stride < (size_t)height * width))
    return fail(RPSF_E_BADARG, "frame stride smaller than one frame");
  SatDeviceRun run;
  rc = sat_device_init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, &run);
  if (rc != RPSF_OK) return rc;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : p->stream;
  const int G = sat_group_frames(p, run);
  SatBatchStats stats;
  stats.frames = n_frames;
  for (int f0 = 0; f0 < n_frames; f0 += G) {
    rc = sat_device_apply_group(p, run, std::min(G, n_frames - f0), static_cast<const float*>(images_dev) + (size_t)f0 * image_stride, image_stride,
                                static_cast<float*>(outs_dev) + (size_t)f0 * out_stride, out_stride, rpsfsatb::ORDER_LONGEST_FIRST, st, &stats,
                                n_masked_per_frame_or_null ? n_masked_per_frame_or_null + f0 : nullptr);
    if (rc != RPSF_OK) return rc;
  }
  stats.store(p);
  return RPSF_OK;
}

extern "C" int rpsf_apply_frames_host_saturated_device(rpsf_plan* p, const void* const* images_host, int image_is_f64, int n_frames, int height,
                                                       int width, int pad_mode, double threshold, int dilation, int neighborhood_width,
                                                       void* const* outs_host, int out_is_f64) {
  if (p && n_frames == 0) {
    SatBatchStats().store(p);
    return RPSF_OK;
  }
  int rc = check_saturated_call(p, images_host, outs_host, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  if (n_frames < 0) return fail(RPSF_E_BADARG, "n_frames must not be negative");
  for (int f = 0; f < n_frames; ++f)
    if (!images_host[f] || !outs_host[f]) return fail(RPSF_E_BADARG, "null frame pointer");
  SatDeviceRun run;
  rc = sat_device_init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, &run);
  if (rc != RPSF_OK) return rc;
  const size_t npix = (size_t)height * width;
  const int G = std::min(sat_group_frames(p, run), n_frames);
  rc = rpsf_detail_pipe_ensure(p, npix * G, 1);
  if (rc != RPSF_OK) return rc;
  const int T = rpsf_detail_host_parts_for(npix * G * sizeof(float));
  SatBatchStats stats;
  stats.frames = n_frames;
  for (int f0 = 0; f0 < n_frames; f0 += G) {
    rc = sat_host_group(p, run, std::min(G, n_frames - f0), images_host + f0, image_is_f64, outs_host + f0, out_is_f64, rpsfsatb::ORDER_LONGEST_FIRST, T,
                        &stats);
    if (rc != RPSF_OK) return rc;
  }
  stats.store(p);
  return rpsf_detail_sweep_check(p);
}

// ------------------------------------------------------------------------------------------------
// Device-array views (include/rpsf.h, rpsf_view): a side that is what rpsf_geometry describes goes into the launch as it is, any other
// through the plan's staging and kernel C1 / C2 (csrc/convert.hip; predicate and checks: csrc/rpsf_core_convert.hpp)
// ------------------------------------------------------------------------------------------------
// One side of a call: `n` views of one shape.  direct: every view zero copy (dense, for the saturation route), one row stride, evenly
// spaced by a positive multiple of 4 bytes that holds a frame.  uniform: one dtype, one pair of strides, evenly spaced - one C1 / C2 launch.
struct ViewSide {
  bool direct = true, uniform = true;
  int64_t frame_bytes = 0;
};
static ViewSide view_side(const rpsf_view* v, int n, bool need_dense) {
  ViewSide s;
  s.frame_bytes = n > 1 ? static_cast<char*>(v[1].data) - static_cast<char*>(v[0].data) : 0;
  for (int f = 0; f < n; ++f) {
    if (!(need_dense ? rpsfconv::dense_f32(v[f]) : rpsfconv::zero_copy(v[f]))) s.direct = false;
    if (v[f].dtype != v[0].dtype || v[f].row_stride != v[0].row_stride || v[f].col_stride != v[0].col_stride ||
        static_cast<char*>(v[f].data) - static_cast<char*>(v[0].data) != (int64_t)f * s.frame_bytes)
      s.direct = s.uniform = false;
  }
  if (n > 1 && (s.frame_bytes <= 0 || s.frame_bytes % 4 || s.frame_bytes < (int64_t)(v[0].rows - 1) * v[0].row_stride + 4 * (int64_t)v[0].cols))
    s.direct = false;
  return s;
}

static int view_staging(DevBuf<float>& buf, size_t& cap, size_t floats) {
  if (floats <= cap) return RPSF_OK;
  HIP_TRY(hipDeviceSynchronize());  // earlier calls, on whatever stream, may still use the old staging
  cap = 0;
  HIP_TRY(buf.alloc(floats));
  cap = floats;
  return RPSF_OK;
}

static int apply_views(rpsf_plan* p, const rpsf_view* images, const rpsf_view* outs, int n, int pad_mode, float pad_value, double threshold, int dilation,
                       int neighborhood_width, void* stream, int* route_or_null, bool batch, const SatMasks* masks = nullptr) {
  if (route_or_null) *route_or_null = 0;
  if (!p) return fail(RPSF_E_BADARG, "null plan");
  if (n < 0) return fail(RPSF_E_BADARG, "n_frames must not be negative");
  if (n == 0) return RPSF_OK;
  if (!images || !outs) return fail(RPSF_E_BADARG, "null argument");
  bool empty = false;
  for (int f = 0; f < n; ++f) {
    bool e_in, e_out;
    if (const char* why = rpsfconv::view_problem(images + f, false, &e_in)) return fail(RPSF_E_BADARG, std::string("image: ") + why);
    if (const char* why = rpsfconv::view_problem(outs + f, true, &e_out)) return fail(RPSF_E_BADARG, std::string("out: ") + why);
    if (images[f].rows != images[0].rows || images[f].cols != images[0].cols || outs[f].rows != images[0].rows || outs[f].cols != images[0].cols)
      return fail(RPSF_E_BADARG, "every image and every out view must have one shape");
    empty = e_in;
  }
  if (empty) return RPSF_OK;
  if (pad_mode < 0 || pad_mode > RPSF_PAD_WRAP) return fail(RPSF_E_BADARG, "unknown pad mode");
  if (!p->have_k) return fail(RPSF_E_STATE, "no transfer kernel installed (call rpsf_plan_set_transfer first)");
  const int H = images[0].rows, W = images[0].cols;
  const bool saturated = masks || !(threshold == std::numeric_limits<double>::infinity());  // (a masked call takes the route whatever the threshold)
  if (masks)
    if (const int bad = check_masks(*masks, n, H, W)) return bad;
  const ViewSide in = view_side(images, n, saturated), out = view_side(outs, n, saturated);
  rpsf_geometry g{H, W, pad_mode, pad_value, 0, 0, 0, H, in.direct ? (int)(images[0].row_stride / 4) : W, 0, H, out.direct ? (int)(outs[0].row_stride / 4) : W};
  SatDeviceRun run;
  int rc;
  if (saturated) {
    if (dilation < 1 || neighborhood_width < 0) return fail(RPSF_E_BADARG, "dilation must be >= 1 and the neighbourhood width >= 0 (other values: the NumPy route)");
    rc = sat_device_init(p, H, W, pad_mode, threshold, dilation, neighborhood_width, &run);
  } else {
    rc = rpsf_detail_check_geometry(p, &g);
  }
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;  // (device-array views: conversions and copies run on the public stream around the apply)
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : p->stream;
  const size_t npix = (size_t)H * W, stage_stride = (npix + 3) / 4 * 4;  // (every staged frame starts on 16 bytes)
  const bool staged = !in.direct || !out.direct;
  if (!in.direct && (rc = view_staging(p->d_view_in, p->view_in_floats, stage_stride * n)) != RPSF_OK) return rc;
  if (!out.direct && (rc = view_staging(p->d_view_out, p->view_out_floats, stage_stride * n)) != RPSF_OK) return rc;
  if (staged) {  // the staging serves one call at a time: a call on another stream waits, on the device, for the last one that used it
    if (!p->ev_view) HIP_TRY(hipEventCreateWithFlags(&p->ev_view, hipEventDisableTiming));
    if (p->view_busy && st != p->view_stream) HIP_TRY(hipStreamWaitEvent(st, p->ev_view, 0));
  }
  const float* d_in = static_cast<const float*>(images[0].data);
  float* d_out = static_cast<float*>(outs[0].data);
  size_t in_stride = (size_t)(in.frame_bytes / 4), out_stride = (size_t)(out.frame_bytes / 4);
  if (!in.direct) {
    if (in.uniform) rc = rpsf_conv_gather(images[0], n, in.frame_bytes, p->d_view_in, (int64_t)stage_stride, st);
    for (int f = 0; !in.uniform && f < n && rc == RPSF_OK; ++f) rc = rpsf_conv_gather(images[f], 1, 0, p->d_view_in + f * stage_stride, 0, st);
    if (rc != RPSF_OK) return rc;
    d_in = p->d_view_in, in_stride = stage_stride;
  }
  if (!out.direct) d_out = p->d_view_out, out_stride = stage_stride;
  if (!saturated) {
    rc = rpsf_detail_launch_batch(p, d_in, d_out, n, in_stride, out_stride, g, st);
  } else {
    const int G = batch ? sat_group_frames(p, run, masks != nullptr) : 1;
    SatBatchStats stats;
    stats.frames = n;
    for (int f0 = 0; f0 < n && rc == RPSF_OK; f0 += G)
      rc = sat_device_apply_group(p, run, std::min(G, n - f0), d_in + (size_t)f0 * in_stride, in_stride, d_out + (size_t)f0 * out_stride, out_stride,
                                  batch ? rpsfsatb::ORDER_LONGEST_FIRST : rpsfsatb::ORDER_FRAMES, st, &stats, nullptr, masks, f0);
    if (batch && rc == RPSF_OK) stats.store(p);
  }
  if (rc == RPSF_OK && !out.direct) {
    if (out.uniform) rc = rpsf_conv_scatter(p->d_view_out, (int64_t)stage_stride, outs[0], n, out.frame_bytes, st);
    for (int f = 0; !out.uniform && f < n && rc == RPSF_OK; ++f) rc = rpsf_conv_scatter(p->d_view_out + f * stage_stride, 0, outs[f], 1, 0, st);
  }
  if (staged) {
    HIP_TRY(hipEventRecord(p->ev_view, st));
    p->view_stream = st, p->view_busy = true;
  }
  if (rc == RPSF_OK && route_or_null)
    *route_or_null = (in.direct ? 0 : RPSF_ROUTE_C1 | (batch ? RPSF_ROUTE_STAGED : 0)) | (out.direct ? 0 : RPSF_ROUTE_C2) | (saturated ? RPSF_ROUTE_SATURATED : 0);
  return rc;
}

extern "C" int rpsf_apply_view(rpsf_plan* p, const rpsf_view* image, const rpsf_view* out, int pad_mode, float pad_value, double threshold, int dilation,
                               int neighborhood_width, void* stream, int* route_or_null) {
  return apply_views(p, image, out, 1, pad_mode, pad_value, threshold, dilation, neighborhood_width, stream, route_or_null, false);
}

extern "C" int rpsf_apply_batch_view(rpsf_plan* p, const rpsf_view* images, const rpsf_view* outs, int n_frames, int pad_mode, float pad_value,
                                     double threshold, int dilation, int neighborhood_width, void* stream, int* route_or_null) {
  return apply_views(p, images, outs, n_frames, pad_mode, pad_value, threshold, dilation, neighborhood_width, stream, route_or_null, true);
}

// The masked entry points: a null mask with fill_nonfinite == 0 IS the unmasked entry point
extern "C" int rpsf_apply_view_masked(rpsf_plan* p, const rpsf_view* image, const rpsf_view* out, int pad_mode, float pad_value, double threshold,
                                      int dilation, int neighborhood_width, const rpsf_view* mask_or_null, int fill_nonfinite, void* stream,
                                      int* route_or_null) {
  if (!mask_or_null && !fill_nonfinite) return rpsf_apply_view(p, image, out, pad_mode, pad_value, threshold, dilation, neighborhood_width, stream, route_or_null);
  const SatMasks masks{mask_or_null, mask_or_null ? 1 : 0, fill_nonfinite};
  return apply_views(p, image, out, 1, pad_mode, pad_value, threshold, dilation, neighborhood_width, stream, route_or_null, false, &masks);
}

extern "C" int rpsf_apply_batch_view_masked(rpsf_plan* p, const rpsf_view* images, const rpsf_view* outs, int n_frames, int pad_mode, float pad_value,
                                            double threshold, int dilation, int neighborhood_width, const rpsf_view* masks_or_null, int n_masks,
                                            int fill_nonfinite, void* stream, int* route_or_null) {
  if (!masks_or_null && !fill_nonfinite)
    return rpsf_apply_batch_view(p, images, outs, n_frames, pad_mode, pad_value, threshold, dilation, neighborhood_width, stream, route_or_null);
  const SatMasks masks{masks_or_null, masks_or_null ? n_masks : 0, fill_nonfinite};
  return apply_views(p, images, outs, n_frames, pad_mode, pad_value, threshold, dilation, neighborhood_width, stream, route_or_null, true, &masks);
}

extern "C" int rpsf_apply_batch_device_masked(rpsf_plan* p, const void* images_dev, void* outs_dev, int n_frames, size_t image_stride, size_t out_stride,
                                              int height, int width, int pad_mode, double threshold, int dilation, int neighborhood_width,
                                              const rpsf_view* masks_or_null, int n_masks, int fill_nonfinite, void* stream,
                                              size_t* n_masked_per_frame_or_null) {
  if (!masks_or_null && !fill_nonfinite)
    return rpsf_apply_batch_device_saturated(p, images_dev, outs_dev, n_frames, image_stride, out_stride, height, width, pad_mode, threshold, dilation,
                                             neighborhood_width, stream, n_masked_per_frame_or_null);
  if (p && n_frames == 0) {
    SatBatchStats().store(p);
    return RPSF_OK;
  }
  int rc = check_saturated_call(p, images_dev, outs_dev, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  if (n_frames < 0) return fail(RPSF_E_BADARG, "n_frames must not be negative");
  if (n_frames > 1 && (image_stride < (size_t)height * width || out_stride < (size_t)height * width))
    return fail(RPSF_E_BADARG, "frame stride smaller than one frame");
  const SatMasks masks{masks_or_null, masks_or_null ? n_masks : 0, fill_nonfinite};
  if ((rc = check_masks(masks, n_frames, height, width)) != RPSF_OK) return rc;
  SatDeviceRun run;
  rc = sat_device_init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, &run);
  if (rc != RPSF_OK) return rc;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : p->stream;
  const int G = sat_group_frames(p, run, true);
  SatBatchStats stats;
  stats.frames = n_frames;
  for (int f0 = 0; f0 < n_frames; f0 += G) {
    rc = sat_device_apply_group(p, run, std::min(G, n_frames - f0), static_cast<const float*>(images_dev) + (size_t)f0 * image_stride, image_stride,
                                static_cast<float*>(outs_dev) + (size_t)f0 * out_stride, out_stride, rpsfsatb::ORDER_LONGEST_FIRST, st, &stats,
                                n_masked_per_frame_or_null ? n_masked_per_frame_or_null + f0 : nullptr, &masks, f0);
    if (rc != RPSF_OK) return rc;
  }
  stats.store(p);
  return RPSF_OK;
}

// `count` dense height x width uint8 host masks into the plan's mask scratch, on the plan's stream; views[f]: mask f there
static int upload_host_masks(rpsf_plan* p, const uint8_t* const* masks_host, int count, int height, int width, std::vector<rpsf_view>* views) {
  const size_t npix = (size_t)height * width;
  if (npix * count > p->host_mask_bytes) {
    HIP_TRY(hipDeviceSynchronize());  // an earlier call may still read the old scratch
    p->host_mask_bytes = 0;
    HIP_TRY(p->d_host_masks.alloc(npix * count));
    p->host_mask_bytes = npix * count;
  }
  views->resize(count);
  for (int f = 0; f < count; ++f) {
    uint8_t* dst = p->d_host_masks + f * npix;
    HIP_TRY(hipMemcpyAsync(dst, masks_host[f], npix, hipMemcpyHostToDevice, p->stream));
    (*views)[f] = rpsf_view{dst, RPSF_DTYPE_UINT8, height, width, (int64_t)width, 1};
  }
  return RPSF_OK;
}

extern "C" int rpsf_apply_frames_host_masked_device(rpsf_plan* p, const void* const* images_host, int image_is_f64, int n_frames, int height, int width,
                                                    int pad_mode, double threshold, int dilation, int neighborhood_width,
                                                    const uint8_t* const* masks_host_or_null, int n_masks, int fill_nonfinite, void* const* outs_host,
                                                    int out_is_f64) {
  if (!masks_host_or_null && !fill_nonfinite)
    return rpsf_apply_frames_host_saturated_device(p, images_host, image_is_f64, n_frames, height, width, pad_mode, threshold, dilation,
                                                   neighborhood_width, outs_host, out_is_f64);
  if (p && n_frames == 0) {
    SatBatchStats().store(p);
    return RPSF_OK;
  }
  int rc = check_saturated_call(p, images_host, outs_host, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  if (n_frames < 0) return fail(RPSF_E_BADARG, "n_frames must not be negative");
  for (int f = 0; f < n_frames; ++f)
    if (!images_host[f] || !outs_host[f]) return fail(RPSF_E_BADARG, "null frame pointer");
  if (!masks_host_or_null) n_masks = 0;
  if (n_masks < 0 || (n_masks > 1 && n_masks != n_frames)) return fail(RPSF_E_BADARG, "mask: no mask, one mask or one mask per frame");
  for (int f = 0; f < n_masks; ++f)
    if (!masks_host_or_null[f]) return fail(RPSF_E_BADARG, "mask: null mask pointer");
  SatDeviceRun run;
  rc = sat_device_init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, &run);
  if (rc != RPSF_OK) return rc;
  const size_t npix = (size_t)height * width;
  const int G = std::min(sat_group_frames(p, run, true), n_frames);
  rc = rpsf_detail_pipe_ensure(p, npix * G, 1);
  if (rc != RPSF_OK) return rc;
  const int T = rpsf_detail_host_parts_for(npix * G * sizeof(float));
  SatBatchStats stats;
  stats.frames = n_frames;
  std::vector<rpsf_view> views;
  if (n_masks == 1 && (rc = upload_host_masks(p, masks_host_or_null, 1, height, width, &views)) != RPSF_OK) return rc;
  for (int f0 = 0; f0 < n_frames; f0 += G) {
    const int fg = std::min(G, n_frames - f0);
    // (the scratch of the group before is free: sat_host_group returned after its stream had finished)
    if (n_masks > 1 && (rc = upload_host_masks(p, masks_host_or_null + f0, fg, height, width, &views)) != RPSF_OK) return rc;
    const SatMasks masks{views.empty() ? nullptr : views.data(), (int)views.size(), fill_nonfinite};
    rc = sat_host_group(p, run, fg, images_host + f0, image_is_f64, outs_host + f0, out_is_f64, rpsfsatb::ORDER_LONGEST_FIRST, T, &stats, &masks);
    if (rc != RPSF_OK) return rc;
  }
  stats.store(p);
  return rpsf_detail_sweep_check(p);
}

extern "C" int rpsf_saturation_kernel_ms(rpsf_plan* p, double ms[5]) {
  if (!p || !ms) return fail(RPSF_E_BADARG, "null argument");
  for (int i = 0; i < 5; ++i) ms[i] = 0.0;
  if (!p->sat_dev) return RPSF_OK;
  HIP_TRY(hipSetDevice(p->device));
  return rpsf_sat_kernel_ms(p->sat_dev.get(), ms);
}

extern "C" int rpsf_saturation_batch_info(rpsf_plan* p, int info[4]) {
  if (!p || !info) return fail(RPSF_E_BADARG, "null argument");
  for (int i = 0; i < 4; ++i) info[i] = p->sat_batch_info[i];
  return RPSF_OK;
}

// The test entries: F1 - F4 alone on n_frames float32 host frames, frame-group by frame-group; the filled padded frames
// ((H + 4N) x (W + 4N) float32 each) and the masks come back
static int sat_fill_frames(rpsf_plan* p, const float* images_host, int n_frames, int height, int width, int pad_mode, double threshold, int dilation,
                           int neighborhood_width, int order, float* padded_host, uint8_t* masks_host, int* groups_per_frame_or_null,
                           SatBatchStats* stats, const SatMasks* masks = nullptr, int* masked_per_frame_or_null = nullptr) {
  if (!p || !images_host || !padded_host || !masks_host) return fail(RPSF_E_BADARG, "null argument");
  if (n_frames < 1) return fail(RPSF_E_BADARG, "n_frames must be positive");
  if (height <= 0 || width <= 0) return fail(RPSF_E_BADARG, "image shape must be positive");
  if (pad_mode < 0 || pad_mode > RPSF_PAD_WRAP) return fail(RPSF_E_BADARG, "unknown pad mode");
  if (dilation < 1 || neighborhood_width / 2 < 1) return fail(RPSF_E_BADARG, "dilation must be >= 1 and neighborhood_width // 2 >= 1");
  if (order < rpsfsatb::ORDER_LONGEST_FIRST || order > rpsfsatb::ORDER_FRAMES) return fail(RPSF_E_BADARG, "order must be 0, 1 or 2");
  const long PH = (long)height + 4L * p->N, PW = (long)width + 4L * p->N;
  if (PH * PW >= ((long)1 << 31)) return fail(RPSF_E_UNSUPPORTED, "padded frame too large for this entry point");
  HIP_TRY(hipSetDevice(p->device));
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;
  rpsf_detail_clear_error(p);
  if (!p->sat_dev) p->sat_dev.reset(rpsf_sat_create());
  SatDevice* sd = p->sat_dev.get();
  const SatCall call{height, width, p->N, pad_mode, dilation, neighborhood_width, threshold, 0, 0, 1};
  const size_t npix = (size_t)height * width, np = (size_t)PH * PW;
  const int G = std::min(n_frames, p->sat_group_opt > 0 ? p->sat_group_opt : rpsfsatb::auto_group_frames(np, (size_t)height * PW, masks != nullptr));
  DevBuf<float> d_images;
  HIP_TRY(d_images.upload(images_host, npix * n_frames));
  stats->frames = n_frames;
  for (int f0 = 0; f0 < n_frames; f0 += G) {
    const int fg = std::min(G, n_frames - f0);
    float *padded = nullptr, *corrected = nullptr;
    size_t p_stride = 0, c_stride = 0;
    const float* d_first = d_images;
    int rc;
    if (!masks) {
      rc = rpsf_sat_fill_batch(sd, call, fg, d_first + (size_t)f0 * npix, npix, order, p->stream, &padded, &p_stride, &corrected, &c_stride);
    } else {
      const std::vector<rpsfsat::MaskView> views = group_views(*masks, f0, fg);
      rc = rpsf_sat_fill_batch_masked(sd, call, fg, d_first + (size_t)f0 * npix, npix, views.empty() ? nullptr : views.data(), masks->fill_nonfinite,
                                      order, p->stream, &padded, &p_stride, &corrected, &c_stride);
    }
    if (rc == RPSF_OK) rc = rpsf_sat_masks_batch(sd, call, p->stream, masks_host + (size_t)f0 * np);  // waits for the stream
    if (rc != RPSF_OK) {
      (void)hipStreamSynchronize(p->stream);
      return rc;
    }
    for (int f = 0; f < fg; ++f) {
      HIP_TRY(hipMemcpy(padded_host + (size_t)(f0 + f) * np, padded + f * p_stride, np * sizeof(float), hipMemcpyDeviceToHost));
      int n_hot, n_mask, n_groups;
      rpsf_sat_frame_counts(sd, f, &n_hot, &n_mask, &n_groups);
      if (groups_per_frame_or_null) groups_per_frame_or_null[f0 + f] = n_groups;
      if (masked_per_frame_or_null) masked_per_frame_or_null[f0 + f] = n_mask;
    }
    long groups = 0, masked = 0;
    rpsf_sat_batch_totals(sd, &groups, &masked);
    stats->frame_groups += 1, stats->groups += groups, stats->masked += masked;
  }
  return RPSF_OK;
}

// one frame; reverse_groups: F4's workgroups take the groups in the reverse of the batch's order instead of the table's own
extern "C" int rpsf_saturation_fill_device(rpsf_plan* p, const float* image_host, int height, int width, int pad_mode, double threshold, int dilation,
                                           int neighborhood_width, int reverse_groups, float* padded_host, uint8_t* mask_host, int* n_groups_or_null) {
  SatBatchStats stats;
  return sat_fill_frames(p, image_host, 1, height, width, pad_mode, threshold, dilation, neighborhood_width,
                         reverse_groups ? rpsfsatb::ORDER_REVERSED : rpsfsatb::ORDER_FRAMES, padded_host, mask_host, n_groups_or_null, &stats);
}

extern "C" int rpsf_saturation_fill_batch_device(rpsf_plan* p, const float* images_host, int n_frames, int height, int width, int pad_mode,
                                                 double threshold, int dilation, int neighborhood_width, int order, float* padded_host,
                                                 uint8_t* masks_host, int* groups_per_frame_or_null) {
  SatBatchStats stats;
  const int rc = sat_fill_frames(p, images_host, n_frames, height, width, pad_mode, threshold, dilation, neighborhood_width, order, padded_host,
                                 masks_host, groups_per_frame_or_null, &stats);
  if (rc == RPSF_OK) stats.store(p);
  return rc;
}

// The masked test entry: n_masks (0, 1 or n_frames) host masks, mask_frame_bytes apart, element (r, c) of a mask at r * mask_row_stride +
// c * mask_col_stride bytes - uploaded as they lie and read through those strides
extern "C" int rpsf_saturation_fill_masked_device(rpsf_plan* p, const float* images_host, int n_frames, int height, int width, int pad_mode,
                                                  double threshold, int dilation, int neighborhood_width, int order, const uint8_t* masks_in_host,
                                                  int n_masks, size_t mask_frame_bytes, int64_t mask_row_stride, int64_t mask_col_stride,
                                                  int fill_nonfinite, float* padded_host, uint8_t* masks_host, int* groups_per_frame_or_null,
                                                  int* masked_per_frame_or_null) {
  if (!p) return fail(RPSF_E_BADARG, "null argument");
  if (!masks_in_host) n_masks = 0;
  if (n_masks < 0 || (n_masks > 1 && n_masks != n_frames)) return fail(RPSF_E_BADARG, "mask: no mask, one mask or one mask per frame");
  if (n_masks && (height <= 0 || width <= 0 || mask_row_stride <= 0 || mask_col_stride <= 0 ||
                  (size_t)(height - 1) * mask_row_stride + (size_t)(width - 1) * mask_col_stride + 1 > mask_frame_bytes))
    return fail(RPSF_E_BADARG, "mask: the strides do not fit mask_frame_bytes");
  HIP_TRY(hipSetDevice(p->device));
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;
  rpsf_detail_clear_error(p);
  DevBuf<uint8_t> d_masks;
  std::vector<rpsf_view> views((size_t)n_masks);
  if (n_masks) HIP_TRY(d_masks.upload(masks_in_host, mask_frame_bytes * n_masks));
  for (int f = 0; f < n_masks; ++f) views[f] = rpsf_view{d_masks + f * mask_frame_bytes, RPSF_DTYPE_UINT8, height, width, mask_row_stride, mask_col_stride};
  const SatMasks masks{views.empty() ? nullptr : views.data(), n_masks, fill_nonfinite};
  SatBatchStats stats;
  return sat_fill_frames(p, images_host, n_frames, height, width, pad_mode, threshold, dilation, neighborhood_width, order, padded_host, masks_host,
                         groups_per_frame_or_null, &stats, &masks, masked_per_frame_or_null);
}

// ------------------------------------------------------------------------------------------------
// Host-side saturation fill (regularizepsf/transform.py:135-138).  Sequential by definition: masked pixels
// are visited in row-major order and each is replaced by the NaN-ignoring mean of the window
// [i - w/2, i + w/2) x [j - w/2, j + w/2), so later pixels see earlier fills.  Window bounds follow Python
// slice semantics (a negative start wraps once; an empty window gives NaN), as in the reference.
// ------------------------------------------------------------------------------------------------

extern "C" int rpsf_saturation_fill(double* padded, int rows, int cols, const uint8_t* mask, int neighborhood_width) {
  if (!padded || !mask || rows <= 0 || cols <= 0) return fail(RPSF_E_BADARG, "bad argument");
  const long h = neighborhood_width / 2;  // floor division, like Python's // for the non-negative widths in use
  const double nan = std::nan("");
  for (long i = 0; i < rows; ++i)
    for (long j = 0; j < cols; ++j) {
      if (!mask[i * cols + j]) continue;
      long r0, r1, c0, c1;
      py_slice(i - h, i + h, rows, &r0, &r1);
      py_slice(j - h, j + h, cols, &c0, &c1);
      double sum = 0.0;
      long cnt = 0;
      for (long r = r0; r < r1; ++r)
        for (long c = c0; c < c1; ++c) {
          double v = padded[r * cols + c];
          if (v == v) sum += v, ++cnt;
        }
      padded[i * cols + j] = cnt ? sum / (double)cnt : nan;
    }
  return RPSF_OK;
}
