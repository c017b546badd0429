// CPU lane emulator for the bad-pixel-mask route of kernels F1 - F5 (test infrastructure, never shipped in the product path): the
// masked variants of F1 and of F2's last pass (rpsf_core_saturation.hpp: f1_pad_masked, f2_cross_merge) with F2 - F5 as they are, once
// as single-frame functions (emumask_fill) and once through the batch drivers of rpsf_core_saturation_batch.hpp in the launch order of
// csrc/saturation.hip (emumask_fill_batch, emumask_restore_batch).  The masks are read through their row and column strides, as the
// kernel reads them.  Every scratch array is laid out as on the device and starts out poisoned.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_saturation_batch.hpp"
#include "emu_ctx.hpp"

using namespace rpsfs;
using namespace rpsfsatb;

namespace {

// ---------------------------------------------------------------------------------------------------------------- one frame
struct Filled {
  Padded f;
  std::vector<float> padded;
  std::vector<uint8_t> bytes[3], exact;
  const uint8_t* mask = nullptr;  // null: nothing hot and nothing exact
  int n_hot = 0, n_exact = 0, n_mask = 0, n_groups = 0;
};

void fill_one(const float* image, int H, int W, int N, int pad_mode, double threshold, int dilation, int width, MaskView m, int fill_nonfinite,
              Filled& s) {
  s.f = Padded{H, W, N, H + 4 * N, W + 4 * N, pad_mode};
  const Padded& f = s.f;
  const long npix = f.npix(), quads = (npix + 3) / 4;
  const int PH = f.PH, PW = f.PW, h = width / 2;
  s.padded.assign(npix, -7.f);
  for (auto& b : s.bytes) b.assign(npix, 9);
  s.exact.assign(npix, 9);
  for (long gid = 0; gid < quads; ++gid)
    f1_pad_masked(gid, f, image, threshold, m, fill_nonfinite, s.padded.data(), s.bytes[0].data(), s.exact.data(), &s.n_hot, &s.n_exact);
  if (s.n_hot == 0 && s.n_exact == 0) return;
  int at = 0;
  for (int pass = 0; pass < dilation; ++pass, at ^= 1)
    for (long gid = 0; gid < quads; ++gid) {
      if (pass == dilation - 1) f2_cross_merge(gid, PH, PW, s.bytes[at].data(), s.exact.data(), s.bytes[at ^ 1].data(), &s.n_mask);
      else f2_cross(gid, PH, PW, s.bytes[at].data(), s.bytes[at ^ 1].data(), nullptr);
    }
  const uint8_t* mask = s.bytes[at].data();
  const uint8_t* grown = mask;
  if (const int reach = box_reach(h); reach > 0) {
    for (long gid = 0; gid < npix; ++gid) f3_rows(gid, PH, PW, reach, mask, s.bytes[at ^ 1].data());
    for (long gid = 0; gid < npix; ++gid) f3_cols(gid, PH, PW, reach, s.bytes[at ^ 1].data(), s.bytes[2].data());
    grown = s.bytes[2].data();
  }
  std::vector<int32_t> labels(npix, -7);
  {
    const int tiles_y = (PH + TILE_R - 1) / TILE_R, tiles_x = (PW + TILE_C - 1) / TILE_C;
    std::vector<int> ll(TILE_R * TILE_C);
    CpuCtx ctx{TILE_THREADS};
    for (int ty = 0; ty < tiles_y; ++ty)
      for (int tx = 0; tx < tiles_x; ++tx) {
        for (int& x : ll) x = -7;
        s3_tile(ctx, grown, PH, PW, ty, tx, ll.data(), labels.data());
      }
    for (long gid = 0; gid < (long)tiles_y * tiles_x * SEAM_SLOTS; ++gid) s3_seam(gid, PH, PW, labels.data());
    for (long gid = 0; gid < npix; ++gid) s3_flatten(gid, npix, labels.data());
  }
  const long nseg = (long)PH * segs_per_row(PW);
  std::vector<int> segcnt(nseg, -1), segoff(nseg, -1), scan_lds(SCAN_THREADS + 32);
  for (long seg = 0; seg < nseg; ++seg) s4_count(seg, PH, PW, labels.data(), segcnt.data());
  CpuCtx scan{SCAN_THREADS};
  s4_scan(scan, nseg, segcnt.data(), segoff.data(), &s.n_groups, scan_lds.data());
  const long n = s.n_groups;
  std::vector<int> roots(n, -1), stats(GROUP_STATS * (size_t)n, -1);
  std::vector<double> fills(s.n_mask, -7.0);
  for (long seg = 0; seg < nseg; ++seg) s4_roots(seg, PH, PW, labels.data(), segoff.data(), roots.data());
  for (long k = 0; k < n; ++k) f3_init(k, n, stats.data());
  for (long gid = 0; gid < npix; ++gid) f3_accumulate(gid, npix, PW, mask, labels.data(), roots.data(), n, stats.data());
  int cursor = 0;
  CpuCtx wave{FILL_LANES};
  for (long b = 0; b < n; ++b) {
    FillLds lds;
    std::memset(&lds, 0xA5, sizeof(lds));  // nothing may depend on what the previous group left
    f4_group(wave, b, PH, PW, h, mask, roots.data(), stats.data(), s.padded.data(), labels.data(), fills.data(), &cursor, &lds);
  }
  s.mask = mask;
}

// ---------------------------------------------------------------------------------------------------------------- a frame-group
struct Group {
  Stack s;
  int frames = 0, at = 0;
  long groups = 0, masked = 0, listed = 0;
  std::vector<float> padded;
  std::vector<uint8_t> bytes[3], exact;
  std::vector<int32_t> labels;
  std::vector<int> segcnt, segoff, counters, info;
};

bool fill_group(const float* images, size_t image_stride, int frames, int H, int W, int N, int pad_mode, double threshold, int dilation, int width,
                const MaskView* masks, int fill_nonfinite, int order_mode, Group& g) {
  const Padded f{H, W, N, H + 4 * N, W + 4 * N, pad_mode};
  const long npix = f.npix(), quads = (npix + 3) / 4, nseg = (long)f.PH * segs_per_row(f.PW);
  const int PH = f.PH, PW = f.PW, h = width / 2;
  const size_t F = (size_t)frames, stride = frame_stride((size_t)npix);
  g.frames = frames;
  g.padded.assign(F * stride, -7.f);
  for (auto& b : g.bytes) b.assign(F * stride, 9);
  g.exact.assign(F * stride, 9);
  g.labels.assign(F * stride, -7);
  g.segcnt.assign(F * nseg, -1), g.segoff.assign(F * nseg, -1);
  g.counters.assign(F * FRAME_COUNTERS + SHARED_COUNTERS, 0);
  g.info.assign(F * FRAME_INFO, -1);
  Stack& s = g.s;
  s.f = f, s.stride = stride, s.nseg = (size_t)nseg;
  s.padded = g.padded.data(), s.labels = g.labels.data(), s.segcnt = g.segcnt.data(), s.segoff = g.segoff.data(), s.counters = g.counters.data();
  for (int i = 0; i < 3; ++i) s.bytes[i] = g.bytes[i].data();
  s.exact = g.exact.data();

  for (int fr = 0; fr < frames; ++fr)
    for (long gid = 0; gid < quads; ++gid) b1_pad_masked(gid, fr, s, images, image_stride, threshold, masks, fill_nonfinite);
  int at = 0;
  for (int pass = 0; pass < dilation; ++pass, at ^= 1)
    for (int fr = 0; fr < frames; ++fr)
      for (long gid = 0; gid < quads; ++gid) {
        if (pass == dilation - 1) b2_cross_merge(gid, fr, s, at);
        else b2_cross(gid, fr, s, at, 0);
      }
  g.at = at;
  int grown = at;
  if (const int reach = box_reach(h); reach > 0) {
    for (int fr = 0; fr < frames; ++fr)
      for (long gid = 0; gid < npix; ++gid) b3_rows(gid, fr, s, reach, at);
    for (int fr = 0; fr < frames; ++fr)
      for (long gid = 0; gid < npix; ++gid) b3_cols(gid, fr, s, reach, at);
    grown = 2;
  }
  const int tiles_y = (PH + TILE_R - 1) / TILE_R, tiles_x = (PW + TILE_C - 1) / TILE_C;
  {
    std::vector<int> ll(TILE_R * TILE_C);
    CpuCtx ctx{TILE_THREADS};
    for (int fr = 0; fr < frames; ++fr)
      for (int ty = 0; ty < tiles_y; ++ty)
        for (int tx = 0; tx < tiles_x; ++tx) {
          for (int& x : ll) x = -7;
          b3_tile(ctx, fr, s, grown, ty, tx, ll.data());
        }
  }
  for (int fr = 0; fr < frames; ++fr)
    for (long gid = 0; gid < (long)tiles_y * tiles_x * SEAM_SLOTS; ++gid) b3_seam(gid, fr, s);
  for (int fr = 0; fr < frames; ++fr)
    for (long gid = 0; gid < npix; ++gid) b3_flatten(gid, fr, s);
  for (int fr = 0; fr < frames; ++fr)
    for (long seg = 0; seg < nseg; ++seg) b3_count(seg, fr, s);
  {
    std::vector<int> scan_lds(SCAN_THREADS + 32);
    CpuCtx scan{SCAN_THREADS};
    for (int fr = 0; fr < frames; ++fr) b3_scan(scan, fr, s, scan_lds.data());
  }
  if (!plan_tables(g.counters.data(), frames, (size_t)H * W, g.info.data(), &g.groups, &g.masked, &g.listed)) return false;
  if (g.groups == 0) return true;
  const size_t n = (size_t)g.groups;
  std::vector<int> roots(n, -1), stats(GROUP_STATS * n, -1), gframe(n, -1), order(n, -1);
  std::vector<double> fills((size_t)g.masked, -7.0);
  int most = 0;
  for (int fr = 0; fr < frames; ++fr) most = std::max(most, g.info[FRAME_INFO * fr + I_GROUPS]);
  const Tables t{g.info.data(), roots.data(), stats.data(), gframe.data(), order.data(), g.counters.data() + F * FRAME_COUNTERS, fills.data(), g.groups};
  for (int fr = 0; fr < frames; ++fr)
    for (long seg = 0; seg < nseg; ++seg) b3_roots(seg, fr, s, t);
  for (int fr = 0; fr < frames; ++fr)
    for (long k = 0; k < most; ++k) b3_init(k, fr, t);
  for (int fr = 0; fr < frames; ++fr)
    for (long gid = 0; gid < npix; ++gid) b3_accumulate(gid, fr, s, t, at);
  if (order_mode != ORDER_FRAMES) {
    for (long k = 0; k < g.groups; ++k) o_hist(k, t);
    for (long k = 0; k < g.groups; ++k) o_scatter(k, t);
  }
  CpuCtx wave{FILL_LANES};
  for (long b = 0; b < g.groups; ++b) {
    FillLds lds;
    std::memset(&lds, 0xA5, sizeof(lds));
    b4_group(wave, b, order_mode, s, t, at, h, &lds);
  }
  return true;
}

bool bad_args(int n_frames, int H, int W, int N, int dilation, int width, int n_masks, long row_stride, long col_stride) {
  return n_frames < 1 || n_frames > MAX_GROUP_FRAMES || H <= 0 || W <= 0 || N <= 0 || dilation < 1 || width / 2 < 1 || n_masks < 0 ||
         (n_masks > 1 && n_masks != n_frames) || (n_masks && (row_stride <= 0 || col_stride <= 0));
}

// masks: n_masks of them, frame_bytes apart; one view per frame (empty: no mask)
std::vector<MaskView> views_of(const uint8_t* masks, int n_masks, size_t frame_bytes, long row_stride, long col_stride, int n_frames) {
  std::vector<MaskView> v(masks && n_masks ? (size_t)n_frames : 0);
  for (size_t f = 0; f < v.size(); ++f) v[f] = MaskView{masks + (n_masks == 1 ? 0 : f) * frame_bytes, row_stride, col_stride};
  return v;
}
}  // namespace

// F1 - F4 of one frame by the single-frame functions: the filled padded frame, the mask M | E, counts[4] = hot, exact, masked, groups
extern "C" int emumask_fill(const float* image, int H, int W, int N, int pad_mode, double threshold, int dilation, int width, const uint8_t* mask_in,
                            long row_stride, long col_stride, int fill_nonfinite, float* padded, uint8_t* mask, int* counts) {
  if (bad_args(1, H, W, N, dilation, width, mask_in ? 1 : 0, row_stride, col_stride)) return -1;
  Filled s;
  fill_one(image, H, W, N, pad_mode, threshold, dilation, width, MaskView{mask_in, row_stride, col_stride}, fill_nonfinite, s);
  const size_t np = (size_t)s.f.npix();
  std::memcpy(padded, s.padded.data(), np * sizeof(float));
  if (s.mask) std::memcpy(mask, s.mask, np);
  else std::memset(mask, 0, np);
  counts[0] = s.n_hot, counts[1] = s.n_exact, counts[2] = s.n_mask, counts[3] = s.n_groups;
  return 0;
}

// F1 - F4 of one frame-group through the batch drivers: dense padded frames and masks, counts[4 * f ...] as above per frame
extern "C" int emumask_fill_batch(const float* images, int n_frames, size_t image_stride, int H, int W, int N, int pad_mode, double threshold,
                                  int dilation, int width, int order_mode, const uint8_t* masks_in, int n_masks, size_t mask_frame_bytes,
                                  long row_stride, long col_stride, int fill_nonfinite, float* padded, uint8_t* masks, int* counts) {
  if (bad_args(n_frames, H, W, N, dilation, width, masks_in ? n_masks : 0, row_stride, col_stride)) return -1;
  const std::vector<MaskView> views = views_of(masks_in, n_masks, mask_frame_bytes, row_stride, col_stride, n_frames);
  Group g;
  if (!fill_group(images, image_stride, n_frames, H, W, N, pad_mode, threshold, dilation, width, views.empty() ? nullptr : views.data(),
                  fill_nonfinite, order_mode, g))
    return -2;
  const size_t np = (size_t)(H + 4 * N) * (W + 4 * N);
  for (int fr = 0; fr < n_frames; ++fr) {
    std::memcpy(padded + (size_t)fr * np, g.padded.data() + fr * g.s.stride, np * sizeof(float));
    const bool idle = g.s.idle(fr);
    if (idle) std::memset(masks + (size_t)fr * np, 0, np);
    else std::memcpy(masks + (size_t)fr * np, g.bytes[g.at].data() + fr * g.s.stride, np);
    int* c = counts + 4 * fr;
    c[0] = *g.s.counter(fr, C_HOT), c[1] = *g.s.counter(fr, C_EXACT), c[2] = idle ? 0 : *g.s.counter(fr, C_MASK), c[3] = g.info[FRAME_INFO * fr + I_GROUPS];
  }
  return 0;
}

// F5 behind F1 - F4 of one frame-group, `corrected` (c_stride floats per frame: the rows of the padded frame from out_row0 on) standing
// in for the correction: outs, per frame the list of masked in-frame pixels (H * W ints apart in `lists`) and its length
extern "C" int emumask_restore_batch(const float* images, int n_frames, size_t image_stride, int H, int W, int N, int pad_mode, double threshold,
                                     int dilation, int width, const uint8_t* masks_in, int n_masks, size_t mask_frame_bytes, long row_stride,
                                     long col_stride, int fill_nonfinite, const float* corrected, size_t c_stride, int out_row0, float* outs,
                                     size_t out_stride, int32_t* lists, int* n_lists) {
  if (bad_args(n_frames, H, W, N, dilation, width, masks_in ? n_masks : 0, row_stride, col_stride)) return -1;
  const std::vector<MaskView> views = views_of(masks_in, n_masks, mask_frame_bytes, row_stride, col_stride, n_frames);
  Group g;
  if (!fill_group(images, image_stride, n_frames, H, W, N, pad_mode, threshold, dilation, width, views.empty() ? nullptr : views.data(),
                  fill_nonfinite, ORDER_LONGEST_FIRST, g))
    return -2;
  std::vector<int32_t> packed((size_t)g.listed + 1, -1);
  for (int fr = 0; fr < n_frames; ++fr)
    for (long gid = 0; gid < (long)H * W; ++gid)
      b5_restore(gid, fr, g.s, g.info.data(), g.at, images, image_stride, corrected, c_stride, out_row0, outs, out_stride, packed.data());
  for (int fr = 0; fr < n_frames; ++fr) {
    const int n = g.s.idle(fr) ? 0 : *g.s.counter(fr, C_LIST);
    const long room = (fr + 1 < n_frames ? g.info[FRAME_INFO * (fr + 1) + I_LIST0] : g.listed) - g.info[FRAME_INFO * fr + I_LIST0];
    if (n > room) return -3;
    n_lists[fr] = n;
    std::memcpy(lists + (size_t)fr * H * W, packed.data() + g.info[FRAME_INFO * fr + I_LIST0], (size_t)n * sizeof(int32_t));
  }
  return 0;
}
