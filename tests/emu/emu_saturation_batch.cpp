// CPU lane emulator for rpsf_core_saturation_batch.hpp (test infrastructure, never shipped in the product path).
// Runs the batch drivers of kernels F1 - F5 with a context whose each() loops over the threads of a workgroup; frames, workgroups and
// grid threads one after the other, in the launch order of csrc/saturation.hip's rpsf_sat_fill_batch - so the frame strides, the
// per-frame counters, labels and root slices, the one group table, F4's order pass and the cut into frame-groups are checked without a GPU.
// Every scratch array is laid out as on the device (frames `stride` apart) and starts out poisoned.
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

struct Group {  // one frame-group, filled
  Stack s;
  int frames = 0, at = 0;
  long groups = 0, masked = 0, listed = 0;
  std::vector<float> padded;
  std::vector<uint8_t> bytes[3];
  std::vector<int32_t> labels;
  std::vector<int> segcnt, segoff, counters, info;
};

// F1 - F4 of `frames` frames; false: the host step refused the counters
bool fill(const float* images, size_t image_stride, int frames, int H, int W, int N, int pad_mode, double threshold, int dilation, int width,
          int order_mode, Group& g) {
  const Padded f{H, W, N, H + 4 * N, W + 4 * N, pad_mode};
  const long npix = f.npix(), quads = (npix + 3) / 4, nseg = (long)f.PH * segs_per_row(f.PW);
  const int PH = f.PH, PW = f.PW, h = width / 2;
  const size_t F = (size_t)frames, stride = frame_stride((size_t)npix);
  g.frames = frames;
  g.padded.assign(F * stride, -7.f);
  for (auto& b : g.bytes) b.assign(F * stride, 9);
  g.labels.assign(F * stride, -7);
  g.segcnt.assign(F * nseg, -1), g.segoff.assign(F * nseg, -1);
  g.counters.assign(F * FRAME_COUNTERS + SHARED_COUNTERS, 0);
  g.info.assign(F * FRAME_INFO, -1);
  Stack& s = g.s;
  s.f = f, s.stride = stride, s.nseg = (size_t)nseg;
  s.padded = g.padded.data(), s.labels = g.labels.data(), s.segcnt = g.segcnt.data(), s.segoff = g.segoff.data(), s.counters = g.counters.data();
  for (int i = 0; i < 3; ++i) s.bytes[i] = g.bytes[i].data();

  for (int fr = 0; fr < frames; ++fr)
    for (long gid = 0; gid < quads; ++gid) b1_pad(gid, fr, s, images, image_stride, threshold);
  int at = 0;
  for (int pass = 0; pass < dilation; ++pass, at ^= 1)
    for (int fr = 0; fr < frames; ++fr)
      for (long gid = 0; gid < quads; ++gid) b2_cross(gid, fr, s, at, pass == dilation - 1);
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
  // ---- the host's one look at the counters
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
    std::vector<int> seen(order);  // every group exactly once, no bucket of shorter groups before a longer one
    std::sort(seen.begin(), seen.end());
    for (long k = 0; k < g.groups; ++k)
      if (seen[k] != k || (k > 0 && order_bucket(stats[GROUP_STATS * order[k]]) < order_bucket(stats[GROUP_STATS * order[k - 1]]))) return false;
  }
  CpuCtx wave{FILL_LANES};
  for (long b = 0; b < g.groups; ++b) {
    FillLds lds;
    std::memset(&lds, 0xA5, sizeof(lds));  // nothing may depend on what the previous group left
    b4_group(wave, b, order_mode, s, t, at, h, &lds);
  }
  return true;
}

bool bad_args(int n_frames, int H, int W, int N, int dilation, int width) {
  return n_frames < 1 || H <= 0 || W <= 0 || N <= 0 || dilation < 1 || width / 2 < 1;
}
}  // namespace

// F1 - F4 on n_frames frames image_stride floats apart, cut into frame-groups of `group` frames (0: auto_group_frames): the filled
// padded frames and the masks (dense, (H + 4N) x (W + 4N) each), the groups per frame; info[4] as rpsf_saturation_batch_info
extern "C" int emusatb_fill(const float* images, int n_frames, size_t image_stride, int H, int W, int N, int pad_mode, double threshold, int dilation,
                            int width, int order_mode, int group, float* padded, uint8_t* masks, int* groups_per_frame, int* info) {
  if (bad_args(n_frames, H, W, N, dilation, width) || group < 0 || group > MAX_GROUP_FRAMES) return -1;
  const size_t np = (size_t)(H + 4 * N) * (W + 4 * N);
  const int G = std::min(n_frames, group > 0 ? group : auto_group_frames(np, (size_t)H * (W + 4 * N)));
  long frame_groups = 0, groups = 0, masked = 0;
  for (int f0 = 0; f0 < n_frames; f0 += G) {
    const int fg = std::min(G, n_frames - f0);
    Group g;
    if (!fill(images + (size_t)f0 * image_stride, image_stride, fg, H, W, N, pad_mode, threshold, dilation, width, order_mode, g)) return -2;
    for (int fr = 0; fr < fg; ++fr) {
      std::memcpy(padded + (size_t)(f0 + fr) * np, g.padded.data() + fr * g.s.stride, np * sizeof(float));
      if (g.s.idle(fr)) std::memset(masks + (size_t)(f0 + fr) * np, 0, np);
      else std::memcpy(masks + (size_t)(f0 + fr) * np, g.bytes[g.at].data() + fr * g.s.stride, np);
      groups_per_frame[f0 + fr] = g.info[FRAME_INFO * fr + I_GROUPS];
    }
    ++frame_groups, groups += g.groups, masked += g.masked;
  }
  info[0] = n_frames, info[1] = (int)frame_groups, info[2] = (int)groups, info[3] = (int)masked;
  return 0;
}

// F5 behind F1 - F4 of one frame-group, with `corrected` (c_stride floats per frame: the rows of the padded frame from out_row0 on)
// standing in for the correction: outs (out_stride floats apart), per frame the list of masked in-frame pixels (H * W ints apart in
// `lists`) and its length
extern "C" int emusatb_restore(const float* images, int n_frames, size_t image_stride, int H, int W, int N, int pad_mode, double threshold,
                               int dilation, int width, const float* corrected, size_t c_stride, int out_row0, float* outs, size_t out_stride,
                               int32_t* lists, int* n_lists) {
  if (bad_args(n_frames, H, W, N, dilation, width) || n_frames > MAX_GROUP_FRAMES) return -1;
  Group g;
  if (!fill(images, image_stride, n_frames, H, W, N, pad_mode, threshold, dilation, width, ORDER_LONGEST_FIRST, g)) return -2;
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
