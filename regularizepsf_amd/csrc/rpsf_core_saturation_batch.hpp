// rpsf_core_saturation_batch.hpp - kernels F1 - F5 of rpsf_core_saturation.hpp for a GROUP OF FRAMES of one shape (csrc/saturation.hip,
// the batch drivers), shared with the CPU lane emulator tests/emu/emu_saturation_batch.cpp.  DESIGN.md 3.8, "Frame batches".
//
// Every function here is the single-frame function of the same number with a frame index: the frame's pointers are the stack's
// pointers plus frame x stride, its counters are its own block of FRAME_COUNTERS ints, and "nothing hot" is that frame's own hot
// count (on the masked route, b1_pad_masked / b2_cross_merge: its hot and its exact count).  Labels and roots stay linear indices WITHIN the frame, so two frames with the same hot layout have the same root values;
// nothing is united, dilated or searched across frames (the last padded row of frame f and the first of frame f + 1 are neighbours
// in memory and in nothing else: every neighbour test is the single-frame test against PH and PW).
//
// Between the labeller and the root list the host reads every frame's counters ONCE (plan_tables): it lays the frames' groups end to
// end in one table (first group and number of groups per frame: FRAME_INFO), likewise their lists of masked in-frame pixels.  F4 is then
// one launch of one wave per group over all frames; the workgroups take the groups longest first from an order array that a small
// device pass fills (o_hist, o_scatter: buckets of floor(log2(masked pixels)), integer atomics only).  The fill's result does not
// depend on that order: a group is filled by one wave alone and reads no other group's pixel.
#pragma once
#include "rpsf_core_saturation.hpp"

#pragma clang fp contract(off)

namespace rpsfsatb {

using namespace rpsfsat;

enum { C_HOT, C_MASK, C_GROUPS, C_LIST, C_EXACT, FRAME_COUNTERS };  // per frame, zeroed before F1; C_EXACT: pixels of the exact plane (masked route)
enum { I_GROUP0, I_GROUPS, I_LIST0, FRAME_INFO };          // per frame, from the host after its one wait
constexpr int ORDER_BUCKETS = 32;
enum { S_CURSOR, S_HIST, S_TAKEN = S_HIST + ORDER_BUCKETS, SHARED_COUNTERS = S_TAKEN + ORDER_BUCKETS };  // per frame-group, zeroed before F1
enum { ORDER_LONGEST_FIRST, ORDER_REVERSED, ORDER_FRAMES };  // F4: longest first; the same order backwards (testing aid); the table's own order

constexpr int MAX_GROUP_FRAMES = 65535;  // the frame is a grid's y or z index
// The scratch of a frame-group is kept under this many bytes: 32 frames of 512 x 512 / N = 64 take 0.5 GB of it, and from there on a
// longer group saves nothing that can be measured (one host wait per group against milliseconds of kernels) - DESIGN.md 3.8
constexpr size_t GROUP_BUDGET_BYTES = (size_t)1 << 30;

// f1_pad / f2_cross store 16 and 4 bytes at 4 gid: every frame of a stack starts on a multiple of 4 elements
RPSFS_HD size_t frame_stride(size_t count) { return (count + 3) & ~(size_t)3; }

// frames per frame-group: 11 bytes per padded pixel (frame, three byte planes, labels), the output rows of the correction and the 16
// bytes per output pixel the shared-K launch keeps per frame in flight
// (masked: one more byte plane, and the caller's mask of the frame in the plan's scratch)
RPSFS_HD int auto_group_frames(size_t padded_pixels, size_t out_pixels, bool masked = false) {
  const size_t per_frame = (masked ? 12 : 11) * frame_stride(padded_pixels) + (4 + 16 + (masked ? 1 : 0)) * frame_stride(out_pixels);
  const size_t g = GROUP_BUDGET_BYTES / per_frame;
  return g < 1 ? 1 : g > (size_t)MAX_GROUP_FRAMES ? MAX_GROUP_FRAMES : (int)g;
}

struct Stack {  // the frames of a frame-group
  Padded f;
  size_t stride;  // of padded, bytes[] and labels, in elements
  size_t nseg;    // of segcnt and segoff
  float* padded;
  uint8_t* bytes[3];
  uint8_t* exact = nullptr;  // the masked route's exact plane (b1_pad_masked, b2_cross_merge); nobody else looks at it
  int32_t* labels;
  int *segcnt, *segoff;
  int* counters;  // FRAME_COUNTERS per frame
  RPSFS_HD int* counter(int fr, int which) const { return counters + (size_t)FRAME_COUNTERS * fr + which; }
  // nothing hot and nothing exact (C_EXACT stays 0 off the masked route); the same two words for all threads of the frame
  RPSFS_HD static bool busy(const int* frame_counters) { return (frame_counters[C_HOT] | frame_counters[C_EXACT]) != 0; }
  RPSFS_HD bool idle(int fr) const { return !busy(counter(fr, 0)); }
};

struct Tables {  // what the host sized after its wait
  const int* info;  // FRAME_INFO per frame
  int* roots;       // frame fr: info[I_GROUPS] ascending frame-local roots from info[I_GROUP0] on
  int* stats;       // GROUP_STATS per group
  int* gframe;      // the group's frame
  int* order;       // F4: workgroup b takes group order[b]
  int* shared;      // SHARED_COUNTERS
  double* fills;
  long total;       // groups over all frames
  RPSFS_HD const int* of(int fr) const { return info + (size_t)FRAME_INFO * fr; }
};

// ------------------------------------------------------------------------------------------------ F1, F2
RPSFS_HD void b1_pad(long gid, int fr, const Stack& s, const float* images, size_t image_stride, double threshold) {
  f1_pad(gid, s.f, images + fr * image_stride, threshold, s.padded + fr * s.stride, s.bytes[0] + fr * s.stride, s.counter(fr, C_HOT));
}
// pass from bytes[from] into bytes[from ^ 1]
RPSFS_HD void b2_cross(long gid, int fr, const Stack& s, int from, int last) {
  if (s.idle(fr)) return;
  f2_cross(gid, s.f.PH, s.f.PW, s.bytes[from] + fr * s.stride, s.bytes[from ^ 1] + fr * s.stride, last ? s.counter(fr, C_MASK) : nullptr);
}
// The masked route: masks[fr] is frame fr's view (masks == null: no frame has one); the last pass of F2 takes the exact plane in
RPSFS_HD void b1_pad_masked(long gid, int fr, const Stack& s, const float* images, size_t image_stride, double threshold, const MaskView* masks,
                            int fill_nonfinite) {
  f1_pad_masked(gid, s.f, images + fr * image_stride, threshold, masks ? masks[fr] : MaskView{nullptr, 0, 0}, fill_nonfinite,
                s.padded + fr * s.stride, s.bytes[0] + fr * s.stride, s.exact + fr * s.stride, s.counter(fr, C_HOT), s.counter(fr, C_EXACT));
}
RPSFS_HD void b2_cross_merge(long gid, int fr, const Stack& s, int from) {
  if (s.idle(fr)) return;
  f2_cross_merge(gid, s.f.PH, s.f.PW, s.bytes[from] + fr * s.stride, s.exact + fr * s.stride, s.bytes[from ^ 1] + fr * s.stride, s.counter(fr, C_MASK));
}

// ------------------------------------------------------------------------------------------------ F3
// `at`: bytes[at] is the mask, bytes[at ^ 1] free; the grown mask goes to bytes[2]
RPSFS_HD void b3_rows(long gid, int fr, const Stack& s, int reach, int at) {
  if (s.idle(fr)) return;
  f3_rows(gid, s.f.PH, s.f.PW, reach, s.bytes[at] + fr * s.stride, s.bytes[at ^ 1] + fr * s.stride);
}
RPSFS_HD void b3_cols(long gid, int fr, const Stack& s, int reach, int at) {
  if (s.idle(fr)) return;
  f3_cols(gid, s.f.PH, s.f.PW, reach, s.bytes[at ^ 1] + fr * s.stride, s.bytes[2] + fr * s.stride);
}
template <class Ctx>
RPSFS_HD void b3_tile(Ctx& ctx, int fr, const Stack& s, int grown, int ty, int tx, int* ll) {
  if (s.idle(fr)) return;
  rpsfs::s3_tile(ctx, s.bytes[grown] + fr * s.stride, s.f.PH, s.f.PW, ty, tx, ll, s.labels + fr * s.stride);
}
RPSFS_HD void b3_seam(long gid, int fr, const Stack& s) {
  if (s.idle(fr)) return;
  rpsfs::s3_seam(gid, s.f.PH, s.f.PW, s.labels + fr * s.stride);
}
RPSFS_HD void b3_flatten(long gid, int fr, const Stack& s) {
  if (s.idle(fr)) return;
  rpsfs::s3_flatten(gid, s.f.npix(), s.labels + fr * s.stride);
}
RPSFS_HD void b3_count(long seg, int fr, const Stack& s) {
  if (s.idle(fr)) return;
  rpsfs::s4_count(seg, s.f.PH, s.f.PW, s.labels + fr * s.stride, s.segcnt + fr * s.nseg);
}
template <class Ctx>
RPSFS_HD void b3_scan(Ctx& ctx, int fr, const Stack& s, int* lds) {  // one workgroup of SCAN_THREADS per frame
  if (s.idle(fr)) return;
  rpsfs::s4_scan(ctx, (long)s.nseg, s.segcnt + fr * s.nseg, s.segoff + fr * s.nseg, s.counter(fr, C_GROUPS), lds);
}

// The host's step between the scan and the root list: info[] from the counters of `frames` frames; in_frame: H * W.
// Returns false when the counters contradict each other or the fill slots would not fit an int.
inline bool plan_tables(const int* counters, int frames, size_t in_frame, int* info, long* groups, long* masked, long* listed) {
  long g = 0, m = 0, l = 0;
  for (int fr = 0; fr < frames; ++fr) {
    const int* c = counters + (size_t)FRAME_COUNTERS * fr;
    int* o = info + (size_t)FRAME_INFO * fr;
    const bool hot = Stack::busy(c);
    if (hot && (c[C_GROUPS] <= 0 || c[C_MASK] <= 0)) return false;
    o[I_GROUP0] = (int)g, o[I_GROUPS] = hot ? c[C_GROUPS] : 0, o[I_LIST0] = (int)l;
    g += o[I_GROUPS];
    if (hot) m += c[C_MASK], l += (size_t)c[C_MASK] < in_frame ? (long)c[C_MASK] : (long)in_frame;
    if (g >= 0x7FFFFFF0L || m >= 0x7FFFFFF0L || l >= 0x7FFFFFF0L) return false;  // `slot` and the offsets are ints
  }
  *groups = g, *masked = m, *listed = l;
  return true;
}

RPSFS_HD void b3_roots(long seg, int fr, const Stack& s, const Tables& t) {
  if (s.idle(fr)) return;
  rpsfs::s4_roots(seg, s.f.PH, s.f.PW, s.labels + fr * s.stride, s.segoff + fr * s.nseg, t.roots + t.of(fr)[I_GROUP0]);
}
RPSFS_HD void b3_init(long k, int fr, const Tables& t) {
  const int* o = t.of(fr);
  if (k >= o[I_GROUPS]) return;
  f3_init(k, o[I_GROUPS], t.stats + (size_t)GROUP_STATS * o[I_GROUP0]);
  t.gframe[o[I_GROUP0] + k] = fr;
}
RPSFS_HD void b3_accumulate(long gid, int fr, const Stack& s, const Tables& t, int at) {
  if (s.idle(fr)) return;
  const int* o = t.of(fr);  // the search stays inside the frame's own slice of the root list
  f3_accumulate(gid, s.f.npix(), s.f.PW, s.bytes[at] + fr * s.stride, s.labels + fr * s.stride, t.roots + o[I_GROUP0], o[I_GROUPS],
                t.stats + (size_t)GROUP_STATS * o[I_GROUP0]);
}

// ------------------------------------------------------------------------------------------------ F4's order
// bucket 0 holds the longest groups: a group's bucket is 31 - floor(log2(masked pixels)), the leading zeros of its count
RPSFS_HD int order_bucket(int count) {
  int b = 0;
  for (unsigned v = count > 0 ? (unsigned)count : 1u; !(v & 0x80000000u); v <<= 1) ++b;
  return b;
}
RPSFS_HD void o_hist(long k, const Tables& t) {
  if (k >= t.total) return;
  fetch_add(t.shared + S_HIST + order_bucket(t.stats[GROUP_STATS * k]), 1);
}
// (after o_hist of ALL groups: a launch of its own).  Within a bucket the places go in the order the threads arrive.
RPSFS_HD void o_scatter(long k, const Tables& t) {
  if (k >= t.total) return;
  const int b = order_bucket(t.stats[GROUP_STATS * k]);
  int at = 0;
  for (int j = 0; j < b; ++j) at += t.shared[S_HIST + j];
  t.order[at + fetch_add(t.shared + S_TAKEN + b, 1)] = (int)k;
}

// ------------------------------------------------------------------------------------------------ F4
// Workgroup b of `t.total`: one group of whichever frame, on that frame's pointers; fills[] and its cursor are the frame-group's
template <class Ctx>
RPSFS_HD void b4_group(Ctx& ctx, long b, int order_mode, const Stack& s, const Tables& t, int at, int h, FillLds* L) {
  const long place = order_mode == ORDER_REVERSED ? t.total - 1 - b : b;
  const long g = order_mode == ORDER_FRAMES ? place : t.order[place];
  const int fr = t.gframe[g];
  f4_group(ctx, g, s.f.PH, s.f.PW, h, s.bytes[at] + fr * s.stride, t.roots, t.stats, s.padded + fr * s.stride, s.labels + fr * s.stride, t.fills,
           t.shared + S_CURSOR, L);
}

// ------------------------------------------------------------------------------------------------ F5
// corrected: per frame the rows of the padded frame from out_row0 on, c_stride apart; lists: frame fr's from info[I_LIST0] on
RPSFS_HD void b5_restore(long gid, int fr, const Stack& s, const int* info, int at, const float* images, size_t image_stride, const float* corrected,
                         size_t c_stride, int out_row0, float* outs, size_t out_stride, int32_t* lists) {
  const bool idle = s.idle(fr);
  f5_restore(gid, s.f, images + fr * image_stride, idle ? nullptr : s.bytes[at] + fr * s.stride, corrected + fr * c_stride, out_row0,
             outs + fr * out_stride, idle ? nullptr : lists + info[(size_t)FRAME_INFO * fr + I_LIST0], s.counter(fr, C_LIST));
}

}  // namespace rpsfsatb
