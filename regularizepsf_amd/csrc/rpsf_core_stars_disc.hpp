// rpsf_core_stars_disc.hpp - what the per-star kernels S6 - S9, S11 and S12 share (DESIGN.md 3.7 "The disc walk"): the box of a disc and
// the walk over it, the field-major records a workgroup keeps in LDS, and the steps of the fold 64 partials -> 8 -> 1.  Plain per-thread
// code, shared with the CPU lane emulators (tests/emu/emu_disc.cpp tests it alone): nothing here calls ctx.each(); the drivers call these
// from inside their own each() bodies, so the barriers stay where each driver has them.
#pragma once
#include "rpsf_core_stars_shape.hpp"

#pragma clang fp contract(off)

namespace rpsfk {
using namespace rpsfs;

// ------------------------------------------------------------------------------------------------ the box and the walk
// The box of the disc of radius R around (y, x): rows floor(y - R) - 1 .. ceil(y + R) + 1 and likewise in x, NOT clipped to the frame.
struct DiscBox {
  int r0, r1, c0, c1;
  long bw, npx;  // the box's width and its number of pixels
};
RPSFS_HD DiscBox disc_box(double y, double x, double R) {
  const int r0 = (int)std::floor(y - R) - 1, r1 = (int)std::ceil(y + R) + 1;
  const int c0 = (int)std::floor(x - R) - 1, c1 = (int)std::ceil(x + R) + 1;
  const long bw = c1 - c0 + 1, npx = (long)(r1 - r0 + 1) * bw;
  return DiscBox{r0, r1, c0, c1, bw, npx};
}

// One lane's share of the walk over the disc q <= R2 around (y, x): the box's pixels lane, lane + 64, ... in raster order.  For pixel
// (r, c): pr = r - y, pc = c - x, q = pr pr + pc pc, in this order of operations; it is in the disc when q <= R2 (false for a NaN).
// in_disc(pr, pc) is called for every pixel of the disc, on the frame or off it; then usable_pixel(r, c, p, pr, pc, q), p = r W + c, for
// those that lie on the frame and are usable().  Counting and summing are the caller's: a caller may leave out more pixels yet.
template <class InDisc, class UsablePixel>
RPSFS_HD void walk_disc(const Frame& fr, const DiscBox& b, double y, double x, double R2, int lane, InDisc&& in_disc,
                        UsablePixel&& usable_pixel) {
  for (long j = lane; j < b.npx; j += WALK_LANES) {
    const int r = b.r0 + (int)(j / b.bw), c = b.c0 + (int)(j % b.bw);
    const double pr = (double)r - y, pc = (double)c - x;
    const double q = pr * pr + pc * pc;
    if (!(q <= R2)) continue;
    in_disc(pr, pc);
    if (r < 0 || r >= fr.H || c < 0 || c >= fr.W) continue;
    const size_t p = (size_t)r * fr.W + c;
    if (!usable(fr.img, fr.mask, p)) continue;
    usable_pixel(r, c, p, pr, pc, q);
  }
}
// (a walk that takes nothing from the pixels off the frame)
template <class UsablePixel>
RPSFS_HD void walk_disc(const Frame& fr, const DiscBox& b, double y, double x, double R2, int lane, UsablePixel&& usable_pixel) {
  walk_disc(fr, b, y, x, R2, lane, [](double, double) {}, usable_pixel);
}

// ------------------------------------------------------------------------------------------------ the residual's peak
// the total order of the residual's peak: larger |e| (a NaN counts as +inf), then the smaller linear index
RPSFS_HD double peak_key(double e) {
  const double a = std::fabs(e);
  return a == a ? a : (double)INFINITY;
}
struct Peak {
  double e;
  long long at;
};
RPSFS_HD void see_residual(Peak& s, double e, long long at) {
  if (at < 0) return;
  const double k = peak_key(e), have = peak_key(s.e);
  if (s.at < 0 || k > have || (k == have && at < s.at)) s.e = e, s.at = at;
}

// ------------------------------------------------------------------------------------------------ the records in LDS
// n records at `base` (a multiple of 16 bytes: n is a multiple of 4), FIELD-MAJOR: field f of record i of n is word f n + i, so that
// neighbouring lanes touch neighbouring words.  A record is DOUBLES doubles, then - HAS_AT - the linear index of a peak (64 bits, < 0: no
// pixel yet), then COUNTS ints.  A driver keeps one record per lane (n = WALK_THREADS) and behind them one per group of 8 lanes
// (n = WALK_WAVES 8).
template <int DOUBLES, bool HAS_AT, int COUNTS>
struct LaneRecords {
  double* d;
  long long* at;  // (null without HAS_AT)
  int* cnt;
  int n;
  static constexpr size_t bytes() { return (size_t)DOUBLES * 8 + (HAS_AT ? 8 : 0) + (size_t)COUNTS * 4; }  // of one record
  RPSFS_HD LaneRecords(void* base, int n_) : d(static_cast<double*>(base)), n(n_) {
    double* end = d + (size_t)DOUBLES * n_;
    at = HAS_AT ? reinterpret_cast<long long*>(end) : nullptr;
    cnt = reinterpret_cast<int*>(HAS_AT ? end + n_ : end);
  }
};
constexpr int WALK_GROUPS = WALK_WAVES * 8;  // the groups of 8 lanes of a workgroup
// the bytes of a driver's records: one per lane, one per group
template <class Records>
RPSFS_HD constexpr size_t walk_records_bytes() {
  return (size_t)(WALK_THREADS + WALK_GROUPS) * Records::bytes();
}

// ------------------------------------------------------------------------------------------------ the fold
// The 64 partial records of a wave fold as 8 groups of 8, each in lane order, and the 8 groups in order; every sum starts from 0.0 (0).
// `acc` holds the lanes' records, `acc2` the groups'.  The step 64 -> 8 is for the first 8 lanes of a wave (thread tid folds records
// 8 lane .. 8 lane + 7 of its wave into group record 8 wave + lane), the step 8 -> 1 for a wave's first lane; the caller picks the
// threads, these only compute.
RPSFS_HD double sum8(const double* v) {
  double s = 0.0;
  for (int j = 0; j < 8; ++j) s += v[j];
  return s;
}
RPSFS_HD int sum8(const int* v) {
  int s = 0;
  for (int j = 0; j < 8; ++j) s += v[j];
  return s;
}
RPSFS_HD Peak peak8(const double* e, const long long* at) {
  Peak seen{0.0, -1};
  for (int j = 0; j < 8; ++j) see_residual(seen, e[j], at[j]);
  return seen;
}
RPSFS_HD int fold_from(int tid) { return tid / WALK_LANES * WALK_LANES + 8 * (tid % WALK_LANES); }  // the first of a thread's 8 lane records
RPSFS_HD int fold_to(int tid) { return tid / WALK_LANES * 8 + tid % WALK_LANES; }                    // its group record

// the doubles 0 .. fields - 1
template <class Records>
RPSFS_HD void fold_sums_64to8(const Records& acc, const Records& acc2, int tid, int fields) {
  for (int f = 0; f < fields; ++f) acc2.d[f * acc2.n + fold_to(tid)] = sum8(acc.d + f * acc.n + fold_from(tid));
}
template <class Records>
RPSFS_HD void fold_sums_8to1(const Records& acc2, int wave, int fields, double* out) {
  for (int f = 0; f < fields; ++f) out[f] = sum8(acc2.d + f * acc2.n + wave * 8);
}
// the ints 0 .. counts - 1
template <class Records>
RPSFS_HD void fold_counts_64to8(const Records& acc, const Records& acc2, int tid, int counts) {
  for (int f = 0; f < counts; ++f) acc2.cnt[f * acc2.n + fold_to(tid)] = sum8(acc.cnt + f * acc.n + fold_from(tid));
}
template <class Records>
RPSFS_HD void fold_counts_8to1(const Records& acc2, int wave, int counts, int* out) {
  for (int f = 0; f < counts; ++f) out[f] = sum8(acc2.cnt + f * acc2.n + wave * 8);
}
// the residual's peak: its signed e in double `field`, its pixel in `at`
template <class Records>
RPSFS_HD void fold_peak_64to8(const Records& acc, const Records& acc2, int tid, int field) {
  const Peak seen = peak8(acc.d + field * acc.n + fold_from(tid), acc.at + fold_from(tid));
  acc2.d[field * acc2.n + fold_to(tid)] = seen.e, acc2.at[fold_to(tid)] = seen.at;
}
template <class Records>
RPSFS_HD Peak fold_peak_8to1(const Records& acc2, int wave, int field) {
  return peak8(acc2.d + field * acc2.n + wave * 8, acc2.at + wave * 8);
}

}  // namespace rpsfk
