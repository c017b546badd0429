// rpsf_core_stars_shape.hpp - second moments and peak per detection of the star finder, shared with the CPU lane
// emulator tests/emu/emu_shapes.cpp.  A driver over a context as in rpsf_core_stars.hpp.
//
//   S5  s5_walk      one wave per row of the last detect (a component, or with the deblend option an object of a split one): a second
//                    walk over the bounding box, around the finished centroid - central moments, sum |d|, the peak and its first pixel
//
// The host describes every kept row (describe): which label array names its pixels, the box, the centroid.  Nothing here writes what
// S1 - S4 or D1 - D4 read; no atomics at all, no workgroup waits for another.  Two runs on one input agree bit for bit.
#pragma once
#include <vector>

#include "rpsf_core_stars_deblend.hpp"

#pragma clang fp contract(off)

namespace rpsfh {
using namespace rpsfs;

// the columns of a shape row (RPSF_STARS_SHAPE_COLUMNS of include/rpsf.h)
enum { COL_ROW, COL_COL, COL_FLUX, COL_AREA, COL_PEAK, COL_PEAK_ROW, COL_PEAK_COL, COL_ROW_MIN, COL_ROW_MAX, COL_COL_MIN, COL_COL_MAX,
       COL_ABS_FLUX, COL_RR, COL_CC, COL_RC, SHAPE_COLUMNS };

struct ShapeRow {  // one kept row of the last detect
  double rbar, cbar, flux, area;  // the row as rpsf_stars_positions returns it, bit for bit
  int root;                       // labels[] of the row's pixels
  int own;                        // owner[] of the row's pixels, or -1: the whole component
  int r0, r1, c0, c1;             // the bounding box, inclusive
};
// where a kept row came from (rpsfd::deblend_rows' `sources`): the component slot, and the object slot of a split component (else -1)
using Source = std::pair<long, long>;

// what one lane, or one group of 8, has seen: the four sums, the highest d and its first pixel (at < 0: no pixel yet)
struct Seen {
  double abs, rr, cc, rc, peak;
  long long at;
};
RPSFS_HD Seen nothing_seen() { return Seen{0.0, 0.0, 0.0, 0.0, 0.0, -1}; }
// the total order of the peak: larger d, then the smaller linear index
RPSFS_HD void see_peak(Seen& s, double d, long long at) {
  if (at < 0) return;
  if (s.at < 0 || d > s.peak || (d == s.peak && at < s.at)) s.peak = d, s.at = at;
}
RPSFS_HD Seen fold8(const Seen* p) {  // in index order
  Seen r = nothing_seen();
  for (int j = 0; j < 8; ++j) {
    r.abs += p[j].abs, r.rr += p[j].rr, r.cc += p[j].cc, r.rc += p[j].rc;
    see_peak(r, p[j].peak, p[j].at);
  }
  return r;
}

RPSFS_HD size_t s5_walk_lds_bytes() { return (size_t)(WALK_THREADS + WALK_WAVES * 8) * sizeof(Seen); }

// One workgroup, WALK_WAVES rows from `first` on, one wave each: lane j takes pixels j, j + 64, ... of the bounding box in raster order,
// skips those of another label and sums |d|, d (dr dr), d (dc dc), d (dr dc) with dr = r - rbar, dc = c - cbar, the products grouped as
// written; the 64 partial sums fold as 8 groups of 8, each in lane order, the peak with see_peak's order.  `owner` is only read for rows
// with own >= 0.  out[SHAPE_COLUMNS i ..]: the columns above, the sums of squares divided by the row's flux.
template <class Ctx>
RPSFS_HD void s5_walk(Ctx& ctx, const Frame& fr, const double* L, const int32_t* labels, const int32_t* owner, const ShapeRow* rows, long count,
                      long first, Seen* lds, double* out) {
  Seen* acc = lds;
  Seen* acc2 = lds + WALK_THREADS;
  const Mesh mesh{L, fr.nbx, 0, 0};
  ctx.each([&](int tid) {
    const long i = first + tid / WALK_LANES;
    const int lane = tid % WALK_LANES;
    Seen s = nothing_seen();
    if (i < count) {
      const ShapeRow row = rows[i];
      const long bw = row.c1 - row.c0 + 1, npx = (long)(row.r1 - row.r0 + 1) * bw;
      for (long j = lane; j < npx; j += WALK_LANES) {
        const int r = row.r0 + (int)(j / bw), c = row.c0 + (int)(j % bw);
        const size_t p = (size_t)r * fr.W + c;
        if (labels[p] != row.root || (row.own >= 0 && owner[p] != row.own)) continue;
        const double d = residual_at(fr, mesh, r, c);
        const double dr = (double)r - row.rbar, dc = (double)c - row.cbar;
        s.abs += std::fabs(d), s.rr += d * (dr * dr), s.cc += d * (dc * dc), s.rc += d * (dr * dc);
        see_peak(s, d, (long long)p);
      }
    }
    acc[tid] = s;
  });
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
    if (lane < 8) acc2[wave * 8 + lane] = fold8(acc + wave * WALK_LANES + 8 * lane);
  });
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES;
    const long i = first + wave;
    if (tid % WALK_LANES != 0 || i >= count) return;
    const Seen s = fold8(acc2 + wave * 8);
    const ShapeRow row = rows[i];
    double* o = out + SHAPE_COLUMNS * i;
    o[COL_ROW] = row.rbar, o[COL_COL] = row.cbar, o[COL_FLUX] = row.flux, o[COL_AREA] = row.area;
    o[COL_PEAK] = s.peak, o[COL_PEAK_ROW] = (double)(s.at / fr.W), o[COL_PEAK_COL] = (double)(s.at % fr.W);
    o[COL_ROW_MIN] = (double)row.r0, o[COL_ROW_MAX] = (double)row.r1, o[COL_COL_MIN] = (double)row.c0, o[COL_COL_MAX] = (double)row.c1;
    o[COL_ABS_FLUX] = s.abs, o[COL_RR] = s.rr / row.flux, o[COL_CC] = s.cc / row.flux, o[COL_RC] = s.rc / row.flux;
  });
}

// ------------------------------------------------------------------------------------------------ the descriptors (host)
// One ShapeRow per row of `found` ((row, col, flux, area) each) from the arrays S4 and D4 left: roots and stats (4 ints) per component,
// peaks and ostats (rpsfd::BOX ints) per object; the last two may be null when no source names an object.
inline std::vector<ShapeRow> describe(const std::vector<double>& found, const std::vector<Source>& sources, int W, const int* roots,
                                      const int* stats, const int* peaks, const int* ostats) {
  std::vector<ShapeRow> rows(sources.size());
  for (size_t i = 0; i < sources.size(); ++i) {
    const long k = sources[i].first, b = sources[i].second;
    ShapeRow& row = rows[i];
    row.rbar = found[4 * i], row.cbar = found[4 * i + 1], row.flux = found[4 * i + 2], row.area = found[4 * i + 3];
    row.root = roots[k];
    if (b < 0) {
      const int* st = stats + 4 * k;
      row.own = -1, row.r0 = row.root / W, row.r1 = st[1], row.c0 = st[2], row.c1 = st[3];
    } else {
      const int* box = ostats + rpsfd::BOX * b;
      row.own = peaks[b], row.r0 = box[1] / W, row.r1 = box[2], row.c0 = box[3], row.c1 = box[4];
    }
  }
  return rows;
}

}  // namespace rpsfh
