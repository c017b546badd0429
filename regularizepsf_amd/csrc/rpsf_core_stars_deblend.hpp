// rpsf_core_stars_deblend.hpp - the star finder's deblend option, shared with the CPU lane emulator
// tests/emu/emu_deblend.cpp.  Drivers over a context and per-thread grid functions as in rpsf_core_stars.hpp.
//
//   D1  d1_up        per pixel: the highest of the pixel and its detected 8-neighbours in the order (f, then the smaller index)
//       d1_peak      per pixel, in a launch of its own: the fixed point of following `up` - nothing is written while anybody walks
//   D2  the peaks in index order by S4's s4_count / s4_scan / s4_roots on the `peak` array;
//       d2_init, d2_accumulate   area, first pixel, bounding box by integer atomics; the saddle by integer max on 64-bit value keys
//       d_walk       one wave per basin that has a neighbour: sum d over its bounding box in S4's fixed order
//   D3  d3_significant   one thread per basin: the three tests, the count of significant basins per component by integer add
//   D4  d4_own       one workgroup per split component: every pixel of an insignificant basin goes to the nearest significant peak of
//                    its component (integer squared distance, then the smaller index); the peaks are gathered chunk by chunk, so their
//                    number has no bound.  Area, first pixel and box of each object by integer atomics.
//       d_walk       one wave per object: S4's moments over the object's bounding box
//
// The walks strictly ascend in a strict total order, so each ends; no workgroup waits for another; the only atomics are integer
// add / min / max.  Two runs on one input agree bit for bit.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "rpsf_core_stars.hpp"

#pragma clang fp contract(off)

namespace rpsfd {
using namespace rpsfs;

constexpr int OWN_THREADS = 256;  // D4: pixels per batch and peaks per chunk
constexpr int BOX = 5;            // ints per basin or object: area, first pixel, last row, first column, last column

#if defined(__HIP_DEVICE_COMPILE__)
RPSFS_HD void max_u64(uint64_t* p, uint64_t v) { atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
#else
RPSFS_HD void max_u64(uint64_t* p, uint64_t v) { if (v > *p) *p = v; }
#endif

// order-preserving map of the doubles onto unsigned integers; every key is above 0, which marks "no saddle"
RPSFS_HD uint64_t key64(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
RPSFS_HD double value64(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  double x;
  std::memcpy(&x, &u, 8);
  return x;
}

// ------------------------------------------------------------------------------------------------ D1
// p above q: a strict total order on pixels with comparable f
RPSFS_HD bool above(const double* f, int p, int q) { return f[p] > f[q] || (f[p] == f[q] && p < q); }

RPSFS_HD void d1_up(long gid, int H, int W, const double* f, const uint8_t* det, int32_t* up) {
  if (gid >= (long)H * W) return;
  if (!det[gid]) {
    up[gid] = -1;
    return;
  }
  const int r = (int)(gid / W), c = (int)(gid % W);
  int best = (int)gid;
  for (int dr = -1; dr <= 1; ++dr)
    for (int dc = -1; dc <= 1; ++dc) {
      const int qr = r + dr, qc = c + dc;
      if ((dr == 0 && dc == 0) || qr < 0 || qr >= H || qc < 0 || qc >= W) continue;
      const int q = qr * W + qc;
      if (det[q] && above(f, q, best)) best = q;
    }
  up[gid] = best;
}

// every step goes to a pixel strictly above: the walk ends at a pixel with up == itself.  `up` is complete and read-only here.
RPSFS_HD void d1_peak(long gid, long npix, const int32_t* up, int32_t* peak) {
  if (gid >= npix) return;
  if (up[gid] < 0) {
    peak[gid] = -1;
    return;
  }
  int x = (int)gid;
  for (;;) {
    const int n = up[x];
    if (n == x) break;
    x = n;
  }
  peak[gid] = x;
}

// ------------------------------------------------------------------------------------------------ D2
RPSFS_HD void box_init(int* box, int q, int W) { box[0] = 0, box[1] = q, box[2] = q / W, box[3] = box[4] = q % W; }
RPSFS_HD void box_add(int* box, int p, int W) {
  fetch_add(box, 1);
  fetch_min(box + 1, p);
  fetch_max(box + 2, p / W);
  fetch_min(box + 3, p % W);
  fetch_max(box + 4, p % W);
}

RPSFS_HD void d2_init(long b, long nb, int W, const int* peaks, int* bstats, uint64_t* saddle) {
  if (b >= nb) return;
  box_init(bstats + BOX * b, peaks[b], W);
  saddle[b] = 0;
}
// pixel gid into its basin's area and box; min(f(p), f(q)) of every 8-adjacent pair across two basins into the saddle of p's basin
// (the pair is met again from q, for q's basin)
RPSFS_HD void d2_accumulate(long gid, int H, int W, const double* f, const int32_t* peak, const int* peaks, long nb, int* bstats,
                            uint64_t* saddle) {
  if (gid >= (long)H * W) return;
  const int mine = peak[gid];
  if (mine < 0) return;
  const long b = s4_slot(peaks, nb, mine);
  box_add(bstats + BOX * b, (int)gid, W);
  const int r = (int)(gid / W), c = (int)(gid % W);
  uint64_t best = 0;
  for (int dr = -1; dr <= 1; ++dr)
    for (int dc = -1; dc <= 1; ++dc) {
      const int qr = r + dr, qc = c + dc;
      if ((dr == 0 && dc == 0) || qr < 0 || qr >= H || qc < 0 || qc >= W) continue;
      const int q = qr * W + qc;
      if (peak[q] < 0 || peak[q] == mine) continue;
      const uint64_t k = key64(f[gid] < f[q] ? f[gid] : f[q]);
      if (k > best) best = k;
    }
  if (best) max_u64(saddle + b, best);
}
// a basin without a neighbour is its whole component: nothing hangs on its flux
RPSFS_HD void d2_want(long b, long nb, const uint64_t* saddle, uint8_t* want) {
  if (b < nb) want[b] = saddle[b] != 0;
}

// ------------------------------------------------------------------------------------------------ the walk of D2 and D4
struct Objects {
  const int32_t* own;   // per pixel: the peak of the basin (D2) or of the object (D4) the pixel belongs to
  const int* peaks;     // ascending
  const int* box;       // BOX ints per peak
  const uint8_t* want;  // 0: not walked, zeros
  long n;
};

// s4_walk over objects: one wave per object from `first` on; lane j takes pixels j, j + 64, ... of the bounding box in raster order,
// the 64 partial sums fold as 8 groups of 8.  A pixel belongs to the object when it lies in the peak's component and own[] names the
// peak (own[] is only defined inside the components that D4 split).  out[4b ..] = sum d, sum d * row, sum d * col, area.
template <class Ctx>
RPSFS_HD void d_walk(Ctx& ctx, const Frame& fr, const double* L, const int32_t* labels, const Objects& o, long first, double* lds, double* out) {
  double* acc = lds;
  double* acc2 = lds + WALK_THREADS * 3;
  const Mesh mesh{L, fr.nbx, 0, 0};
  ctx.each([&](int tid) {
    const long b = first + tid / WALK_LANES;
    const int lane = tid % WALK_LANES;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (b < o.n && o.want[b]) {
      const int* box = o.box + BOX * b;
      const int q = o.peaks[b], root = labels[q], r0 = box[1] / fr.W, c0 = box[3];
      const long bw = box[4] - c0 + 1, npx = (long)(box[2] - r0 + 1) * bw;
      for (long j = lane; j < npx; j += WALK_LANES) {
        const int r = r0 + (int)(j / bw), c = c0 + (int)(j % bw);
        const size_t p = (size_t)r * fr.W + c;
        if (labels[p] != root || o.own[p] != q) continue;
        const double d = residual_at(fr, mesh, r, c);
        s0 += d, s1 += d * (double)r, s2 += d * (double)c;
      }
    }
    acc[3 * tid] = s0, acc[3 * tid + 1] = s1, acc[3 * tid + 2] = s2;
  });
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
    if (lane >= 8) return;
    for (int m = 0; m < 3; ++m) {
      double s = 0.0;
      for (int j = 0; j < 8; ++j) s += acc[3 * (wave * WALK_LANES + 8 * lane + j) + m];
      acc2[3 * (wave * 8 + lane) + m] = s;
    }
  });
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES;
    const long b = first + wave;
    if (tid % WALK_LANES != 0 || b >= o.n) return;
    for (int m = 0; m < 3; ++m) {
      double s = 0.0;
      for (int j = 0; j < 8; ++j) s += acc2[3 * (wave * 8 + j) + m];
      out[4 * b + m] = s;
    }
    out[4 * b + 3] = (double)o.box[BOX * b];
  });
}

// ------------------------------------------------------------------------------------------------ D3
struct Significance {
  long min_area;
  double contrast, prominence, T;
};
// basin b: its component's slot, the three tests, one more significant basin for the component; the object's box starts at the peak.
// (nsig is zeroed before the launch.)
RPSFS_HD void d3_significant(long b, long nb, int W, const double* f, const int32_t* labels, const int* roots, long count, const double* moments,
                             const int* peaks, const int* bstats, const uint64_t* saddle, const double* bflux, const Significance& s,
                             int* bcomp, uint8_t* sig, int* nsig, int* ostats) {
  if (b >= nb) return;
  const int q = peaks[b];
  const long k = s4_slot(roots, count, labels[q]);
  bcomp[b] = (int)k;
  bool yes = false;
  if (saddle[b] != 0) {
    const double share = s.contrast * moments[4 * k], need = s.prominence * s.T, rise = f[q] - value64(saddle[b]);
    yes = bstats[BOX * b] >= s.min_area && bflux[4 * b] >= share && rise >= need;
  }
  sig[b] = yes;
  if (yes) fetch_add(nsig + k, 1);
  box_init(ostats + BOX * b, q, W);
}

// ------------------------------------------------------------------------------------------------ D4
RPSFS_HD size_t d4_own_lds_bytes() { return (size_t)OWN_THREADS * (sizeof(long long) + 3 * sizeof(int)); }

// Component k, if it has two or more significant basins: owner[p] for each of its pixels.  The pixels of the bounding box go in
// batches of OWN_THREADS, one per thread; per batch the basins whose peaks can lie in the component (slots lo .. hi of the ascending
// peak list) pass through LDS in chunks of OWN_THREADS.  Chunks and their entries ascend in peak index, so on equal distance the
// first seen - the smaller index - stays.
template <class Ctx>
RPSFS_HD void d4_own(Ctx& ctx, int W, const int32_t* labels, const int* roots, const int* stats, long k, const int32_t* peak, const int* peaks,
                     long nb, const int* bcomp, const uint8_t* sig, const int* nsig, void* lds, int32_t* owner, int* ostats) {
  if (nsig[k] < 2) return;
  long long* bestd = static_cast<long long*>(lds);
  int* besti = reinterpret_cast<int*>(bestd + OWN_THREADS);
  int* pix = besti + OWN_THREADS;
  int* chunk = pix + OWN_THREADS;
  const int root = roots[k], r0 = root / W, c0 = stats[4 * k + 2];
  const long bw = stats[4 * k + 3] - c0 + 1, npx = (long)(stats[4 * k + 1] - r0 + 1) * bw;
  const long lo = s4_slot(peaks, nb, root);  // the root is the component's first pixel: no peak of it lies before
  const int last = stats[4 * k + 1] * W + stats[4 * k + 3];
  long hi = s4_slot(peaks, nb, last);  // the first slot with peaks[slot] >= last, or nb - 1
  hi = peaks[hi] <= last ? hi + 1 : hi;
  for (long base = 0; base < npx; base += OWN_THREADS) {
    ctx.each([&](int tid) {
      const long j = base + tid;
      pix[tid] = -1, bestd[tid] = -1, besti[tid] = -1;
      if (j >= npx) return;
      const int p = (r0 + (int)(j / bw)) * W + c0 + (int)(j % bw);
      if (labels[p] != root) return;
      if (sig[s4_slot(peaks, nb, peak[p])]) besti[tid] = peak[p];  // a pixel of a significant basin stays
      pix[tid] = p;
    });
    for (long cb = lo; cb < hi; cb += OWN_THREADS) {
      ctx.each([&](int tid) {
        const long b = cb + tid;
        chunk[tid] = (b < hi && bcomp[b] == k && sig[b]) ? peaks[b] : -1;
      });
      ctx.each([&](int tid) {
        const int p = pix[tid];
        if (p < 0 || (besti[tid] >= 0 && bestd[tid] < 0)) return;
        long long d = bestd[tid];
        int at = besti[tid];
        for (int e = 0; e < OWN_THREADS; ++e) {
          const int q = chunk[e];
          if (q < 0) continue;
          const long long dr = p / W - q / W, dc = p % W - q % W, dq = dr * dr + dc * dc;
          if (at < 0 || dq < d) d = dq, at = q;
        }
        bestd[tid] = d, besti[tid] = at;
      });
    }
    ctx.each([&](int tid) {
      const int p = pix[tid];
      if (p < 0) return;
      owner[p] = besti[tid];
      box_add(ostats + BOX * s4_slot(peaks, nb, besti[tid]), p, W);
    });
  }
}

// the objects whose moments are wanted: significant basins of split components with an area inside the limits
RPSFS_HD void d4_want(long b, long nb, const int* bcomp, const uint8_t* sig, const int* nsig, const int* ostats, long min_area, long max_area,
                      uint8_t* want) {
  if (b >= nb) return;
  const int area = ostats[BOX * b];
  want[b] = sig[b] && nsig[bcomp[b]] >= 2 && area >= min_area && (max_area < 0 || area <= max_area);
}

// ------------------------------------------------------------------------------------------------ the rows (host)
// Rows (row, col, flux, area) in raster order of each object's first pixel: an unsplit component is S4's row (first pixel: its root),
// a split one gives its objects.  *split: the number of split components.  `sources`, when given, receives per kept row the component
// slot and the object slot (-1 for an unsplit component).
inline std::vector<double> deblend_rows(long count, const int* roots, const double* moments, const int* nsig, long nb, const int* bcomp,
                                        const uint8_t* sig, const int* ostats, const double* omoments, long min_area, long max_area,
                                        size_t* split, std::vector<std::pair<long, long>>* sources = nullptr) {
  std::vector<std::pair<int, long>> order;  // (first pixel, slot): component k as k, object b as count + b; first pixels are distinct
  *split = 0;
  for (long k = 0; k < count; ++k) {
    if (nsig[k] >= 2) ++*split;
    else order.emplace_back(roots[k], k);
  }
  for (long b = 0; b < nb; ++b)
    if (sig[b] && nsig[bcomp[b]] >= 2) order.emplace_back(ostats[BOX * b + 1], count + b);
  std::sort(order.begin(), order.end());
  std::vector<double> rows;
  if (sources) sources->clear();
  for (const auto& [first, slot] : order) {
    const long b = slot - count;
    const double* m = b < 0 ? moments + 4 * slot : omoments + 4 * b;
    const double flux = m[0], area = m[3];
    if (area < (double)min_area || (max_area >= 0 && area > (double)max_area) || !(flux > 0.0)) continue;
    rows.insert(rows.end(), {m[1] / flux, m[2] / flux, flux, area});
    if (sources) sources->emplace_back(b < 0 ? slot : (long)bcomp[b], b < 0 ? -1 : b);
  }
  return rows;
}

}  // namespace rpsfd
