// rpsf_core_saturation.hpp - the saturation branch of apply on the device (csrc/saturation.hip), shared with the CPU lane emulator
// tests/emu/emu_saturation.cpp.  DESIGN.md 3.8 has the definition step by step.
//
// Written as rpsf_core_stars.hpp is: grid kernels without barriers are plain per-thread functions of the global thread index, the one
// workgroup kernel (F4) is a DRIVER over a context whose each(f) runs f(tid) for every thread and then a barrier; whatever the driver
// keeps between two each() calls is computed from LDS words that all threads read alike.
//
//   F1  f1_pad        4 pixels of the 2N-padded frame per thread: pad index map, float32 frame, hot byte (value > threshold), hot count
//       f1_pad_masked   the same with a bad-pixel mask: an EXACT byte per pixel beside the hot one (the caller's mask through the pad map, non-finite values)
//   F2  f2_cross      one pass of the cross element over the bytes, 4 pixels per thread; `dilation` passes make the mask
//       f2_cross_merge  the last pass on the masked route: the exact bytes are or-ed in undilated
//   F3  f3_rows, f3_cols   box dilation of the mask by box_reach(h), separable; the S3 / S4 drivers of rpsf_core_stars.hpp label it
//                          8-connected and list the roots; f3_init, f3_accumulate: count and bounding box of the MASKED pixels of a group
//   F4  f4_group      one wave per group: the group's bounding box in raster order, 64 pixels at a time; per masked pixel of the group
//                     the lanes load the window, the float64 sum runs in window raster order, the mean is kept as float64 for the
//                     pixels after it (as the host route keeps it) and stored as float32 in the frame
//   F5  f5_restore    raw values back on the mask, crop to H x W, the masked in-frame pixels listed for the host
//
// The only atomics are integer adds / min / max.  Two runs on one input give the same bits.
#pragma once
#include "rpsf_core_stars.hpp"

#pragma clang fp contract(off)

namespace rpsfsat {

using rpsfs::fetch_add;
using rpsfs::fetch_max;
using rpsfs::fetch_min;
using rpsfs::load_relaxed;

constexpr int FILL_LANES = 64;  // F4: one wave per workgroup, so every barrier of the driver is a wave's own
constexpr int GROUP_STATS = 5;  // per group: masked pixels, first row, last row, first column, last column

// np.pad's index maps, as the patch kernels evaluate them (rpsf_core.hpp, pad_index); -1: "the constant"
RPSFS_HD int pad_index(int i, int n, int mode) {
  if (i >= 0 && i < n) return i;
  switch (mode) {
    case 1: {  // symmetric
      int p = 2 * n, k = i % p;
      if (k < 0) k += p;
      return k < n ? k : p - 1 - k;
    }
    case 2: {  // reflect
      if (n == 1) return 0;
      int p = 2 * n - 2, k = i % p;
      if (k < 0) k += p;
      return k < n ? k : p - k;
    }
    case 3: return i < 0 ? 0 : n - 1;  // edge
    case 4: {                          // wrap
      int k = i % n;
      return k < 0 ? k + n : k;
    }
    default: return -1;
  }
}

// Python's slice arithmetic for [start, stop) over a length-n axis: a negative bound wraps once, an empty window has hi <= lo
RPSFS_HD void py_slice(long start, long stop, long n, long* lo, long* hi) {
  if (start < 0) start = start + n > 0 ? start + n : 0;
  if (stop < 0) stop = stop + n > 0 ? stop + n : 0;
  *lo = start < n ? start : n;
  *hi = stop < n ? stop : n;
}

// Two masked pixels influence each other only within h rows and h columns; boxes of this reach around them then touch or overlap
RPSFS_HD int box_reach(int h) { return h / 2; }  // ceil((h - 1) / 2)

struct Padded {  // the 2N-padded frame
  int H, W, N, PH, PW, pad_mode;
  RPSFS_HD long npix() const { return (long)PH * PW; }
};

struct alignas(16) Quad {
  float v[4];
};

// ------------------------------------------------------------------------------------------------ F1
// Thread gid: pixels 4 gid .. 4 gid + 3 of the padded frame in linear order (one 16-byte store of the frame, one 4-byte store of the bytes)
RPSFS_HD void f1_pad(long gid, const Padded& f, const float* image, double threshold, float* padded, uint8_t* hot, int* n_hot) {
  const long q0 = 4 * gid, npix = f.npix();
  if (q0 >= npix) return;
  Quad out;
  uint32_t bytes = 0;
  int count = 0;
  const int n = npix - q0 < 4 ? (int)(npix - q0) : 4;
  for (int k = 0; k < n; ++k) {
    const long q = q0 + k;
    const int r = (int)(q / f.PW), c = (int)(q % f.PW);
    const int sr = pad_index(r - 2 * f.N, f.H, f.pad_mode), sc = pad_index(c - 2 * f.N, f.W, f.pad_mode);
    const float v = (sr < 0 || sc < 0) ? 0.f : image[(size_t)sr * f.W + sc];
    out.v[k] = v;
    if ((double)v > threshold) bytes |= 1u << (8 * k), ++count;  // NaN is not hot
  }
  if (n == 4) {
    *reinterpret_cast<Quad*>(padded + q0) = out;
    *reinterpret_cast<uint32_t*>(hot + q0) = bytes;
  } else {
    for (int k = 0; k < n; ++k) padded[q0 + k] = out.v[k], hot[q0 + k] = (uint8_t)(bytes >> (8 * k));
  }
  if (count) fetch_add(n_hot, count);
}

// ------------------------------------------------------------------------------------------------ F1 with a bad-pixel mask
// The caller's mask of one frame: H x W bytes, nonzero = masked, element (r, c) at data + r * row_stride + c * col_stride (bytes,
// positive).  data == null: no mask.
struct MaskView {
  const uint8_t* data;
  long row_stride, col_stride;
};

RPSFS_HD bool nonfinite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7F800000u) == 0x7F800000u; }  // NaN, +Inf, -Inf

// f1_pad, and next to the hot byte the EXACT byte: the mask byte of the pad-mapped source pixel (0 where the pad is "the constant"),
// or-ed with "the padded value is not finite" when fill_nonfinite.  Exact pixels are masked as they are: F2 does not dilate them.
RPSFS_HD void f1_pad_masked(long gid, const Padded& f, const float* image, double threshold, MaskView m, int fill_nonfinite, float* padded,
                            uint8_t* hot, uint8_t* exact, int* n_hot, int* n_exact) {
  const long q0 = 4 * gid, npix = f.npix();
  if (q0 >= npix) return;
  Quad out;
  uint32_t bytes = 0, ebytes = 0;
  int count = 0, ecount = 0;
  const int n = npix - q0 < 4 ? (int)(npix - q0) : 4;
  for (int k = 0; k < n; ++k) {
    const long q = q0 + k;
    const int r = (int)(q / f.PW), c = (int)(q % f.PW);
    const int sr = pad_index(r - 2 * f.N, f.H, f.pad_mode), sc = pad_index(c - 2 * f.N, f.W, f.pad_mode);
    const bool inside = sr >= 0 && sc >= 0;
    const float v = inside ? image[(size_t)sr * f.W + sc] : 0.f;
    out.v[k] = v;
    if ((double)v > threshold) bytes |= 1u << (8 * k), ++count;  // NaN is not hot
    bool e = inside && m.data && m.data[sr * m.row_stride + sc * m.col_stride];
    if (fill_nonfinite && nonfinite(v)) e = true;
    if (e) ebytes |= 1u << (8 * k), ++ecount;
  }
  if (n == 4) {
    *reinterpret_cast<Quad*>(padded + q0) = out;
    *reinterpret_cast<uint32_t*>(hot + q0) = bytes;
    *reinterpret_cast<uint32_t*>(exact + q0) = ebytes;
  } else {
    for (int k = 0; k < n; ++k) padded[q0 + k] = out.v[k], hot[q0 + k] = (uint8_t)(bytes >> (8 * k)), exact[q0 + k] = (uint8_t)(ebytes >> (8 * k));
  }
  if (count) fetch_add(n_hot, count);
  if (ecount) fetch_add(n_exact, ecount);
}

// ------------------------------------------------------------------------------------------------ F2
// One pass of scipy's cross element, background outside: dst = src or any of its four neighbours.  n_set (optional) counts dst.
RPSFS_HD void f2_cross(long gid, int PH, int PW, const uint8_t* src, uint8_t* dst, int* n_set) {
  const long q0 = 4 * gid, npix = (long)PH * PW;
  if (q0 >= npix) return;
  uint32_t bytes = 0;
  int count = 0;
  const int n = npix - q0 < 4 ? (int)(npix - q0) : 4;
  for (int k = 0; k < n; ++k) {
    const long q = q0 + k;
    const int r = (int)(q / PW), c = (int)(q % PW);
    const bool on = src[q] || (c > 0 && src[q - 1]) || (c < PW - 1 && src[q + 1]) || (r > 0 && src[q - PW]) || (r < PH - 1 && src[q + PW]);
    if (on) bytes |= 1u << (8 * k), ++count;
  }
  if (n == 4) *reinterpret_cast<uint32_t*>(dst + q0) = bytes;
  else
    for (int k = 0; k < n; ++k) dst[q0 + k] = (uint8_t)(bytes >> (8 * k));
  if (n_set && count) fetch_add(n_set, count);
}
// F2's LAST pass with the exact plane carried along: dst = (src dilated once) or exact; n_set counts the union
RPSFS_HD void f2_cross_merge(long gid, int PH, int PW, const uint8_t* src, const uint8_t* exact, uint8_t* dst, int* n_set) {
  const long q0 = 4 * gid, npix = (long)PH * PW;
  if (q0 >= npix) return;
  uint32_t bytes = 0;
  int count = 0;
  const int n = npix - q0 < 4 ? (int)(npix - q0) : 4;
  for (int k = 0; k < n; ++k) {
    const long q = q0 + k;
    const int r = (int)(q / PW), c = (int)(q % PW);
    const bool on = exact[q] || src[q] || (c > 0 && src[q - 1]) || (c < PW - 1 && src[q + 1]) || (r > 0 && src[q - PW]) || (r < PH - 1 && src[q + PW]);
    if (on) bytes |= 1u << (8 * k), ++count;
  }
  if (n == 4) *reinterpret_cast<uint32_t*>(dst + q0) = bytes;
  else
    for (int k = 0; k < n; ++k) dst[q0 + k] = (uint8_t)(bytes >> (8 * k));
  if (count) fetch_add(n_set, count);
}

// ------------------------------------------------------------------------------------------------ F3
RPSFS_HD void f3_rows(long gid, int PH, int PW, int reach, const uint8_t* mask, uint8_t* tmp) {
  if (gid >= (long)PH * PW) return;
  const int c = (int)(gid % PW);
  const int a = c - reach > 0 ? c - reach : 0, b = c + reach < PW - 1 ? c + reach : PW - 1;
  uint8_t on = 0;
  for (int k = a; k <= b && !on; ++k) on = mask[gid - c + k];
  tmp[gid] = on;
}
RPSFS_HD void f3_cols(long gid, int PH, int PW, int reach, const uint8_t* tmp, uint8_t* grown) {
  if (gid >= (long)PH * PW) return;
  const int r = (int)(gid / PW);
  const int a = r - reach > 0 ? r - reach : 0, b = r + reach < PH - 1 ? r + reach : PH - 1;
  uint8_t on = 0;
  for (int k = a; k <= b && !on; ++k) on = tmp[gid + (long)(k - r) * PW];
  grown[gid] = on;
}
RPSFS_HD void f3_init(long k, long count, int* stats) {
  if (k >= count) return;
  int* s = stats + GROUP_STATS * k;
  s[0] = 0, s[1] = 0x7FFFFFFF, s[2] = -1, s[3] = 0x7FFFFFFF, s[4] = -1;
}
// labels: the smallest linear index of the pixel's component of the GROWN mask (-1 off it); only masked pixels count
RPSFS_HD void f3_accumulate(long gid, long npix, int PW, const uint8_t* mask, const int32_t* labels, const int* roots, long count, int* stats) {
  if (gid >= npix || !mask[gid]) return;
  int* s = stats + GROUP_STATS * rpsfs::s4_slot(roots, count, labels[gid]);
  const int r = (int)(gid / PW), c = (int)(gid % PW);
  fetch_add(s, 1);
  fetch_min(s + 1, r);
  fetch_max(s + 2, r);
  fetch_min(s + 3, c);
  fetch_max(s + 4, c);
}

// ------------------------------------------------------------------------------------------------ F4
struct FillLds {  // two copies of everything: what chunk n + 1 writes is not what the driver still reads of chunk n
  double v[2][FILL_LANES];  // a window element; NaN: not counted
  int mine[2][FILL_LANES];
  int base;
};

// Group g.  The group's masked pixels are visited in raster order of its bounding box - the frame's raster order among them, and no
// other group's pixel lies in any of their windows.  A visited pixel keeps its mean as float64 in fills[] (the host route's frame is
// float64 while it fills), its place there as -2 - slot in labels[], and the float32 value in the frame; a masked pixel not yet
// visited counts as NaN.  `cursor` hands every group its own stretch of fills[].
template <class Ctx>
RPSFS_HD void f4_group(Ctx& ctx, long g, int PH, int PW, int h, const uint8_t* mask, const int* roots, const int* stats, float* padded,
                       int32_t* labels, double* fills, int* cursor, FillLds* L) {
  const int root = roots[g];
  const int* s = stats + GROUP_STATS * g;
  const int count = s[0], r_first = s[1], c_first = s[3];
  const long bw = s[4] - c_first + 1, npx = (long)(s[2] - r_first + 1) * bw;
  ctx.each([&](int tid) {
    if (tid == 0) L->base = fetch_add(cursor, count);
  });
  const int base = L->base;
  int done = 0, wbuf = 0;
  for (long j0 = 0, chunk = 0; j0 < npx && done < count; j0 += FILL_LANES, ++chunk) {
    const int cb = (int)(chunk & 1);
    ctx.each([&](int tid) {
      const long j = j0 + tid;
      int mine = 0;
      if (j < npx) {
        const size_t p = (size_t)(r_first + j / bw) * PW + (c_first + j % bw);
        mine = mask[p] && load_relaxed(labels + p) == root;
      }
      L->mine[cb][tid] = mine;
    });
    unsigned long long bits = 0;  // (all 64 words are read at once; a test per word would wait for LDS 64 times)
    for (int t = 0; t < FILL_LANES; ++t) bits |= (unsigned long long)(L->mine[cb][t] != 0) << t;
    while (bits) {
      const int t = __builtin_ctzll(bits);
      bits &= bits - 1;
      const long i = r_first + (j0 + t) / bw, j = c_first + (j0 + t) % bw;
      long r0, r1, c0, c1;
      py_slice(i - h, i + h, PH, &r0, &r1);
      py_slice(j - h, j + h, PW, &c0, &c1);
      const long ww = c1 - c0, n = (r1 > r0 && ww > 0) ? (r1 - r0) * ww : 0;
      double sum = 0.0;
      long cnt = 0;
      for (long w0 = 0; w0 < n; w0 += FILL_LANES) {
        wbuf ^= 1;
        const int wb = wbuf;
        ctx.each([&](int tid) {
          const long w = w0 + tid;
          double v = std::nan("");
          if (w < n) {
            const size_t p = (size_t)(r0 + w / ww) * PW + (c0 + w % ww);
            const int m = mask[p], l = labels[p];  // three loads that do not wait for each other; a masked pixel's label is this group's own
            const float x = padded[p];
            if (!m) v = (double)x;
            else if (l < -1) v = fills[-2 - l];
          }
          L->v[wb][tid] = v;
        });
        for (int e = 0; e < FILL_LANES; ++e) {  // window raster order; no branch, so that the 64 reads are in flight together
          const double v = L->v[wb][e], with = sum + v;
          const bool ok = v == v;
          sum = ok ? with : sum, cnt += ok;
        }
      }
      const double mean = cnt ? sum / (double)cnt : std::nan("");
      const int slot = base + done;
      ctx.each([&](int tid) {
        if (tid != 0) return;
        const size_t p = (size_t)i * PW + j;
        fills[slot] = mean, padded[p] = (float)mean, labels[p] = -2 - slot;
      });
      ++done;
    }
  }
}

// ------------------------------------------------------------------------------------------------ F5
// Thread gid: pixel gid of the H x W result.  `corrected` holds the rows of the padded frame from row out_row0 on; mask == null: nothing was hot.
RPSFS_HD void f5_restore(long gid, const Padded& f, const float* image, const uint8_t* mask, const float* corrected, int out_row0, float* out,
                         int32_t* list, int* n_list) {
  if (gid >= (long)f.H * f.W) return;
  const int r = (int)(gid / f.W), c = (int)(gid % f.W);
  const size_t p = (size_t)(r + 2 * f.N) * f.PW + (c + 2 * f.N);
  if (mask && mask[p]) {
    out[gid] = image[gid];
    list[fetch_add(n_list, 1)] = (int32_t)gid;
  } else {
    out[gid] = corrected[p - (size_t)out_row0 * f.PW];
  }
}

}  // namespace rpsfsat
