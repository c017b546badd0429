// rpsf_core_builder_sub.hpp - kernel B1n of the PSF builder (csrc/builder.hip): B1 with the fitted neighbours of every star taken out of its
// patch while it is gathered (DESIGN.md 3.6 "Neighbour-subtracted patches"), and the host's neighbour lists beside it.  Shared with the
// CPU lane emulator tests/emu/emu_builder_sub.cpp: as in rpsf_core_builder.hpp every function does the work of ONE thread of a workgroup
// between two barriers.
//
//   B1n  one workgroup per patch, B1's launch shape and LDS block.  Phase 1 of B1 (the gather) is replaced by phase 1n; the tap tables, the
//        two prefilter passes, the separable shift, the zero / non-finite scan, the plane fit and phase 5 are rpsf_core_builder.hpp's own
//        functions, called and not copied (regularizepsf/image_processing.py:82-121 is what they restate, unchanged).
//
// PHASE 1n.  For patch pixel (r, c) with (rr, rc) the rounded corner: fr = mirror_index(rr + r, H), fc = mirror_index(rc + c, W); s = 0.0;
// for j ascending over the patch's neighbour list: pr = fr - y_j, pc = fc - x_j, q = pr pr + pc pc, and when q <= R R:
// s = s + flux_j * model_at(cube + cell_j N_m^2, N_m, h, pr, pc) with h = N_m / 2 - 0.5 - the comparison, model_at and h spelled as S8 and
// S10 spell them (rpsf_core_stars_fit.hpp, rpsf_core_stars_render.hpp), contraction off.  The patch value is
// (double)(float)((double)img[fr W + fc] - s): the float32 rounding makes it, bit for bit, what B1 reads from the float32 frame S10 writes
// in its residual mode with every star of the list drawn, and a pixel no neighbour reaches keeps the frame's own bits.
// The sum lives in the pixel's own float64 slot of the patch between the chunks, so it costs no register; the neighbour records are staged
// into LDS RENDER_CHUNK at a time as S10 stages them, behind B1's block.  A pixel is touched by one thread only, the order of its sum is
// the order of the list: no atomics, no scratch, no workgroup waits for another, two runs agree bit for bit.
// A patch whose list is empty takes B1's own gather instead: with s = 0.0 the value above is (double)img[fr W + fc] itself for every pixel that
// is not NaN, and a NaN pixel rejects the patch either way.  (It does not make the patch as cheap as in B1: measured, B1n with every list empty
// stays 11 % above B1)
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "rpsf_core_builder.hpp"
#include "rpsf_core_stars_render.hpp"

#pragma clang fp contract(off)

namespace rpsfbn {

constexpr int CHUNK = rpsfn::RENDER_CHUNK;
constexpr int BUCKET = 32;  // pixels per side of a bucket of the host's grid

// what B1n reads besides B1's own arguments: the subtraction set as the host uploaded it and the patches' neighbour lists
struct Sub {
  const double* cube;  // n_cells x N_m x N_m
  int model_n;         // N_m
  double R2, h;        // R R and the star's centre in a cell, N_m / 2.0 - 0.5
  const double* pos;   // (row, col) per star of the set
  const double* flux;
  const int* cell;
  const long long* offsets;  // offsets[k] .. offsets[k + 1] of `index` are patch k's neighbours, ascending
  const int* index;
};

// LDS of one B1n workgroup: B1's block, then one chunk of records, field-major as S10's (rows, columns, fluxes as float64, cells as int32)
RPSFB_HD size_t chunk_bytes() { return (size_t)CHUNK * (3 * 8 + 4); }
RPSFB_HD size_t lds_bytes(int N) { return rpsfb::lds_bytes(N) + chunk_bytes(); }
struct Chunk {
  double *row, *col, *flux;
  int* cell;
};
RPSFB_HD Chunk carve_chunk(void* base, int N) {
  Chunk k;
  k.row = reinterpret_cast<double*>(static_cast<char*>(base) + rpsfb::lds_bytes(N));  // (a multiple of 8: B1's block is doubles, then an even number of ints)
  k.col = k.row + CHUNK;
  k.flux = k.col + CHUNK;
  k.cell = reinterpret_cast<int*>(k.flux + CHUNK);
  return k;
}

// phase 1n-a: the sums start at 0.0, B1's flags at 0.  A thread writes only the pixels it alone reads in 1n-c and 1n-d: no barrier follows.
RPSFB_HD void b1n_begin(int tid, int nthreads, int N, const rpsfb::Lds& s) {
  const int ld = rpsfb::ld_for(N);
  for (int p = tid; p < N * N; p += nthreads) s.patch[(p / N) * ld + p % N] = 0.0;
  if (tid < 3) s.flag[tid] = 0;
}
// phase 1n-b: threads 0 .. len - 1 stage one record of the list each, `first` on
RPSFB_HD void b1n_stage(int tid, const Sub& sub, long long first, int len, const Chunk& k) {
  if (tid >= len) return;
  const int i = sub.index[first + tid];
  k.row[tid] = sub.pos[2 * (size_t)i], k.col[tid] = sub.pos[2 * (size_t)i + 1], k.flux[tid] = sub.flux[i], k.cell[tid] = sub.cell[i];
}
// phase 1n-c (after a barrier; another one before the next 1n-b): every pixel takes the chunk's records in order
RPSFB_HD void b1n_add(int tid, int nthreads, int N, int H, int W, int rr, int rc, const Sub& sub, int len, const Chunk& k, const rpsfb::Lds& s) {
  const int ld = rpsfb::ld_for(N);
  const size_t cell_words = (size_t)sub.model_n * sub.model_n;
  for (int p = tid; p < N * N; p += nthreads) {
    const int r = p / N, c = p % N;
    const int fr = rpsfb::mirror_index((long)rr + r, H), fc = rpsfb::mirror_index((long)rc + c, W);
    double sum = s.patch[r * ld + c];
    for (int j = 0; j < len; ++j) {
      const double pr = (double)fr - k.row[j], pc = (double)fc - k.col[j];
      const double q = pr * pr + pc * pc;
      if (!(q <= sub.R2)) continue;
      sum += k.flux[j] * rpsff::model_at(sub.cube + (size_t)k.cell[j] * cell_words, sub.model_n, sub.h, pr, pc);
    }
    s.patch[r * ld + c] = sum;
  }
}
// phase 1n-d: the gather itself, the sum taken out, rounded to float32 once
RPSFB_HD void b1n_gather(int tid, int nthreads, int N, const float* img, int H, int W, int rr, int rc, const rpsfb::Lds& s) {
  const int ld = rpsfb::ld_for(N);
  for (int p = tid; p < N * N; p += nthreads) {
    const int r = p / N, c = p % N;
    const size_t at = (size_t)rpsfb::mirror_index((long)rr + r, H) * W + rpsfb::mirror_index((long)rc + c, W);
    s.patch[r * ld + c] = (double)(float)((double)img[at] - s.patch[r * ld + c]);
  }
}

// ------------------------------------------------------------------------------------------------ the neighbour lists, on the host
// the hull [lo, hi] of mirror_index(first + k, len) over k = 0 .. N - 1
inline void mirrored_hull(long first, int N, int len, int& lo, int& hi) {
  lo = len, hi = -1;
  for (int k = 0; k < N; ++k) {
    const int m = rpsfb::mirror_index(first + k, len);
    lo = m < lo ? m : lo, hi = m > hi ? m : hi;
  }
}

// Star j of the set is on patch k's list when j != own[k] (own[k] = -1: nobody is left in), star_rendered(flux_j, cell_j, n_cells), and S10's
// box of j - floor(y - R) - 1 .. ceil(y + R) + 1 in rows, likewise in columns - clipped to the frame meets the rectangle [min fr, max fr] x
// [min fc, max fc] of the patch's mirrored rows and columns.  Ascending within a list.  (B1n's result needs a superset in ascending order,
// not this exact list: a star whose disc reaches no pixel adds nothing.)  Every drawn star goes into the bucket of its clipped box's first
// corner; a patch looks into the buckets a box that meets its rectangle can start in, so the time is linear in stars plus patches for a
// bounded density of stars.
inline void neighbour_lists(int H, int W, int N, size_t n_patches, const int32_t* corners, const int32_t* own, size_t n_all, const double* pos,
                            const double* flux, const int* cell, int n_cells, double R, std::vector<long long>& offsets,
                            std::vector<int>& index) {
  offsets.assign(n_patches + 1, 0);
  index.clear();
  struct Box {
    int r0, r1, c0, c1;  // r0 > r1: not drawn, or off the frame
  };
  std::vector<Box> boxes(n_all);
  const long by = ((long)H + BUCKET - 1) / BUCKET, bx = ((long)W + BUCKET - 1) / BUCKET;
  std::vector<long long> start((size_t)(by * bx) + 1, 0);
  for (size_t j = 0; j < n_all; ++j) {
    boxes[j] = Box{1, 0, 1, 0};
    if (!rpsfn::star_rendered(flux[j], cell[j], n_cells)) continue;
    const double y = pos[2 * j], x = pos[2 * j + 1];
    const rpsfk::DiscBox box = rpsfk::disc_box(y, x, R);  // (the caller has checked position_ok: the box is far from an int's range)
    long r0 = box.r0, r1 = box.r1, c0 = box.c0, c1 = box.c1;
    if (r0 < 0) r0 = 0;
    if (c0 < 0) c0 = 0;
    if (r1 > H - 1) r1 = H - 1;
    if (c1 > W - 1) c1 = W - 1;
    if (r0 > r1 || c0 > c1) continue;
    boxes[j] = Box{(int)r0, (int)r1, (int)c0, (int)c1};
    ++start[(size_t)((r0 / BUCKET) * bx + c0 / BUCKET) + 1];
  }
  for (size_t b = 0; b < (size_t)(by * bx); ++b) start[b + 1] += start[b];
  std::vector<int> members((size_t)start.back());
  {
    std::vector<long long> next(start.begin(), start.end() - 1);
    for (size_t j = 0; j < n_all; ++j)
      if (boxes[j].r0 <= boxes[j].r1) members[(size_t)next[(size_t)((boxes[j].r0 / BUCKET) * bx + boxes[j].c0 / BUCKET)]++] = (int)j;
  }
  const long reach = (long)std::ceil(2.0 * R) + 4;  // no box is taller or wider: (ceil(y + R) + 1) - (floor(y - R) - 1) <= 2 R + 4
  std::vector<int> found;
  for (size_t k = 0; k < n_patches; ++k) {
    int rlo, rhi, clo, chi;
    mirrored_hull(corners[2 * k], N, H, rlo, rhi);
    mirrored_hull(corners[2 * k + 1], N, W, clo, chi);
    found.clear();
    const long b0 = (rlo - reach < 0 ? 0 : rlo - reach) / BUCKET, b1 = rhi / BUCKET;
    const long d0 = (clo - reach < 0 ? 0 : clo - reach) / BUCKET, d1 = chi / BUCKET;
    for (long b = b0; b <= b1; ++b)
      for (long d = d0; d <= d1; ++d)
        for (long long m = start[(size_t)(b * bx + d)]; m < start[(size_t)(b * bx + d) + 1]; ++m) {
          const int j = members[(size_t)m];
          const Box& box = boxes[j];
          if (j != own[k] && box.r0 <= rhi && box.r1 >= rlo && box.c0 <= chi && box.c1 >= clo) found.push_back(j);
        }
    std::sort(found.begin(), found.end());
    index.insert(index.end(), found.begin(), found.end());
    offsets[k + 1] = (long long)index.size();
  }
}

}  // namespace rpsfbn
