// CPU lane emulator for rpsf_core_stars.hpp (test infrastructure, never shipped in the product path).
// Runs the drivers and per-thread functions of the star finder's kernels with a context whose each() loops over the threads of a
// workgroup, workgroups and grid threads one after the other, in the launch order of csrc/stars.hip - so the clipping rounds, the
// exact median, the background surface, the filter, the labelling and the moments are checked without a GPU.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_stars.hpp"
#include "emu_ctx.hpp"

using namespace rpsfs;

namespace {
std::vector<uint8_t> mask_or_zeros(const uint8_t* mask, size_t npix) {
  std::vector<uint8_t> m(npix, 0);
  if (mask)
    for (size_t i = 0; i < npix; ++i) m[i] = mask[i] != 0;
  return m;
}
void label(const uint8_t* det, int H, int W, int32_t* labels) {
  const int tiles_y = (H + TILE_R - 1) / TILE_R, tiles_x = (W + TILE_C - 1) / TILE_C;
  std::vector<int> ll(TILE_R * TILE_C);
  CpuCtx ctx{TILE_THREADS};
  for (int ty = 0; ty < tiles_y; ++ty)
    for (int tx = 0; tx < tiles_x; ++tx) {
      for (int& x : ll) x = -7;  // nothing may depend on what the previous tile left
      s3_tile(ctx, det, H, W, ty, tx, ll.data(), labels);
    }
  for (long gid = 0; gid < (long)tiles_y * tiles_x * SEAM_SLOTS; ++gid) s3_seam(gid, H, W, labels);
  for (long gid = 0; gid < (long)H * W; ++gid) s3_flatten(gid, (long)H * W, labels);
}
}  // namespace

extern "C" void emus_info(int* tile_rows, int* tile_cols) { *tile_rows = TILE_R, *tile_cols = TILE_C; }

// S1's LDS carve as the kernel and the launch read it: where the Part records start, what they take, what a workgroup asks for
extern "C" void emus_s1_carve(int box, size_t* offset, size_t* records, size_t* bytes) {
  *offset = s1_part_offset(box), *records = S1_RECORDS * sizeof(Part), *bytes = s1_lds_bytes(box);
}

extern "C" int emus_background(const float* img, const uint8_t* mask, int H, int W, int box, double* level, double* rms) {
  if (H <= 0 || W <= 0 || box < MIN_BOX || box > MAX_BOX) return -1;
  const std::vector<uint8_t> m = mask_or_zeros(mask, (size_t)H * W);
  const Frame fr{img, m.data(), H, W, box, (H + box - 1) / box, (W + box - 1) / box};
  std::vector<double> lds(s1_lds_bytes(box) / sizeof(double) + 1);
  CpuCtx ctx{S1_THREADS};
  for (int bi = 0; bi < fr.nby; ++bi)
    for (int bj = 0; bj < fr.nbx; ++bj) {
      for (double& x : lds) x = std::nan("");
      s1_box(ctx, fr, bi, bj, lds.data(), level, rms);
    }
  return 0;
}

extern "C" int emus_label(const uint8_t* det, int H, int W, int32_t* labels) {
  if (H <= 0 || W <= 0) return -1;
  label(det, H, W, labels);
  return 0;
}

// S2 - S4 as rpsf_stars_detect runs them; rows (row, col, flux, area) into `out` (room for `capacity` rows), the count kept into *count
extern "C" int emus_detect(const float* img, const uint8_t* mask, int H, int W, int box, const double* L, double T, long min_area,
                           long max_area, double* out, long capacity, long* count) {
  if (H <= 0 || W <= 0 || box < MIN_BOX || box > MAX_BOX) return -1;
  const long npix = (long)H * W;
  const std::vector<uint8_t> m = mask_or_zeros(mask, (size_t)npix);
  const Frame fr{img, m.data(), H, W, box, (H + box - 1) / box, (W + box - 1) / box};
  std::vector<uint8_t> det(npix, 9);
  std::vector<int32_t> labels(npix, -7);
  {
    std::vector<double> lds(s2_lds_bytes() / sizeof(double));
    CpuCtx ctx{TILE_THREADS};
    for (int ty = 0; ty < (H + TILE_R - 1) / TILE_R; ++ty)
      for (int tx = 0; tx < (W + TILE_C - 1) / TILE_C; ++tx) {
        for (double& x : lds) x = std::nan("");
        s2_tile(ctx, fr, L, T, ty, tx, lds.data(), det.data());
      }
  }
  label(det.data(), H, W, labels.data());
  const long nseg = (long)H * segs_per_row(W);
  std::vector<int> segcnt(nseg, -1), segoff(nseg, -1), scan_lds(SCAN_THREADS + 32);
  int total = -1;
  for (long seg = 0; seg < nseg; ++seg) s4_count(seg, H, W, labels.data(), segcnt.data());
  CpuCtx scan{SCAN_THREADS};
  s4_scan(scan, nseg, segcnt.data(), segoff.data(), &total, scan_lds.data());
  *count = 0;
  if (total <= 0) return 0;
  std::vector<int> roots(total, -1), stats(4 * (size_t)total, -1);
  std::vector<double> moments(4 * (size_t)total, std::nan(""));
  for (long seg = 0; seg < nseg; ++seg) s4_roots(seg, H, W, labels.data(), segoff.data(), roots.data());
  for (long k = 0; k < total; ++k) s4_init(k, total, W, roots.data(), stats.data());
  for (long gid = 0; gid < npix; ++gid) s4_accumulate(gid, npix, W, labels.data(), roots.data(), total, stats.data());
  std::vector<double> lds(s4_walk_lds_bytes() / sizeof(double));
  CpuCtx walk{WALK_THREADS};
  for (long first = 0; first < total; first += WALK_WAVES)
    s4_walk(walk, fr, L, labels.data(), roots.data(), stats.data(), total, min_area, max_area, first, lds.data(), moments.data());
  for (long k = 0; k < total; ++k) {
    const double flux = moments[4 * k], area = moments[4 * k + 3];
    if (area < (double)min_area || (max_area >= 0 && area > (double)max_area) || !(flux > 0.0)) continue;
    if (*count < capacity) {
      double* row = out + 4 * *count;
      row[0] = moments[4 * k + 1] / flux, row[1] = moments[4 * k + 2] / flux, row[2] = flux, row[3] = area;
    }
    ++*count;
  }
  return 0;
}
