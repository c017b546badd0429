// CPU lane emulator for rpsf_core_saturation.hpp (test infrastructure, never shipped in the product path).
// Runs the per-thread functions and the drivers of kernels F1 - F5 with a context whose each() loops over the threads of a workgroup,
// workgroups and grid threads one after the other, in the launch order of csrc/saturation.hip - so the pad map, the dilation, the
// grouping and the ordered fill are checked without a GPU.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_saturation.hpp"
#include "emu_ctx.hpp"

using namespace rpsfs;
using namespace rpsfsat;

namespace {

struct Filled {
  Padded f;
  std::vector<float> padded;
  std::vector<uint8_t> bytes[3];
  const uint8_t* mask = nullptr;  // null: nothing hot
  int n_hot = 0, n_mask = 0, n_groups = 0;
};

void fill(const float* image, int H, int W, int N, int pad_mode, double threshold, int dilation, int width, int reverse, Filled& s) {
  s.f = Padded{H, W, N, H + 4 * N, W + 4 * N, pad_mode};
  const Padded& f = s.f;
  const long npix = f.npix(), quads = (npix + 3) / 4;
  const int PH = f.PH, PW = f.PW, h = width / 2;
  s.padded.assign(npix, -7.f);
  for (auto& b : s.bytes) b.assign(npix, 9);
  for (long gid = 0; gid < quads; ++gid) f1_pad(gid, f, image, threshold, s.padded.data(), s.bytes[0].data(), &s.n_hot);
  if (s.n_hot == 0) return;
  int at = 0;
  for (int pass = 0; pass < dilation; ++pass, at ^= 1)
    for (long gid = 0; gid < quads; ++gid)
      f2_cross(gid, PH, PW, s.bytes[at].data(), s.bytes[at ^ 1].data(), pass == dilation - 1 ? &s.n_mask : nullptr);
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
    f4_group(wave, reverse ? n - 1 - b : b, PH, PW, h, mask, roots.data(), stats.data(), s.padded.data(), labels.data(), fills.data(), &cursor,
             &lds);
  }
  s.mask = mask;
}
}  // namespace

// F1 - F4: the filled padded frame and the mask ((H + 4N) x (W + 4N) each)
extern "C" int emusat_fill(const float* image, int H, int W, int N, int pad_mode, double threshold, int dilation, int width, int reverse,
                           float* padded, uint8_t* mask, int* n_groups) {
  if (H <= 0 || W <= 0 || N <= 0 || dilation < 1 || width / 2 < 1) return -1;
  Filled s;
  fill(image, H, W, N, pad_mode, threshold, dilation, width, reverse, s);
  const size_t np = (size_t)s.f.npix();
  std::memcpy(padded, s.padded.data(), np * sizeof(float));
  if (s.mask) std::memcpy(mask, s.mask, np);
  else std::memset(mask, 0, np);
  *n_groups = s.n_groups;
  return 0;
}

// F5 behind F1 - F4 with `corrected` standing in for the correction of the filled frame (rows out_row0 ... of the padded frame):
// out (H x W), the list of masked in-frame pixels (room for H * W) and its length
extern "C" int emusat_restore(const float* image, int H, int W, int N, int pad_mode, double threshold, int dilation, int width,
                              const float* corrected, int out_row0, float* out, int32_t* list, int* n_list) {
  if (H <= 0 || W <= 0 || N <= 0 || dilation < 1 || width / 2 < 1) return -1;
  Filled s;
  fill(image, H, W, N, pad_mode, threshold, dilation, width, 0, s);
  *n_list = 0;
  for (long gid = 0; gid < (long)H * W; ++gid) f5_restore(gid, s.f, image, s.mask, corrected, out_row0, out, list, n_list);
  return 0;
}
