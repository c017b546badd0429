// CPU lane emulator for rpsf_core_stars_shape.hpp (test infrastructure, never shipped in the product path).
// Runs S2 - S4, with the deblend option D1 - D4, and then S5 in the launch order of csrc/stars.hip (rpsf_stars_detect followed by
// rpsf_stars_measure): each() loops over the threads of a workgroup, workgroups and grid threads run one after the other.  Every array a
// kernel does not write in full starts with garbage.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_stars_shape.hpp"
#include "emu_ctx.hpp"

using namespace rpsfd;

namespace {
void label(const uint8_t* det, int H, int W, int32_t* labels) {
  const int tiles_y = (H + TILE_R - 1) / TILE_R, tiles_x = (W + TILE_C - 1) / TILE_C;
  std::vector<int> ll(TILE_R * TILE_C);
  CpuCtx ctx{TILE_THREADS};
  for (int ty = 0; ty < tiles_y; ++ty)
    for (int tx = 0; tx < tiles_x; ++tx) {
      for (int& x : ll) x = -7;
      s3_tile(ctx, det, H, W, ty, tx, ll.data(), labels);
    }
  for (long gid = 0; gid < (long)tiles_y * tiles_x * SEAM_SLOTS; ++gid) s3_seam(gid, H, W, labels);
  for (long gid = 0; gid < (long)H * W; ++gid) s3_flatten(gid, (long)H * W, labels);
}
// the entries with labels[p] == p in index order (S4's count, scan, roots)
std::vector<int> fixed_points(const int32_t* labels, int H, int W) {
  const long nseg = (long)H * segs_per_row(W);
  std::vector<int> segcnt(nseg, -1), segoff(nseg, -1), scan_lds(SCAN_THREADS + 32);
  int total = -1;
  for (long seg = 0; seg < nseg; ++seg) s4_count(seg, H, W, labels, segcnt.data());
  CpuCtx scan{SCAN_THREADS};
  s4_scan(scan, nseg, segcnt.data(), segoff.data(), &total, scan_lds.data());
  std::vector<int> roots(total > 0 ? total : 0, -1);
  for (long seg = 0; seg < nseg; ++seg) s4_roots(seg, H, W, labels, segoff.data(), roots.data());
  return roots;
}
}  // namespace

// info[3] = WALK_WAVES, the shape columns, the workgroups of S5 the last emush_measure ran
static long launches = 0;
extern "C" void emush_info(long* info) { info[0] = WALK_WAVES, info[1] = rpsfh::SHAPE_COLUMNS, info[2] = launches; }

// rpsf_stars_detect (after rpsf_stars_set_deblend(on, contrast, prominence)), rpsf_stars_positions and rpsf_stars_measure /
// rpsf_stars_shapes: `positions` takes capacity x 4, `shapes` capacity x SHAPE_COLUMNS doubles, *count the number of rows
extern "C" int emush_measure(const float* img, const uint8_t* mask, int H, int W, int box, const double* L, double T, long min_area,
                             long max_area, int on, double contrast, double prominence, double* positions, double* shapes, long capacity,
                             long* count) {
  if (H <= 0 || W <= 0 || box < MIN_BOX || box > MAX_BOX) return -1;
  const long npix = (long)H * W;
  std::vector<uint8_t> m(npix, 0);
  if (mask)
    for (long i = 0; i < npix; ++i) m[i] = mask[i] != 0;
  const Frame fr{img, m.data(), H, W, box, (H + box - 1) / box, (W + box - 1) / box};
  std::vector<uint8_t> det(npix, 9);
  std::vector<int32_t> labels(npix, -7), owner(on ? npix : 0, -7);
  std::vector<double> f(on ? npix : 0, std::nan(""));
  {
    std::vector<double> lds(s2_lds_bytes() / sizeof(double));
    CpuCtx ctx{TILE_THREADS};
    for (int ty = 0; ty < (H + TILE_R - 1) / TILE_R; ++ty)
      for (int tx = 0; tx < (W + TILE_C - 1) / TILE_C; ++tx) {
        for (double& x : lds) x = std::nan("");
        s2_tile(ctx, fr, L, T, ty, tx, lds.data(), det.data(), on ? f.data() : nullptr);
      }
  }
  label(det.data(), H, W, labels.data());
  *count = 0;
  launches = 0;
  const std::vector<int> roots = fixed_points(labels.data(), H, W);
  const long n = (long)roots.size();
  if (n == 0) return 0;
  std::vector<int> stats(4 * (size_t)n, -1), peaks, ostats;
  std::vector<double> moments(4 * (size_t)n, std::nan(""));
  for (long k = 0; k < n; ++k) s4_init(k, n, W, roots.data(), stats.data());
  for (long gid = 0; gid < npix; ++gid) s4_accumulate(gid, npix, W, labels.data(), roots.data(), n, stats.data());
  std::vector<double> lds(s4_walk_lds_bytes() / sizeof(double));
  CpuCtx walk{WALK_THREADS};
  for (long first = 0; first < n; first += WALK_WAVES)
    s4_walk(walk, fr, L, labels.data(), roots.data(), stats.data(), n, min_area, on ? -1 : max_area, first, lds.data(), moments.data());
  std::vector<double> rows;
  std::vector<rpsfh::Source> sources;
  if (!on) {
    for (long k = 0; k < n; ++k) {
      const double flux = moments[4 * k], area = moments[4 * k + 3];
      if (area < (double)min_area || (max_area >= 0 && area > (double)max_area) || !(flux > 0.0)) continue;
      rows.insert(rows.end(), {moments[4 * k + 1] / flux, moments[4 * k + 2] / flux, flux, area});
      sources.emplace_back(k, -1);
    }
  } else {
    std::vector<int32_t> up(npix, -7), peak(npix, -7);
    for (long gid = 0; gid < npix; ++gid) d1_up(gid, H, W, f.data(), det.data(), up.data());
    for (long gid = 0; gid < npix; ++gid) d1_peak(gid, npix, up.data(), peak.data());
    peaks = fixed_points(peak.data(), H, W);
    const long nb = (long)peaks.size();
    if (nb < 1) return -2;
    std::vector<int> bstats(BOX * (size_t)nb, -7), bcomp(nb, -7), nsig(n, 0);
    ostats.assign(BOX * (size_t)nb, -7);
    std::vector<uint64_t> saddle(nb, 77);
    std::vector<uint8_t> sig(nb, 9), want(nb, 9);
    std::vector<double> bflux(4 * (size_t)nb, std::nan("")), omoments(4 * (size_t)nb, std::nan(""));
    for (long b = 0; b < nb; ++b) d2_init(b, nb, W, peaks.data(), bstats.data(), saddle.data());
    for (long gid = 0; gid < npix; ++gid) d2_accumulate(gid, H, W, f.data(), peak.data(), peaks.data(), nb, bstats.data(), saddle.data());
    for (long b = 0; b < nb; ++b) d2_want(b, nb, saddle.data(), want.data());
    for (long first = 0; first < nb; first += WALK_WAVES)
      d_walk(walk, fr, L, labels.data(), Objects{peak.data(), peaks.data(), bstats.data(), want.data(), nb}, first, lds.data(), bflux.data());
    const Significance test{min_area, contrast, prominence, T};
    for (long b = 0; b < nb; ++b)
      d3_significant(b, nb, W, f.data(), labels.data(), roots.data(), n, moments.data(), peaks.data(), bstats.data(), saddle.data(),
                     bflux.data(), test, bcomp.data(), sig.data(), nsig.data(), ostats.data());
    std::vector<long long> own_lds(d4_own_lds_bytes() / sizeof(long long) + 1);
    CpuCtx own{OWN_THREADS};
    for (long k = 0; k < n; ++k) {
      for (long long& x : own_lds) x = 0x5555555555555555ll;
      d4_own(own, W, labels.data(), roots.data(), stats.data(), k, peak.data(), peaks.data(), nb, bcomp.data(), sig.data(), nsig.data(),
             own_lds.data(), owner.data(), ostats.data());
    }
    for (long b = 0; b < nb; ++b) d4_want(b, nb, bcomp.data(), sig.data(), nsig.data(), ostats.data(), min_area, max_area, want.data());
    for (long first = 0; first < nb; first += WALK_WAVES)
      d_walk(walk, fr, L, labels.data(), Objects{owner.data(), peaks.data(), ostats.data(), want.data(), nb}, first, lds.data(),
             omoments.data());
    size_t split = 0;
    rows = deblend_rows(n, roots.data(), moments.data(), nsig.data(), nb, bcomp.data(), sig.data(), ostats.data(), omoments.data(), min_area,
                        max_area, &split, &sources);
  }
  const long kept = (long)rows.size() / 4;
  *count = kept;
  if (kept == 0 || kept > capacity) return 0;
  for (long i = 0; i < 4 * kept; ++i) positions[i] = rows[i];
  // S5
  const std::vector<rpsfh::ShapeRow> described = rpsfh::describe(rows, sources, W, roots.data(), stats.data(), peaks.data(), ostats.data());
  for (const rpsfh::ShapeRow& row : described)
    if (row.r0 < 0 || row.r1 < row.r0 || row.r1 >= H || row.c0 < 0 || row.c1 < row.c0 || row.c1 >= W) return -3;
  std::vector<rpsfh::Seen> seen(rpsfh::s5_walk_lds_bytes() / sizeof(rpsfh::Seen));
  for (long i = 0; i < rpsfh::SHAPE_COLUMNS * kept; ++i) shapes[i] = std::nan("");
  for (long first = 0; first < kept; first += WALK_WAVES) {
    for (rpsfh::Seen& x : seen) x = rpsfh::Seen{std::nan(""), std::nan(""), std::nan(""), std::nan(""), std::nan(""), 77};
    rpsfh::s5_walk(walk, fr, L, labels.data(), on ? owner.data() : nullptr, described.data(), kept, first, seen.data(), shapes);
    ++launches;
  }
  return 0;
}
