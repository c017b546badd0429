// rpsf_core_stars_photometry.hpp - forced aperture photometry at positions the caller supplies (DESIGN.md 3.7 "Apertures", S6), shared
// with the CPU lane emulator tests/emu/emu_photometry.cpp.  A driver over a context as in rpsf_core_stars.hpp.
//
//   S6  s6_apertures   one wave per position: circular apertures at up to MAX_RADII radii with sub-pixel coverage counted on an s x s
//                      lattice per pixel; per radius the flux and the two coverage counts, on the outermost radius sum w |d|, the raw
//                      first and second moments around the position, the peak and its first pixel
//
// It reads the finder's frame, mask and filtered mesh and the positions, and writes its own output rows and nothing else: nothing S1 - S5
// or D1 - D4 read or wrote changes.  No atomics at all, no workgroup waits for another.  Two runs on one input agree bit for bit.
// This is NOT sep's sum_circle: a sub-sample counts when q <= R R, and masked pixels are left out and reported, not corrected for.
#pragma once
#include "rpsf_core_stars_disc.hpp"

#pragma clang fp contract(off)

namespace rpsfp {
using namespace rpsfk;

constexpr int MAX_RADII = 8, MAX_SUBPIX = 8;
constexpr double MAX_RADIUS = 64.0, MAX_COORD = 1048576.0;  // |y|, |x| < 2^20: every pixel index of a box is an int far from overflow
enum { SUM_ABS, SUM_MR, SUM_MC, SUM_MRR, SUM_MCC, SUM_MRC, SUMS };
// a row of the output (RPSF_STARS_PHOTOMETRY_COLUMNS(m) of include/rpsf.h): row, col, flux[m], N_use[m], N_all[m], the six sums, peak,
// peak_row, peak_col
RPSFS_HD constexpr int photometry_columns(int m) { return 2 + 3 * m + SUMS + 3; }

struct Apertures {
  int m, s;
  double rmax;           // R_{m-1}
  double r2[MAX_RADII];  // R_k R_k; -1 from m on, which no q reaches
};

// what is wrong with the radii or subpix (null: nothing)
inline const char* apertures_problem(int m, const double* radii, int subpix) {
  if (m < 1 || m > MAX_RADII) return "the number of radii must lie in 1 ... 8";
  if (subpix < 1 || subpix > MAX_SUBPIX) return "subpix must lie in 1 ... 8";
  if (!radii) return "null argument";
  for (int k = 0; k < m; ++k) {
    if (!(radii[k] > 0.0) || !(radii[k] <= MAX_RADIUS)) return "the radii must lie in 0 < R <= 64";
    if (k > 0 && !(radii[k] > radii[k - 1])) return "the radii must ascend strictly";
  }
  return nullptr;
}
inline bool position_ok(double y, double x) { return std::fabs(y) < MAX_COORD && std::fabs(x) < MAX_COORD; }  // (false for NaN and inf)

inline Apertures make_apertures(int m, const double* radii, int subpix) {
  Apertures ap{};
  ap.m = m, ap.s = subpix, ap.rmax = radii[m - 1];
  for (int k = 0; k < MAX_RADII; ++k) ap.r2[k] = k < m ? radii[k] * radii[k] : -1.0;
  return ap;
}

// ------------------------------------------------------------------------------------------------ the records in LDS
// One record per lane and one per group of 8 lanes, field-major (field f of record i of n is word f n + i: neighbouring lanes touch
// neighbouring words): m + SUMS + 1 doubles (the fluxes, the six sums, the peak), the peak's linear index (64 bits, < 0: no pixel yet),
// then 2 m ints (N_use, N_all).  In front of them two tables every lane reads alike: w[n] = n / (s s) for n = 0 ... 64 and the sub-sample
// offsets o_a = (2a + 1 - s) / (2s).
constexpr int WEIGHTS = MAX_SUBPIX * MAX_SUBPIX + 1;
constexpr size_t WEIGHT_BYTES = ((size_t)(WEIGHTS + MAX_SUBPIX) * sizeof(double) + 15) & ~(size_t)15;
RPSFS_HD constexpr size_t s6_record_bytes(int m) { return (size_t)(m + SUMS + 2) * 8 + (size_t)(2 * m) * 4; }
RPSFS_HD constexpr size_t s6_lds_bytes(int m) { return WEIGHT_BYTES + (size_t)(WALK_THREADS + WALK_WAVES * 8) * s6_record_bytes(m); }

struct Records {  // n records for m radii at `base` (a multiple of 16 bytes: n is a multiple of 4)
  double* d;
  long long* at;
  int* cnt;
  int n;
  RPSFS_HD Records(void* base, int n_, int m) : d(static_cast<double*>(base)), n(n_) {
    at = reinterpret_cast<long long*>(d + (size_t)(m + SUMS + 1) * n);
    cnt = reinterpret_cast<int*>(at + n);
  }
};

// records i0 ... i0 + 7 of `src` in index order into record i of `dst`: the sums added, the peak folded with see_peak's order
RPSFS_HD void s6_fold8(const Records& src, int i0, const Records& dst, int i, int m) {
  for (int f = 0; f < m + SUMS; ++f) dst.d[f * dst.n + i] = sum8(src.d + f * src.n + i0);
  rpsfh::Seen seen = rpsfh::nothing_seen();
  for (int j = 0; j < 8; ++j) rpsfh::see_peak(seen, src.d[(m + SUMS) * src.n + i0 + j], src.at[i0 + j]);
  dst.d[(m + SUMS) * dst.n + i] = seen.peak, dst.at[i] = seen.at;
  for (int f = 0; f < 2 * m; ++f) dst.cnt[f * dst.n + i] = sum8(src.cnt + f * src.n + i0);
}

// One workgroup, WALK_WAVES positions from `first` on, one wave each.  pos[2 i ..] = (y, x).  The box is disc_box(y, x, R_max)
// (rpsf_core_stars_disc.hpp); lane j takes its pixels j, j + 64, ... in raster order - every pixel of the box, not walk_disc's disc.  For pixel
// (r, c): pr = r - y, pc = c - x, q_ab = (pr + o_a)(pr + o_a) + (pc + o_b)(pc + o_b), n_k = #{q_ab <= R_k R_k}, w_k = n_k / (s s).
// N_all_k sums n_k over the box, N_use_k over the usable pixels of the frame; with d the residual against the mesh (use_mesh) or the
// pixel itself, flux_k = sum w_k d, and with w = w_{m-1}, t = w d: sum w |d|, t pr, t pc, t (pr pr), t (pc pc), t (pr pc), the products
// grouped as written; the peak is the largest d where n_{m-1} > 0.  The 64 partial records fold as 8 groups of 8, each in lane order.
// A pixel with n_{m-1} = 0 has every n_k = 0 (the radii ascend) and adds zeros only: it is skipped.  With use_mesh and none[0] set (no
// valid mesh node) every flux, sum and the peak are NaN and the counts are delivered; `L` is not read then.  A position without a usable
// pixel under its outermost aperture has peak NaN at (-1, -1).
template <class Ctx>
RPSFS_HD void s6_apertures(Ctx& ctx, const Frame& fr, const double* L, const int* none, int use_mesh, const Apertures& ap,
                           const double* pos, long count, long first, void* lds, double* out) {
  const int m = ap.m, s = ap.s;
  double* weight = static_cast<double*>(lds);
  const double* o = weight + WEIGHTS;
  const Records acc(static_cast<char*>(lds) + WEIGHT_BYTES, WALK_THREADS, m);
  const Records acc2(static_cast<char*>(lds) + WEIGHT_BYTES + WALK_THREADS * s6_record_bytes(m), WALK_WAVES * 8, m);
  const bool no_mesh = use_mesh && none[0] != 0;
  const bool subtract = use_mesh && !no_mesh;
  const Mesh mesh{L, fr.nbx, 0, 0};
  const int columns = photometry_columns(m);
  ctx.each([&](int tid) {
    if (tid <= s * s) weight[tid] = (double)tid / (double)(s * s);
    if (tid < s) weight[WEIGHTS + tid] = (double)(2 * tid + 1 - s) / (double)(2 * s);
    for (int f = 0; f < m + SUMS + 1; ++f) acc.d[f * WALK_THREADS + tid] = 0.0;
    acc.at[tid] = -1;
    for (int f = 0; f < 2 * m; ++f) acc.cnt[f * WALK_THREADS + tid] = 0;
  });
  ctx.each([&](int tid) {
    const long i = first + tid / WALK_LANES;
    const int lane = tid % WALK_LANES;
    if (i >= count) return;
    const double y = pos[2 * i], x = pos[2 * i + 1];
    const DiscBox box = disc_box(y, x, ap.rmax);
    double* sum = acc.d + tid;
    int* cnt = acc.cnt + tid;
    rpsfh::Seen seen = rpsfh::nothing_seen();
    for (long j = lane; j < box.npx; j += WALK_LANES) {
      const int r = box.r0 + (int)(j / box.bw), c = box.c0 + (int)(j % box.bw);
      const double pr = (double)r - y, pc = (double)c - x;
      int n[MAX_RADII] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int a = 0; a < s; ++a) {
        const double qr = (pr + o[a]) * (pr + o[a]);
        for (int b = 0; b < s; ++b) {
          const double q = qr + (pc + o[b]) * (pc + o[b]);
#pragma unroll
          for (int k = 0; k < MAX_RADII; ++k) n[k] += q <= ap.r2[k];
        }
      }
      int outer = 0;
#pragma unroll
      for (int k = 0; k < MAX_RADII; ++k)
        if (k == m - 1) outer = n[k];
      if (outer == 0) continue;
#pragma unroll
      for (int k = 0; k < MAX_RADII; ++k)
        if (k < m) cnt[(m + k) * WALK_THREADS] += n[k];
      if (r < 0 || r >= fr.H || c < 0 || c >= fr.W) continue;
      const size_t p = (size_t)r * fr.W + c;
      if (!usable(fr.img, fr.mask, p)) continue;
      const double d = subtract ? (double)fr.img[p] - background_at(fr, mesh, r, c) : (double)fr.img[p];
#pragma unroll
      for (int k = 0; k < MAX_RADII; ++k)
        if (k < m) cnt[k * WALK_THREADS] += n[k], sum[k * WALK_THREADS] += weight[n[k]] * d;
      const double w = weight[outer], t = w * d;
      double* six = sum + m * WALK_THREADS;
      six[SUM_ABS * WALK_THREADS] += w * std::fabs(d);
      six[SUM_MR * WALK_THREADS] += t * pr, six[SUM_MC * WALK_THREADS] += t * pc;
      six[SUM_MRR * WALK_THREADS] += t * (pr * pr), six[SUM_MCC * WALK_THREADS] += t * (pc * pc), six[SUM_MRC * WALK_THREADS] += t * (pr * pc);
      rpsfh::see_peak(seen, d, (long long)p);
    }
    sum[(m + SUMS) * WALK_THREADS] = seen.peak, acc.at[tid] = seen.at;
  });
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
    if (lane < 8) s6_fold8(acc, wave * WALK_LANES + 8 * lane, acc2, wave * 8 + lane, m);
  });
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES;
    const long i = first + wave;
    if (tid % WALK_LANES != 0 || i >= count) return;
    const int G = WALK_GROUPS, g0 = wave * 8;
    const double nan = std::nan("");
    double* o = out + (size_t)columns * i;
    o[0] = pos[2 * i], o[1] = pos[2 * i + 1];
    for (int f = 0; f < m + SUMS; ++f) {  // the fluxes, then the six sums: the output's order but for the counts in between
      const double v = sum8(acc2.d + f * G + g0);
      o[2 + (f < m ? f : f + 2 * m)] = no_mesh ? nan : v;
    }
    for (int f = 0; f < 2 * m; ++f) o[2 + m + f] = (double)sum8(acc2.cnt + f * G + g0);
    rpsfh::Seen seen = rpsfh::nothing_seen();
    for (int j = 0; j < 8; ++j) rpsfh::see_peak(seen, acc2.d[(m + SUMS) * G + g0 + j], acc2.at[g0 + j]);
    double* peak = o + 2 + 3 * m + SUMS;
    const bool found = seen.at >= 0 && !no_mesh;
    peak[0] = found ? seen.peak : nan;
    peak[1] = found ? (double)(seen.at / fr.W) : -1.0, peak[2] = found ? (double)(seen.at % fr.W) : -1.0;
  });
}

}  // namespace rpsfp
