// rpsf_core_stars_fit_weighted.hpp - S8's fit with one weight per pixel, w = 1 / v, and the formal variances of what it fits (DESIGN.md 3.7
// "Weighted fits", S12), shared with the CPU lane emulator tests/emu/emu_fit_weighted.cpp.  A driver over a context as in
// rpsf_core_stars.hpp.
//
//   S12 s12_fit_weighted   one wave per position: S8's box, walk, disc and fold; per usable pixel the variance v from a float32 map or from
//                          the noise model sky_variance + max(pixel, 0) / gain, the weighted sums of the normal equations, the solve for
//                          flux and background and their covariance in the wave's first lane, and a second walk over the same pixels for
//                          the residual: sum w e e, sum |e| and S8's peak
//
// The model, the residual's peak order, the usable pixels of the frame and the background surface are S8's own functions (model_at,
// see_residual, peak_key, usable, background_at, finite_d), called and not copied.  It reads the finder's frame, mask, filtered mesh and
// variance frame, the positions, the cell indices and the cube, and writes its own output rows and nothing else.  No atomics at all, no
// workgroup waits for another, no square root: errors are derived on the host.  Two runs on one input agree bit for bit.
//
// WITH v = 1 EVERYWHERE every term below is S8's term bit for bit - w = 1, w m = m, w d = d, Sw = n exactly - so f, bg, chi2, abs_res and
// the peak are S8's in every bit.  With v = 2^k: w = 2^-k exactly, every weighted sum is S8's times 2^-k, D is S8's times 2^-2k; f, bg,
// abs_res and the peak keep S8's bits, chi2 is 2^-k times S8's, var_f = 2^k (n / D_S8).  (As long as nothing under- or overflows.)
//
// This is NOT a PSF-photometry package's fit: the position is given and not fitted, the interpolation is bilinear and cut at R, and the
// variances are formal - what the given v imply and nothing else; a wrong v gives a wrong error.
#pragma once
#include "rpsf_core_stars_fit.hpp"

#pragma clang fp contract(off)

namespace rpsfw {
using namespace rpsff;

constexpr int FITW_COLUMNS = 25;
enum { VARIANCE_MAP = 0, VARIANCE_MODEL = 1 };
// a row of the output (RPSF_STARS_FIT_WEIGHTED_COLUMNS of include/rpsf.h): S8's four scalars and two counts, then
enum { W_SM, W_SM_ALL, W_SW, W_SWM, W_SWMM, W_SWD, W_SWDM, W_SWDD, W_SUMS };  // sum m (usable), sum m (the disc), sum w, w m, w m m, w d, w d m, w d d
enum { WCOL_SUMS = (int)COL_NALL + 1, WCOL_F = (int)WCOL_SUMS + (int)W_SUMS, WCOL_BG, WCOL_VAR_F, WCOL_VAR_BG, WCOL_COV, WCOL_CHI2, WCOL_ABS_RES,
       WCOL_PEAK_RES, WCOL_PEAK_E, WCOL_PEAK_ROW, WCOL_PEAK_COL };
static_assert((int)WCOL_PEAK_COL + 1 == FITW_COLUMNS, "a row is the four scalars, the two counts, the eight sums, f, bg, their three variances and the six residual columns");
static_assert((int)R_SUMS <= (int)W_SUMS, "pass 2's fields lie in pass 1's words");

struct Variance {
  const float* map;  // VARIANCE_MAP: a frame of the finder's shape (not read otherwise)
  int mode;
  double sky, gain;  // VARIANCE_MODEL: v = sky + max(pixel, 0) / gain
};

// what is wrong with the noise model's parameters (null: nothing)
inline const char* variance_problem(int mode, double sky_variance, double gain) {
  if (mode == VARIANCE_MAP) return nullptr;
  if (mode != VARIANCE_MODEL) return "variance_mode must be RPSF_STARS_VARIANCE_MAP or RPSF_STARS_VARIANCE_MODEL";
  if (!(sky_variance >= 0.0) || !finite_d(sky_variance)) return "sky_variance must be finite and not negative";
  if (!(gain > 0.0)) return "gain must be positive (+inf: no photon term)";
  if (sky_variance == 0.0 && !finite_d(gain)) return "sky_variance = 0 with gain = +inf leaves no variance at all";
  return nullptr;
}

// the weight of the frame's pixel p, in exactly this order of operations; the pixel is S8-usable, so img[p] is finite
RPSFS_HD double weight_at(const Variance& var, const float* img, size_t p) {
  const double v = var.mode == VARIANCE_MAP ? (double)var.map[p] : var.sky + (img[p] > 0 ? (double)img[p] : 0.0) / var.gain;
  return 1.0 / v;
}
// v that is NaN, <= 0, +inf or so small that 1 / v overflows: the pixel is left out like a masked one
RPSFS_HD bool weight_ok(double w) { return w > 0.0 && finite_d(w); }

// ------------------------------------------------------------------------------------------------ the records in LDS
// S8's layout with W_SUMS doubles per record; behind the records what the first lane of each wave hands to its lanes: f, bg, whether
// pass 2 runs.
RPSFS_HD constexpr size_t s12_record_bytes() { return (size_t)W_SUMS * 8 + 8 + 2 * 4; }
RPSFS_HD constexpr size_t s12_lds_bytes() { return (size_t)(WALK_THREADS + WALK_WAVES * 8) * s12_record_bytes() + S8_STATE_BYTES; }

struct WRecords {  // n records at `base` (a multiple of 16 bytes: n is a multiple of 4)
  double* d;
  long long* at;
  int* cnt;
  int n;
  RPSFS_HD WRecords(void* base, int n_) : d(static_cast<double*>(base)), n(n_) {
    at = reinterpret_cast<long long*>(d + (size_t)W_SUMS * n_);
    cnt = reinterpret_cast<int*>(at + n_);
  }
};

// One workgroup, WALK_WAVES positions from `first` on, one wave each: s8_fit's box, walk and disc.  A pixel of the disc counts in n_all and
// Sm_all as S8's; it is usable (n) when it lies on the frame, S8's usable() holds and w = 1 / v has w > 0 and finite.  Then, with m and d
// S8's:  wm = w m, wd = w d, Sm += m, Sw += w, Swm += wm, Swmm += wm m, Swd += wd, Swdm += wd m, Swdd += wd d.  The fold is S8's.
// THE SOLVE, in the wave's first lane, in this order: with background D = Sw Swmm - Swm Swm, f = (Sw Swdm - Swm Swd) / D,
// bg = (Swd - f Swm) / Sw, var_f = Sw / D, var_bg = Swmm / D, cov = - Swm / D; without it D = Swmm, f = Swdm / D, bg = 0, var_f = 1 / D,
// var_bg = cov = 0.  The flags are S8's: TOO_FEW at n < 3 (with background) or n < 1, else DEGENERATE when D is not finite or D <= 0.
// PASS 2 walks the same pixels in the same order with e = d - (f m + bg): chi2 = sum w (e e), abs_res = sum |e| and S8's peak of e, both
// unweighted.
template <class Ctx>
RPSFS_HD void s12_fit_weighted(Ctx& ctx, const Frame& fr, const double* L, const int* none, int use_mesh, const Model& model, const Fit& fit,
                               const Variance& var, const double* pos, const int* cell, long count, long first, void* lds, double* out) {
  const WRecords acc(lds, WALK_THREADS);
  const WRecords acc2(static_cast<char*>(lds) + WALK_THREADS * s12_record_bytes(), WALK_WAVES * 8);
  double* st = reinterpret_cast<double*>(static_cast<char*>(lds) + (WALK_THREADS + WALK_WAVES * 8) * s12_record_bytes());
  int* go = reinterpret_cast<int*>(st + FS_DOUBLES * WALK_WAVES);
  const bool no_mesh = use_mesh && none[0] != 0;
  const bool subtract = use_mesh && !no_mesh;
  const Mesh mesh{L, fr.nbx, 0, 0};
  const int N = model.N;
  const size_t cell_words = (size_t)N * N;
  ctx.each([&](int tid) {  // pass 1
    const long i = first + tid / WALK_LANES;
    const int lane = tid % WALK_LANES;
    double s[W_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int n_use = 0, n_all = 0;
    if (i < count) {
      const double y = pos[2 * i], x = pos[2 * i + 1];
      const int k = cell[i];
      const bool counts_only = no_mesh || k < 0 || k >= model.n_cells;
      const double* C = counts_only ? nullptr : model.cube + (size_t)k * cell_words;
      const int r0 = (int)std::floor(y - fit.R) - 1, r1 = (int)std::ceil(y + fit.R) + 1;
      const int c0 = (int)std::floor(x - fit.R) - 1, c1 = (int)std::ceil(x + fit.R) + 1;
      const long bw = c1 - c0 + 1, npx = (long)(r1 - r0 + 1) * bw;
      for (long j = lane; j < npx; j += WALK_LANES) {
        const int r = r0 + (int)(j / bw), c = c0 + (int)(j % bw);
        const double pr = (double)r - y, pc = (double)c - x;
        const double q = pr * pr + pc * pc;
        if (!(q <= fit.R2)) continue;
        ++n_all;
        double m = 0.0;
        if (!counts_only) m = model_at(C, N, fit.h, pr, pc), s[W_SM_ALL] += m;
        if (r < 0 || r >= fr.H || c < 0 || c >= fr.W) continue;
        const size_t p = (size_t)r * fr.W + c;
        if (!usable(fr.img, fr.mask, p)) continue;
        const double w = weight_at(var, fr.img, p);
        if (!weight_ok(w)) continue;
        ++n_use;
        if (counts_only) continue;
        const double d = subtract ? (double)fr.img[p] - background_at(fr, mesh, r, c) : (double)fr.img[p];
        const double wm = w * m, wd = w * d;
        s[W_SM] += m, s[W_SW] += w, s[W_SWM] += wm, s[W_SWMM] += wm * m, s[W_SWD] += wd, s[W_SWDM] += wd * m, s[W_SWDD] += wd * d;
      }
    }
#pragma unroll
    for (int f = 0; f < W_SUMS; ++f) acc.d[f * WALK_THREADS + tid] = s[f];
    acc.cnt[tid] = n_use, acc.cnt[WALK_THREADS + tid] = n_all;
  });
  ctx.each([&](int tid) {  // 64 partials to 8
    const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
    if (lane >= 8) return;
    const int G = WALK_WAVES * 8, i0 = wave * WALK_LANES + 8 * lane, g = wave * 8 + lane;
    for (int f = 0; f < W_SUMS; ++f) {
      double v = 0.0;
      for (int j = 0; j < 8; ++j) v += acc.d[f * WALK_THREADS + i0 + j];
      acc2.d[f * G + g] = v;
    }
    for (int f = 0; f < 2; ++f) {
      int v = 0;
      for (int j = 0; j < 8; ++j) v += acc.cnt[f * WALK_THREADS + i0 + j];
      acc2.cnt[f * G + g] = v;
    }
  });
  ctx.each([&](int tid) {  // 8 to 1, and the wave's first lane solves
    const int wave = tid / WALK_LANES;
    if (tid % WALK_LANES != 0) return;
    const long i = first + wave;
    go[wave] = 0;
    if (i >= count) return;
    const int G = WALK_WAVES * 8, g0 = wave * 8;
    double s[W_SUMS];
    for (int f = 0; f < W_SUMS; ++f) {
      double v = 0.0;
      for (int j = 0; j < 8; ++j) v += acc2.d[f * G + g0 + j];
      s[f] = v;
    }
    int cnt[2];
    for (int f = 0; f < 2; ++f) {
      int v = 0;
      for (int j = 0; j < 8; ++j) v += acc2.cnt[f * G + g0 + j];
      cnt[f] = v;
    }
    const double nan = std::nan("");
    const int k = cell[i];
    int flags = (no_mesh ? FLAG_NO_MESH : 0) | (k < 0 || k >= model.n_cells ? FLAG_BAD_CELL : 0);
    double f = nan, bg = nan, var_f = nan, var_bg = nan, cov = nan;
    if (flags == 0) {
      if (cnt[0] < (fit.background ? 3 : 1)) {
        flags |= FLAG_TOO_FEW;
      } else if (fit.background) {
        const double D = s[W_SW] * s[W_SWMM] - s[W_SWM] * s[W_SWM];
        if (!finite_d(D) || D <= 0.0) {
          flags |= FLAG_DEGENERATE;
        } else {
          f = (s[W_SW] * s[W_SWDM] - s[W_SWM] * s[W_SWD]) / D;
          bg = (s[W_SWD] - f * s[W_SWM]) / s[W_SW];
          var_f = s[W_SW] / D, var_bg = s[W_SWMM] / D, cov = -s[W_SWM] / D;
        }
      } else {
        const double D = s[W_SWMM];
        if (!finite_d(D) || D <= 0.0) {
          flags |= FLAG_DEGENERATE;
        } else {
          f = s[W_SWDM] / D;
          bg = 0.0;
          var_f = 1.0 / D, var_bg = 0.0, cov = 0.0;
        }
      }
    }
    const bool sums = (flags & (FLAG_NO_MESH | FLAG_BAD_CELL)) == 0;
    double* o = out + (size_t)FITW_COLUMNS * i;
    o[COL_FY] = pos[2 * i], o[COL_FX] = pos[2 * i + 1], o[COL_CELL] = (double)k, o[COL_FFLAGS] = (double)flags;
    o[COL_N] = (double)cnt[0], o[COL_NALL] = (double)cnt[1];
    for (int c = 0; c < W_SUMS; ++c) o[WCOL_SUMS + c] = sums ? s[c] : nan;
    o[WCOL_F] = f, o[WCOL_BG] = bg, o[WCOL_VAR_F] = var_f, o[WCOL_VAR_BG] = var_bg, o[WCOL_COV] = cov;
    if (flags == 0) {
      st[FS_F * WALK_WAVES + wave] = f, st[FS_BG * WALK_WAVES + wave] = bg, go[wave] = 1;
    } else {
      o[WCOL_CHI2] = o[WCOL_ABS_RES] = o[WCOL_PEAK_RES] = o[WCOL_PEAK_E] = nan;
      o[WCOL_PEAK_ROW] = o[WCOL_PEAK_COL] = -1.0;
    }
  });
  ctx.each([&](int tid) {  // pass 2: the same pixels in the same order
    const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
    if (!go[wave]) return;
    const long i = first + wave;
    const double y = pos[2 * i], x = pos[2 * i + 1];
    const double f = st[FS_F * WALK_WAVES + wave], bg = st[FS_BG * WALK_WAVES + wave];
    const double* C = model.cube + (size_t)cell[i] * cell_words;
    const int r0 = (int)std::floor(y - fit.R) - 1, r1 = (int)std::ceil(y + fit.R) + 1;
    const int c0 = (int)std::floor(x - fit.R) - 1, c1 = (int)std::ceil(x + fit.R) + 1;
    const long bw = c1 - c0 + 1, npx = (long)(r1 - r0 + 1) * bw;
    double chi2 = 0.0, abs_res = 0.0;
    Peak seen{0.0, -1};
    for (long j = lane; j < npx; j += WALK_LANES) {
      const int r = r0 + (int)(j / bw), c = c0 + (int)(j % bw);
      const double pr = (double)r - y, pc = (double)c - x;
      const double q = pr * pr + pc * pc;
      if (!(q <= fit.R2)) continue;
      if (r < 0 || r >= fr.H || c < 0 || c >= fr.W) continue;
      const size_t p = (size_t)r * fr.W + c;
      if (!usable(fr.img, fr.mask, p)) continue;
      const double w = weight_at(var, fr.img, p);
      if (!weight_ok(w)) continue;
      const double m = model_at(C, N, fit.h, pr, pc);
      const double d = subtract ? (double)fr.img[p] - background_at(fr, mesh, r, c) : (double)fr.img[p];
      const double e = d - (f * m + bg);
      chi2 += w * (e * e), abs_res += std::fabs(e);
      see_residual(seen, e, (long long)p);
    }
    acc.d[R_CHI2 * WALK_THREADS + tid] = chi2, acc.d[R_ABS * WALK_THREADS + tid] = abs_res;
    acc.d[R_PEAK * WALK_THREADS + tid] = seen.e, acc.at[tid] = seen.at;
  });
  ctx.each([&](int tid) {  // 64 partials to 8
    const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
    if (lane >= 8 || !go[wave]) return;
    const int G = WALK_WAVES * 8, i0 = wave * WALK_LANES + 8 * lane, g = wave * 8 + lane;
    for (int f = 0; f < R_PEAK; ++f) {
      double v = 0.0;
      for (int j = 0; j < 8; ++j) v += acc.d[f * WALK_THREADS + i0 + j];
      acc2.d[f * G + g] = v;
    }
    Peak seen{0.0, -1};
    for (int j = 0; j < 8; ++j) see_residual(seen, acc.d[R_PEAK * WALK_THREADS + i0 + j], acc.at[i0 + j]);
    acc2.d[R_PEAK * G + g] = seen.e, acc2.at[g] = seen.at;
  });
  ctx.each([&](int tid) {  // 8 to 1
    const int wave = tid / WALK_LANES;
    if (tid % WALK_LANES != 0 || !go[wave]) return;
    const int G = WALK_WAVES * 8, g0 = wave * 8;
    double* o = out + (size_t)FITW_COLUMNS * (first + wave);
    for (int f = 0; f < R_PEAK; ++f) {
      double v = 0.0;
      for (int j = 0; j < 8; ++j) v += acc2.d[f * G + g0 + j];
      o[WCOL_CHI2 + f] = v;
    }
    Peak seen{0.0, -1};
    for (int j = 0; j < 8; ++j) see_residual(seen, acc2.d[R_PEAK * G + g0 + j], acc2.at[g0 + j]);
    // (flags == 0 has n >= 1: there is a pixel)
    o[WCOL_PEAK_RES] = std::fabs(seen.e), o[WCOL_PEAK_E] = seen.e;
    o[WCOL_PEAK_ROW] = (double)(seen.at / fr.W), o[WCOL_PEAK_COL] = (double)(seen.at % fr.W);
  });
}

}  // namespace rpsfw
