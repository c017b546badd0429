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

// ------------------------------------------------------------------------------------------------ the variance policy of fit_disc
// A usable pixel whose w is not weight_ok is left out like a masked one.  Then, with m and d S8's:  wm = w m, wd = w d, Sm += m, Sw += w,
// Swm += wm, Swmm += wm m, Swd += wd, Swdm += wd m, Swdd += wd d.  THE SOLVE, in this order: with background D = Sw Swmm - Swm Swm,
// f = (Sw Swdm - Swm Swd) / D, bg = (Swd - f Swm) / Sw, var_f = Sw / D, var_bg = Swmm / D, cov = - Swm / D; without it D = Swmm,
// f = Swdm / D, bg = 0, var_f = 1 / D, var_bg = cov = 0.  The flags are S8's.  Pass 2's chi2 = sum w (e e); abs_res and the peak are
// unweighted.
struct VarianceWeights {
  static constexpr int SUMS = W_SUMS, VARIANCES = 3;
  using Weight = double;
  Variance var;
  RPSFS_HD bool weigh(const Frame& fr, size_t p, Weight& w) const { return weight_ok(w = weight_at(var, fr.img, p)); }
  RPSFS_HD static void add(double* s, Weight w, double m, double d) {
    const double wm = w * m, wd = w * d;
    s[W_SM] += m, s[W_SW] += w, s[W_SWM] += wm, s[W_SWMM] += wm * m, s[W_SWD] += wd, s[W_SWDM] += wd * m, s[W_SWDD] += wd * d;
  }
  RPSFS_HD static double chi2_term(Weight w, double e) { return w * (e * e); }
  RPSFS_HD static bool solve(const double* s, int, int background, double& f, double& bg, double* v) {  // v: var_f, var_bg, cov
    const double D = background ? s[W_SW] * s[W_SWMM] - s[W_SWM] * s[W_SWM] : s[W_SWMM];
    if (!finite_d(D) || D <= 0.0) return false;
    if (background) {
      f = (s[W_SW] * s[W_SWDM] - s[W_SWM] * s[W_SWD]) / D;
      bg = (s[W_SWD] - f * s[W_SWM]) / s[W_SW];
      v[0] = s[W_SW] / D, v[1] = s[W_SWMM] / D, v[2] = -s[W_SWM] / D;
    } else {
      f = s[W_SWDM] / D;
      bg = 0.0;
      v[0] = 1.0 / D, v[1] = 0.0, v[2] = 0.0;
    }
    return true;
  }
};
static_assert((int)W_SM == (int)F_SM && (int)W_SM_ALL == (int)F_SM_ALL, "the first two sums are S8's");
static_assert((int)WCOL_VAR_F + VarianceWeights::VARIANCES == (int)WCOL_CHI2, "the variances stand between bg and chi2");

// S8's records with W_SUMS doubles per record, and S8's state behind them
RPSFS_HD constexpr size_t s12_record_bytes() { return FitRecords<VarianceWeights>::bytes(); }
RPSFS_HD constexpr size_t s12_lds_bytes() { return fit_lds_bytes<VarianceWeights>(); }

// S12: fit_disc with the variance policy, rows of FITW_COLUMNS
template <class Ctx>
RPSFS_HD void s12_fit_weighted(Ctx& ctx, const Frame& fr, const double* L, const int* none, int use_mesh, const Model& model, const Fit& fit,
                               const Variance& var, const double* pos, const int* cell, long count, long first, void* lds, double* out) {
  fit_disc(ctx, fr, L, none, use_mesh, model, fit, VarianceWeights{var}, pos, cell, count, first, lds, out);
}

}  // namespace rpsfw
