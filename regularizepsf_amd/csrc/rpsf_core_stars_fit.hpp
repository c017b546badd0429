// rpsf_core_stars_fit.hpp - linear least-squares fits of a PSF model cell to stars at positions the caller supplies (DESIGN.md 3.7 "Model
// fits", S8), shared with the CPU lane emulator tests/emu/emu_fit.cpp.  A driver over a context as in rpsf_core_stars.hpp.
//
//   S8  s8_fit   one wave per position: the cell of the model cube bilinearly interpolated onto the pixels of a disc around the position,
//                the six sums of the normal equations, the solve for flux and background in the wave's first lane, and a second walk
//                over the same pixels for the residual: sum e e, sum |e| and the largest |e| with its sign and first pixel
//
// It reads the finder's frame, mask and filtered mesh, the positions, the cell indices and the cube, and writes its own output rows and
// nothing else: nothing S1 - S7 or D1 - D4 read or wrote changes.  No atomics at all, no workgroup waits for another.  Two runs on one input
// agree bit for bit.  This is NOT a PSF-photometry package's fit: the weights are uniform (no error column, no variance weighting), the
// position is given and not fitted, the interpolation is bilinear and does not conserve flux below the pixel scale, and masked pixels are
// left out and reported through the counts, not corrected for.
#pragma once
#include "rpsf_core_stars_refine.hpp"

#pragma clang fp contract(off)

namespace rpsff {
using namespace rpsfr;

constexpr int FIT_COLUMNS = 20, MIN_MODEL = 4, MAX_MODEL = 256;
enum { FLAG_NO_MESH = 1, FLAG_TOO_FEW = 2, FLAG_DEGENERATE = 4, FLAG_BAD_CELL = 8 };
// a row of the output (RPSF_STARS_FIT_COLUMNS of include/rpsf.h)
enum { COL_FY, COL_FX, COL_CELL, COL_FFLAGS, COL_N, COL_NALL, COL_FSUMS };
enum { F_SM, F_SM_ALL, F_SMM, F_SD, F_SDM, F_SDD, F_SUMS };  // sum m (usable), sum m (the whole disc), sum m m, sum d, sum d m, sum d d
enum { COL_F = (int)COL_FSUMS + (int)F_SUMS, COL_BG, COL_CHI2, COL_ABS_RES, COL_PEAK_RES, COL_PEAK_E, COL_PEAK_ROW, COL_PEAK_COL };
static_assert((int)COL_PEAK_COL + 1 == FIT_COLUMNS, "a row is the four scalars, the two counts, the six sums, f, bg and the six residual columns");
enum { R_CHI2, R_ABS, R_PEAK, R_SUMS };  // pass 2's fields, in pass 1's words: sum e e, sum |e|, the signed e of the peak
enum { RES_CHI2, RES_ABS, RES_PEAK, RES_PEAK_E, RES_PEAK_ROW, RES_PEAK_COL };  // the six residual columns that end a row, from its chi2 on
static_assert((int)COL_CHI2 + RES_PEAK_COL == (int)COL_PEAK_COL && (int)R_CHI2 == RES_CHI2 && (int)R_ABS == RES_ABS, "pass 2's sums are its first columns");

struct Model {
  const double* cube;  // n_cells x N x N
  int n_cells, N;
};
struct Fit {
  double R, R2, h;  // the fit radius, R R, and the star's centre in the cell: N / 2.0 - 0.5
  int background;   // 1: flux and a constant are fitted; 0: the flux alone
};

// the largest fit radius of an N x N cell: every pixel of the disc has its four model samples inside the cell
inline double max_fit_radius(int N) { return N / 2.0 - 1.0 < MAX_RADIUS ? N / 2.0 - 1.0 : MAX_RADIUS; }
inline bool model_size_ok(int N) { return N >= MIN_MODEL && N <= MAX_MODEL; }
// what is wrong with the radius or fit_background, as far as it can be said without the model (null: nothing)
inline const char* fit_problem(double radius, int fit_background) {
  if (!(radius > 0.0) || !(radius <= MAX_RADIUS)) return "radius must lie in 0 < R <= min(64, N / 2 - 1)";
  if (fit_background != 0 && fit_background != 1) return "fit_background must be 0 or 1";
  return nullptr;
}
inline Fit make_fit(double radius, int fit_background, int N) { return Fit{radius, radius * radius, N / 2.0 - 0.5, fit_background}; }

// The model at pixel offset (pr, pc) = (r - y, c - x) from the star, in exactly this order of operations: the star's centre
// sits at index h of the cell on both axes.  |pr|, |pc| <= R <= N / 2 - 1 keeps 0 <= i and i + 1 <= N - 1.
RPSFS_HD double model_at(const double* C, int N, double h, double pr, double pc) {
  const double u = pr + h, v = pc + h;
  const double fu = std::floor(u), fv = std::floor(v);
  const int i = (int)fu, j = (int)fv;
  const double a = u - fu, b = v - fv;
  const double* p = C + (size_t)i * N + j;
  return ((1.0 - a) * ((1.0 - b) * p[0] + b * p[1])) + (a * ((1.0 - b) * p[N] + b * p[N + 1]));
}

// ------------------------------------------------------------------------------------------------ the weights of a fit
// s8_fit and s12_fit_weighted (rpsf_core_stars_fit_weighted.hpp) are ONE driver, fit_disc, over a weight policy chosen at compile time.
// A policy says how many sums a lane keeps (SUMS; the first two are Sm over the usable pixels and Sm_all over the whole disc), how many
// variances the solve adds to a row (VARIANCES), what a usable pixel weighs and whether that leaves it out (weigh), what it adds to the
// sums (add) and to chi2 (chi2_term), and THE SOLVE (false: DEGENERATE).  The uniform policy is S8: it carries no weight at all.
struct UniformWeights {
  static constexpr int SUMS = F_SUMS, VARIANCES = 0;
  struct Weight {};
  RPSFS_HD bool weigh(const Frame&, size_t, Weight&) const { return true; }
  RPSFS_HD static void add(double* s, Weight, double m, double d) { s[F_SM] += m, s[F_SMM] += m * m, s[F_SD] += d, s[F_SDM] += d * m, s[F_SDD] += d * d; }
  RPSFS_HD static double chi2_term(Weight, double e) { return e * e; }
  // with background D = n Smm - Sm Sm, f = (n Sdm - Sm Sd) / D, bg = (Sd - f Sm) / n; without it D = Smm, f = Sdm / Smm, bg = 0
  RPSFS_HD static bool solve(const double* s, int n_use, int background, double& f, double& bg, double*) {
    const double n = (double)n_use;
    const double D = background ? n * s[F_SMM] - s[F_SM] * s[F_SM] : s[F_SMM];
    if (!finite_d(D) || D <= 0.0) return false;
    if (background) {
      f = (n * s[F_SDM] - s[F_SM] * s[F_SD]) / D;
      bg = (s[F_SD] - f * s[F_SM]) / n;
    } else {
      f = s[F_SDM] / D;
      bg = 0.0;
    }
    return true;
  }
};

// ------------------------------------------------------------------------------------------------ the records in LDS
// LaneRecords (rpsf_core_stars_disc.hpp) of the policy's sums, the peak's linear index, then n and n_all.  Pass 2 puts its R_SUMS doubles
// into the first words of pass 1's.  Behind them what the first lane of each wave hands to its lanes after the solve: f, bg and whether
// pass 2 runs.
enum { FS_F, FS_BG, FS_DOUBLES };
template <class W>
using FitRecords = LaneRecords<W::SUMS, true, 2>;
constexpr size_t S8_STATE_BYTES = ((size_t)WALK_WAVES * (FS_DOUBLES * 8 + 4) + 15) & ~(size_t)15;
template <class W>
RPSFS_HD constexpr size_t fit_lds_bytes() {
  return walk_records_bytes<FitRecords<W>>() + S8_STATE_BYTES;
}
RPSFS_HD constexpr size_t s8_record_bytes() { return FitRecords<UniformWeights>::bytes(); }
RPSFS_HD constexpr size_t s8_lds_bytes() { return fit_lds_bytes<UniformWeights>(); }
static_assert((int)R_SUMS <= (int)F_SUMS, "pass 2's fields lie in pass 1's words");

// One workgroup, WALK_WAVES positions from `first` on, one wave each.  pos[2 i ..] = (y, x), cell[i] its cell of the cube.  The walk is
// walk_disc's over disc_box(y, x, R).  A pixel of the disc counts in n_all, and m = model_at into Sm_all; when it lies on the frame, is
// usable and the policy's weigh() keeps it (n), with d the residual against the mesh (use_mesh) or the pixel itself, the policy adds to
// its sums - S8's: Sm += m, Smm += m m, Sd += d, Sdm += d m, Sdd += d d.  The fold is the disc header's.  TOO_FEW: n < 3 (with
// background) or n < 1; else the policy's SOLVE in the wave's first lane, DEGENERATE: D not finite or D <= 0; either way f, bg, the
// variances and pass 2's columns are NaN (the peak at (-1, -1)).  PASS 2 walks the same pixels in the same order with
// e = d - (f m + bg): chi2 = sum of the policy's chi2_term (S8's: e e), abs_res = sum |e|, and the peak by see_residual's order.
// With use_mesh and none[0] set (NO_MESH) or a cell outside 0 .. n_cells - 1 (BAD_CELL) only the counts are taken - neither `L` nor the
// cube is read - and every sum, f, bg and pass 2's columns are NaN.
// A row: S8's four scalars and two counts, the policy's sums, f, bg, its variances, then the six residual columns.
template <class W, class Ctx>
RPSFS_HD void fit_disc(Ctx& ctx, const Frame& fr, const double* L, const int* none, int use_mesh, const Model& model, const Fit& fit,
                       const W& weights, const double* pos, const int* cell, long count, long first, void* lds, double* out) {
  constexpr int C_F = (int)COL_FSUMS + W::SUMS, C_VAR = C_F + 2, C_RES = C_VAR + W::VARIANCES, COLUMNS = C_RES + 6;
  const FitRecords<W> acc(lds, WALK_THREADS);
  const FitRecords<W> acc2(static_cast<char*>(lds) + WALK_THREADS * FitRecords<W>::bytes(), WALK_GROUPS);
  double* st = reinterpret_cast<double*>(static_cast<char*>(lds) + walk_records_bytes<FitRecords<W>>());
  int* go = reinterpret_cast<int*>(st + FS_DOUBLES * WALK_WAVES);
  const bool no_mesh = use_mesh && none[0] != 0;
  const bool subtract = use_mesh && !no_mesh;
  const Mesh mesh{L, fr.nbx, 0, 0};
  const int N = model.N;
  const size_t cell_words = (size_t)N * N;
  ctx.each([&](int tid) {  // pass 1
    const long i = first + tid / WALK_LANES;
    const int lane = tid % WALK_LANES;
    double s[W::SUMS] = {};
    int n_use = 0, n_all = 0;
    if (i < count) {
      const double y = pos[2 * i], x = pos[2 * i + 1];
      const int k = cell[i];
      const bool counts_only = no_mesh || k < 0 || k >= model.n_cells;
      const double* C = counts_only ? nullptr : model.cube + (size_t)k * cell_words;
      double m = 0.0;
      walk_disc(
          fr, disc_box(y, x, fit.R), y, x, fit.R2, lane,
          [&](double pr, double pc) {
            ++n_all;
            m = 0.0;
            if (!counts_only) m = model_at(C, N, fit.h, pr, pc), s[F_SM_ALL] += m;
          },
          [&](int r, int c, size_t p, double, double, double) {
            typename W::Weight w;
            if (!weights.weigh(fr, p, w)) return;
            ++n_use;
            if (counts_only) return;
            const double d = subtract ? (double)fr.img[p] - background_at(fr, mesh, r, c) : (double)fr.img[p];
            W::add(s, w, m, d);
          });
    }
#pragma unroll
    for (int f = 0; f < W::SUMS; ++f) acc.d[f * WALK_THREADS + tid] = s[f];
    acc.cnt[tid] = n_use, acc.cnt[WALK_THREADS + tid] = n_all;
  });
  ctx.each([&](int tid) {  // 64 partials to 8
    if (tid % WALK_LANES >= 8) return;
    fold_sums_64to8(acc, acc2, tid, W::SUMS), fold_counts_64to8(acc, acc2, tid, 2);
  });
  ctx.each([&](int tid) {  // 8 to 1, and the wave's first lane solves
    const int wave = tid / WALK_LANES;
    if (tid % WALK_LANES != 0) return;
    const long i = first + wave;
    go[wave] = 0;
    if (i >= count) return;
    double s[W::SUMS];
    int cnt[2];
    fold_sums_8to1(acc2, wave, W::SUMS, s), fold_counts_8to1(acc2, wave, 2, cnt);
    const double nan = std::nan("");
    const int k = cell[i];
    int flags = (no_mesh ? FLAG_NO_MESH : 0) | (k < 0 || k >= model.n_cells ? FLAG_BAD_CELL : 0);
    double f = nan, bg = nan, var[W::VARIANCES + 1];
    for (int c = 0; c < W::VARIANCES; ++c) var[c] = nan;
    if (flags == 0) {
      if (cnt[0] < (fit.background ? 3 : 1)) {
        flags |= FLAG_TOO_FEW;
      } else if (!W::solve(s, cnt[0], fit.background, f, bg, var)) {
        flags |= FLAG_DEGENERATE;
      }
    }
    const bool sums = (flags & (FLAG_NO_MESH | FLAG_BAD_CELL)) == 0;
    double* o = out + (size_t)COLUMNS * i;
    o[COL_FY] = pos[2 * i], o[COL_FX] = pos[2 * i + 1], o[COL_CELL] = (double)k, o[COL_FFLAGS] = (double)flags;
    o[COL_N] = (double)cnt[0], o[COL_NALL] = (double)cnt[1];
    for (int c = 0; c < W::SUMS; ++c) o[COL_FSUMS + c] = sums ? s[c] : nan;
    o[C_F] = f, o[C_F + 1] = bg;
    for (int c = 0; c < W::VARIANCES; ++c) o[C_VAR + c] = var[c];
    if (flags == 0) {
      st[FS_F * WALK_WAVES + wave] = f, st[FS_BG * WALK_WAVES + wave] = bg, go[wave] = 1;
    } else {
      o[C_RES + RES_CHI2] = o[C_RES + RES_ABS] = o[C_RES + RES_PEAK] = o[C_RES + RES_PEAK_E] = nan;
      o[C_RES + RES_PEAK_ROW] = o[C_RES + RES_PEAK_COL] = -1.0;
    }
  });
  ctx.each([&](int tid) {  // pass 2: the same pixels in the same order
    const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
    if (!go[wave]) return;
    const long i = first + wave;
    const double y = pos[2 * i], x = pos[2 * i + 1];
    const double f = st[FS_F * WALK_WAVES + wave], bg = st[FS_BG * WALK_WAVES + wave];
    const double* C = model.cube + (size_t)cell[i] * cell_words;
    double chi2 = 0.0, abs_res = 0.0;
    Peak seen{0.0, -1};
    walk_disc(fr, disc_box(y, x, fit.R), y, x, fit.R2, lane, [&](int r, int c, size_t p, double pr, double pc, double) {
      typename W::Weight w;
      if (!weights.weigh(fr, p, w)) return;
      const double m = model_at(C, N, fit.h, pr, pc);
      const double d = subtract ? (double)fr.img[p] - background_at(fr, mesh, r, c) : (double)fr.img[p];
      const double e = d - (f * m + bg);
      chi2 += W::chi2_term(w, e), abs_res += std::fabs(e);
      see_residual(seen, e, (long long)p);
    });
    acc.d[R_CHI2 * WALK_THREADS + tid] = chi2, acc.d[R_ABS * WALK_THREADS + tid] = abs_res;
    acc.d[R_PEAK * WALK_THREADS + tid] = seen.e, acc.at[tid] = seen.at;
  });
  ctx.each([&](int tid) {  // 64 partials to 8
    if (tid % WALK_LANES >= 8 || !go[tid / WALK_LANES]) return;
    fold_sums_64to8(acc, acc2, tid, R_PEAK), fold_peak_64to8(acc, acc2, tid, R_PEAK);
  });
  ctx.each([&](int tid) {  // 8 to 1
    const int wave = tid / WALK_LANES;
    if (tid % WALK_LANES != 0 || !go[wave]) return;
    double* o = out + (size_t)COLUMNS * (first + wave) + C_RES;
    fold_sums_8to1(acc2, wave, R_PEAK, o);  // RES_CHI2, RES_ABS
    const Peak seen = fold_peak_8to1(acc2, wave, R_PEAK);
    // (flags == 0 has n >= 1: there is a pixel)
    o[RES_PEAK] = std::fabs(seen.e), o[RES_PEAK_E] = seen.e;
    o[RES_PEAK_ROW] = (double)(seen.at / fr.W), o[RES_PEAK_COL] = (double)(seen.at % fr.W);
  });
}

// S8: the fit with uniform weights, rows of FIT_COLUMNS
template <class Ctx>
RPSFS_HD void s8_fit(Ctx& ctx, const Frame& fr, const double* L, const int* none, int use_mesh, const Model& model, const Fit& fit,
                     const double* pos, const int* cell, long count, long first, void* lds, double* out) {
  fit_disc(ctx, fr, L, none, use_mesh, model, fit, UniformWeights{}, pos, cell, count, first, lds, out);
}

}  // namespace rpsff
