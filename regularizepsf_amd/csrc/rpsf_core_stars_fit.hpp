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

// the total order of the residual's peak: larger |e| (a NaN counts as +inf), then the smaller linear index
RPSFS_HD double peak_key(double e) {
  const double a = std::fabs(e);
  return a == a ? a : (double)INFINITY;
}
struct Peak {
  double e;
  long long at;
};
RPSFS_HD void see_residual(Peak& s, double e, long long at) {
  if (at < 0) return;
  const double k = peak_key(e), have = peak_key(s.e);
  if (s.at < 0 || k > have || (k == have && at < s.at)) s.e = e, s.at = at;
}

// ------------------------------------------------------------------------------------------------ the records in LDS
// One record per lane and one per group of 8 lanes, field-major as S6's and S7's (field f of record i of n is word f n + i): F_SUMS
// doubles, the peak's linear index (64 bits, < 0: no pixel yet), then n and n_all.  Pass 2 puts its R_SUMS doubles into the first words
// of pass 1's.  Behind them what the first lane of each wave hands to its lanes after the solve: f, bg and whether pass 2 runs.
enum { FS_F, FS_BG, FS_DOUBLES };
RPSFS_HD constexpr size_t s8_record_bytes() { return (size_t)F_SUMS * 8 + 8 + 2 * 4; }
constexpr size_t S8_STATE_BYTES = ((size_t)WALK_WAVES * (FS_DOUBLES * 8 + 4) + 15) & ~(size_t)15;
RPSFS_HD constexpr size_t s8_lds_bytes() { return (size_t)(WALK_THREADS + WALK_WAVES * 8) * s8_record_bytes() + S8_STATE_BYTES; }
static_assert((int)R_SUMS <= (int)F_SUMS, "pass 2's fields lie in pass 1's words");

struct FRecords {  // n records at `base` (a multiple of 16 bytes: n is a multiple of 4)
  double* d;
  long long* at;
  int* cnt;
  int n;
  RPSFS_HD FRecords(void* base, int n_) : d(static_cast<double*>(base)), n(n_) {
    at = reinterpret_cast<long long*>(d + (size_t)F_SUMS * n_);
    cnt = reinterpret_cast<int*>(at + n_);
  }
};

// One workgroup, WALK_WAVES positions from `first` on, one wave each.  pos[2 i ..] = (y, x), cell[i] its cell of the cube.  The box runs
// from floor(y - R) - 1 to ceil(y + R) + 1 and likewise in x, not clipped to the frame; lane j takes its pixels j, j + 64, ... in raster
// order.  For pixel (r, c): pr = r - y, pc = c - x, q = pr pr + pc pc; it is in the disc when q <= R R (n_all, and m = model_at into
// Sm_all), and then, when it lies on the frame and is usable (n), with d the residual against the mesh (use_mesh) or the pixel itself:
// Sm += m, Smm += m m, Sd += d, Sdm += d m, Sdd += d d.  The 64 partial records fold as 8 groups of 8, each in lane order, and the 8
// groups in order.  THE SOLVE, in the wave's first lane, in this order: with background D = n Smm - Sm Sm, f = (n Sdm - Sm Sd) / D,
// bg = (Sd - f Sm) / n; without it D = Smm, f = Sdm / Smm, bg = 0.  TOO_FEW: n < 3 (with background) or n < 1; else DEGENERATE: D not
// finite or D <= 0; either way f, bg and pass 2's columns are NaN (the peak at (-1, -1)).  PASS 2 walks the same pixels in the same order
// with e = d - (f m + bg): chi2 = sum e e, abs_res = sum |e|, and the peak by see_residual's order.
// With use_mesh and none[0] set (NO_MESH) or a cell outside 0 .. n_cells - 1 (BAD_CELL) only the counts are taken - neither `L` nor the
// cube is read - and every sum, f, bg and pass 2's columns are NaN.
template <class Ctx>
RPSFS_HD void s8_fit(Ctx& ctx, const Frame& fr, const double* L, const int* none, int use_mesh, const Model& model, const Fit& fit,
                     const double* pos, const int* cell, long count, long first, void* lds, double* out) {
  const FRecords acc(lds, WALK_THREADS);
  const FRecords acc2(static_cast<char*>(lds) + WALK_THREADS * s8_record_bytes(), WALK_WAVES * 8);
  double* st = reinterpret_cast<double*>(static_cast<char*>(lds) + (WALK_THREADS + WALK_WAVES * 8) * s8_record_bytes());
  int* go = reinterpret_cast<int*>(st + FS_DOUBLES * WALK_WAVES);
  const bool no_mesh = use_mesh && none[0] != 0;
  const bool subtract = use_mesh && !no_mesh;
  const Mesh mesh{L, fr.nbx, 0, 0};
  const int N = model.N;
  const size_t cell_words = (size_t)N * N;
  ctx.each([&](int tid) {  // pass 1
    const long i = first + tid / WALK_LANES;
    const int lane = tid % WALK_LANES;
    double s[F_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
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
        if (!counts_only) m = model_at(C, N, fit.h, pr, pc), s[F_SM_ALL] += m;
        if (r < 0 || r >= fr.H || c < 0 || c >= fr.W) continue;
        const size_t p = (size_t)r * fr.W + c;
        if (!usable(fr.img, fr.mask, p)) continue;
        ++n_use;
        if (counts_only) continue;
        const double d = subtract ? (double)fr.img[p] - background_at(fr, mesh, r, c) : (double)fr.img[p];
        s[F_SM] += m, s[F_SMM] += m * m, s[F_SD] += d, s[F_SDM] += d * m, s[F_SDD] += d * d;
      }
    }
#pragma unroll
    for (int f = 0; f < F_SUMS; ++f) acc.d[f * WALK_THREADS + tid] = s[f];
    acc.cnt[tid] = n_use, acc.cnt[WALK_THREADS + tid] = n_all;
  });
  ctx.each([&](int tid) {  // 64 partials to 8
    const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
    if (lane >= 8) return;
    const int G = WALK_WAVES * 8, i0 = wave * WALK_LANES + 8 * lane, g = wave * 8 + lane;
    for (int f = 0; f < F_SUMS; ++f) {
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
    double s[F_SUMS];
    for (int f = 0; f < F_SUMS; ++f) {
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
    double f = nan, bg = nan;
    if (flags == 0) {
      const double n = (double)cnt[0];
      if (cnt[0] < (fit.background ? 3 : 1)) {
        flags |= FLAG_TOO_FEW;
      } else if (fit.background) {
        const double D = n * s[F_SMM] - s[F_SM] * s[F_SM];
        if (!finite_d(D) || D <= 0.0) {
          flags |= FLAG_DEGENERATE;
        } else {
          f = (n * s[F_SDM] - s[F_SM] * s[F_SD]) / D;
          bg = (s[F_SD] - f * s[F_SM]) / n;
        }
      } else {
        const double D = s[F_SMM];
        if (!finite_d(D) || D <= 0.0) {
          flags |= FLAG_DEGENERATE;
        } else {
          f = s[F_SDM] / D;
          bg = 0.0;
        }
      }
    }
    const bool sums = (flags & (FLAG_NO_MESH | FLAG_BAD_CELL)) == 0;
    double* o = out + (size_t)FIT_COLUMNS * i;
    o[COL_FY] = pos[2 * i], o[COL_FX] = pos[2 * i + 1], o[COL_CELL] = (double)k, o[COL_FFLAGS] = (double)flags;
    o[COL_N] = (double)cnt[0], o[COL_NALL] = (double)cnt[1];
    for (int c = 0; c < F_SUMS; ++c) o[COL_FSUMS + c] = sums ? s[c] : nan;
    o[COL_F] = f, o[COL_BG] = bg;
    if (flags == 0) {
      st[FS_F * WALK_WAVES + wave] = f, st[FS_BG * WALK_WAVES + wave] = bg, go[wave] = 1;
    } else {
      o[COL_CHI2] = o[COL_ABS_RES] = o[COL_PEAK_RES] = o[COL_PEAK_E] = nan;
      o[COL_PEAK_ROW] = o[COL_PEAK_COL] = -1.0;
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
      const double m = model_at(C, N, fit.h, pr, pc);
      const double d = subtract ? (double)fr.img[p] - background_at(fr, mesh, r, c) : (double)fr.img[p];
      const double e = d - (f * m + bg);
      chi2 += e * e, abs_res += std::fabs(e);
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
    double* o = out + (size_t)FIT_COLUMNS * (first + wave);
    for (int f = 0; f < R_PEAK; ++f) {
      double v = 0.0;
      for (int j = 0; j < 8; ++j) v += acc2.d[f * G + g0 + j];
      o[COL_CHI2 + f] = v;
    }
    Peak seen{0.0, -1};
    for (int j = 0; j < 8; ++j) see_residual(seen, acc2.d[R_PEAK * G + g0 + j], acc2.at[g0 + j]);
    // (flags == 0 has n >= 1: there is a pixel)
    o[COL_PEAK_RES] = std::fabs(seen.e), o[COL_PEAK_E] = seen.e;
    o[COL_PEAK_ROW] = (double)(seen.at / fr.W), o[COL_PEAK_COL] = (double)(seen.at % fr.W);
  });
}

}  // namespace rpsff
