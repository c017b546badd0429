// rpsf_core_stars_refine.hpp - Gaussian-windowed positions and moments at positions the caller supplies (DESIGN.md 3.7 "Windowed
// positions", S7), shared with the CPU lane emulator tests/emu/emu_refine.cpp.  A driver over a context as in rpsf_core_stars.hpp.
//
//   S7  s7_refine   one wave per position: the iteration p <- p + 2 (sum w d (r - p)) / (sum w d) under the window w = g(q / 2 sigma^2),
//                   q <= (4 sigma)^2, until the step is below eps, the cap of iterations, no flux or a run-away; then the same walk once
//                   more at the position returned: the counts, sum w d, sum w |d| and the raw first and second windowed moments
//
// It reads the finder's frame, mask and filtered mesh, the positions and the sigmas, and writes its own output rows and nothing else:
// nothing S1 - S6 or D1 - D4 read or wrote changes.  No atomics at all, no workgroup waits for another.  Two runs on one input agree bit
// for bit.  This is NOT sep's winpos: no sub-pixel sampling of the window's rim, the comparison is q <= R R, and masked pixels are left out
// and reported, not corrected for.
#pragma once
#include "rpsf_core_stars_photometry.hpp"

#pragma clang fp contract(off)

namespace rpsfr {
using namespace rpsfp;

constexpr int REFINE_COLUMNS = 18, MAX_ITER = 64;
constexpr double MIN_SIGMA = 0.5, MAX_SIGMA = 16.0, WINDOW_RADII = 4.0;  // R = 4 sigma <= MAX_RADIUS
enum { FLAG_NO_FLUX = 1, FLAG_RAN_AWAY = 2, FLAG_NOT_CONVERGED = 4 };
// a row of the output (RPSF_STARS_REFINE_COLUMNS of include/rpsf.h)
enum { COL_Y0, COL_X0, COL_Y, COL_X, COL_SIGMA, COL_NITER, COL_FLAGS, COL_DY, COL_DX, COL_N_USE, COL_N_ALL, COL_SUMS };
enum { W_S, W_ABS, W_MR, W_MC, W_MRR, W_MCC, W_MRC, W_SUMS };  // sum t, sum w |d|, sum t pr, t pc, t (pr pr), t (pc pc), t (pr pc); t = w d
static_assert((int)COL_SUMS + (int)W_SUMS == REFINE_COLUMNS, "a row is the nine scalars, the two counts and the seven sums");

struct Refine {
  int max_iter;
  double eps2, max_shift2;  // eps eps, max_shift max_shift
};

// what is wrong with the iteration's arguments (null: nothing)
inline const char* refine_problem(int max_iter, double eps, double max_shift) {
  if (max_iter < 0 || max_iter > MAX_ITER) return "max_iter must lie in 0 ... 64";
  if (!(eps > 0.0) || !(eps <= 1.7976931348623157e308)) return "eps must be positive and finite";
  if (!(max_shift > 0.0) || !(max_shift <= MAX_RADIUS)) return "max_shift must lie in 0 < max_shift <= 64";
  return nullptr;
}
inline bool sigma_ok(double sigma) { return sigma >= MIN_SIGMA && sigma <= MAX_SIGMA; }  // (false for NaN)
inline Refine make_refine(int max_iter, double eps, double max_shift) { return Refine{max_iter, eps * eps, max_shift * max_shift}; }

RPSFS_HD bool finite_d(double v) { return std::fabs(v) <= 1.7976931348623157e308; }

// ------------------------------------------------------------------------------------------------ the window function
// g(t) = exp(-t) for 0 <= t <= 8 (and a little beyond) in float64 + - x only, so that the kernel, the emulator and the NumPy restatement
// give the same bits where the math libraries' exp would not.  Operation for operation:
//   n = the integer part of t LOG2E + 0.5 (the argument is not negative: truncation is floor);   r = (t - n LN2_HI) - n LN2_LO;
//   z = -r;   p = 1/13!;  p = p z + 1/j!  for j = 12 ... 0;   g = p 2^-n, the power of two built from its exponent bits.
// 1/j! is the float64 quotient 1.0 / j! (j! is exact up to 13!).
constexpr double LOG2E = 1.44269504088896338700e+00, LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
RPSFS_HD double window_g(double t) {
  const int n = (int)(t * LOG2E + 0.5);
  const double r = (t - (double)n * LN2_HI) - (double)n * LN2_LO;
  const double z = -r;
  double p = 1.0 / 6227020800.0;
  p = p * z + 1.0 / 479001600.0;
  p = p * z + 1.0 / 39916800.0;
  p = p * z + 1.0 / 3628800.0;
  p = p * z + 1.0 / 362880.0;
  p = p * z + 1.0 / 40320.0;
  p = p * z + 1.0 / 5040.0;
  p = p * z + 1.0 / 720.0;
  p = p * z + 1.0 / 120.0;
  p = p * z + 1.0 / 24.0;
  p = p * z + 1.0 / 6.0;
  p = p * z + 1.0 / 2.0;
  p = p * z + 1.0;
  p = p * z + 1.0;
  const uint64_t bits = (uint64_t)(1023 - n) << 52;  // 2^-n, n = 0 ... 12
  double scale;
  std::memcpy(&scale, &bits, 8);
  return p * scale;
}

// ------------------------------------------------------------------------------------------------ the records in LDS
// LaneRecords (rpsf_core_stars_disc.hpp) of the W_SUMS sums, then N_use and N_all.  Behind them the state of the workgroup's WALK_WAVES
// stars, which the first lane of each wave writes and every lane of the wave reads after the barrier: the position, the last step, niter,
// the flags and the mode.
enum { MODE_DONE, MODE_ITERATE, MODE_MEASURE };
enum { ST_Y, ST_X, ST_DY, ST_DX, ST_DOUBLES };
enum { ST_NITER, ST_FLAGS, ST_MODE, ST_INTS };
using WRecords = LaneRecords<W_SUMS, false, 2>;
RPSFS_HD constexpr size_t s7_record_bytes() { return WRecords::bytes(); }
constexpr size_t S7_STATE_BYTES = ((size_t)WALK_WAVES * (ST_DOUBLES * 8 + ST_INTS * 4) + 15) & ~(size_t)15;
RPSFS_HD constexpr size_t s7_lds_bytes() { return walk_records_bytes<WRecords>() + S7_STATE_BYTES; }

// One workgroup, WALK_WAVES positions from `first` on, one wave each.  pos[2 i ..] = (y, x), sigma[i] its window.  A WALK at p = (y, x):
// R = 4 sigma, h = 1 / (2 sigma sigma); walk_disc over disc_box(y, x, R) (rpsf_core_stars_disc.hpp).  A pixel of the window counts in N_all,
// and then, when it lies on the frame and is usable (N_use), with d the residual against the mesh (use_mesh) or the pixel itself, w = g(q h)
// and t = w d:  sum t, w |d|, t pr, t pc, t (pr pr), t (pc pc), t (pr pc), the products grouped as written.  The fold is the disc header's.
//
// THE ITERATION (rpsf.h) runs in ROUNDS of three each(): the walk, the fold, and the decision of the wave's first lane,
// which publishes the new position through LDS.  Every round ends in barriers, so its trip count is the same for every thread: a round
// starts only while one of the WALK_WAVES mode words - LDS words that every thread reads alike, after a barrier and two barriers before
// they are written again - is not MODE_DONE, and there are at most max_iter + 1 rounds.  A wave whose star is finished (or has none:
// i >= count) keeps its state and sits the remaining rounds out INSIDE the each() bodies; no thread skips an each().
// A star in MODE_MEASURE takes the walk whose sums are delivered; a stop without flux or by running away delivers the walk just made, which
// is that walk.  With use_mesh and none[0] set (no valid mesh node) nothing iterates: flag NO_FLUX, every sum NaN, the counts delivered.
template <class Ctx>
RPSFS_HD void s7_refine(Ctx& ctx, const Frame& fr, const double* L, const int* none, int use_mesh, const Refine& rf, const double* pos,
                        const double* sigma, long count, long first, void* lds, double* out) {
  const WRecords acc(lds, WALK_THREADS);
  const WRecords acc2(static_cast<char*>(lds) + WALK_THREADS * s7_record_bytes(), WALK_GROUPS);
  double* st = reinterpret_cast<double*>(static_cast<char*>(lds) + walk_records_bytes<WRecords>());
  int* sti = reinterpret_cast<int*>(st + ST_DOUBLES * WALK_WAVES);
  const bool no_mesh = use_mesh && none[0] != 0;
  const bool subtract = use_mesh && !no_mesh;
  const Mesh mesh{L, fr.nbx, 0, 0};
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES;
    const long i = first + wave;
    if (tid % WALK_LANES != 0) return;
    const bool have = i < count;
    st[ST_Y * WALK_WAVES + wave] = have ? pos[2 * i] : 0.0, st[ST_X * WALK_WAVES + wave] = have ? pos[2 * i + 1] : 0.0;
    st[ST_DY * WALK_WAVES + wave] = st[ST_DX * WALK_WAVES + wave] = std::nan("");
    sti[ST_NITER * WALK_WAVES + wave] = 0;
    sti[ST_FLAGS * WALK_WAVES + wave] = have && no_mesh ? FLAG_NO_FLUX : 0;
    sti[ST_MODE * WALK_WAVES + wave] = !have ? MODE_DONE : (no_mesh || rf.max_iter == 0) ? MODE_MEASURE : MODE_ITERATE;
  });
  for (int round = 0; round <= rf.max_iter; ++round) {
    int active = 0;
    for (int w = 0; w < WALK_WAVES; ++w) active += sti[ST_MODE * WALK_WAVES + w] != MODE_DONE;
    if (active == 0) break;
    ctx.each([&](int tid) {  // the walk
      const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
      if (sti[ST_MODE * WALK_WAVES + wave] == MODE_DONE) return;
      const long i = first + wave;
      const double y = st[ST_Y * WALK_WAVES + wave], x = st[ST_X * WALK_WAVES + wave], sg = sigma[i];
      const double R = WINDOW_RADII * sg, R2 = R * R, h = 1.0 / (2.0 * sg * sg);
      double s[W_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      int n_use = 0, n_all = 0;
      walk_disc(fr, disc_box(y, x, R), y, x, R2, lane, [&](double, double) { ++n_all; }, [&](int r, int c, size_t p, double pr, double pc, double q) {
        ++n_use;
        const double d = subtract ? (double)fr.img[p] - background_at(fr, mesh, r, c) : (double)fr.img[p];
        const double w = window_g(q * h), t = w * d;
        s[W_S] += t, s[W_ABS] += w * std::fabs(d);
        s[W_MR] += t * pr, s[W_MC] += t * pc;
        s[W_MRR] += t * (pr * pr), s[W_MCC] += t * (pc * pc), s[W_MRC] += t * (pr * pc);
      });
#pragma unroll
      for (int f = 0; f < W_SUMS; ++f) acc.d[f * WALK_THREADS + tid] = s[f];
      acc.cnt[tid] = n_use, acc.cnt[WALK_THREADS + tid] = n_all;
    });
    ctx.each([&](int tid) {  // 64 partials to 8
      const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
      if (lane >= 8 || sti[ST_MODE * WALK_WAVES + wave] == MODE_DONE) return;
      fold_sums_64to8(acc, acc2, tid, W_SUMS), fold_counts_64to8(acc, acc2, tid, 2);
    });
    ctx.each([&](int tid) {  // 8 to 1, and the wave's first lane decides
      const int wave = tid / WALK_LANES;
      if (tid % WALK_LANES != 0 || sti[ST_MODE * WALK_WAVES + wave] == MODE_DONE) return;
      const long i = first + wave;
      double s[W_SUMS];
      int cnt[2];
      fold_sums_8to1(acc2, wave, W_SUMS, s), fold_counts_8to1(acc2, wave, 2, cnt);
      const double y = st[ST_Y * WALK_WAVES + wave], x = st[ST_X * WALK_WAVES + wave];
      int flags = sti[ST_FLAGS * WALK_WAVES + wave], niter = sti[ST_NITER * WALK_WAVES + wave];
      bool deliver = sti[ST_MODE * WALK_WAVES + wave] == MODE_MEASURE;
      if (!deliver) {
        if (!finite_d(s[W_S]) || s[W_S] <= 0.0) {
          flags |= FLAG_NO_FLUX, deliver = true;
        } else {
          const double dy = s[W_MR] / s[W_S], dx = s[W_MC] / s[W_S];
          const double ny = y + 2.0 * dy, nx = x + 2.0 * dx;
          const double ey = ny - pos[2 * i], ex = nx - pos[2 * i + 1];
          st[ST_DY * WALK_WAVES + wave] = dy, st[ST_DX * WALK_WAVES + wave] = dx;
          if (!finite_d(ny) || !finite_d(nx) || ey * ey + ex * ex > rf.max_shift2) {
            flags |= FLAG_RAN_AWAY, deliver = true;
          } else {
            st[ST_Y * WALK_WAVES + wave] = ny, st[ST_X * WALK_WAVES + wave] = nx;
            ++niter;
            if (dy * dy + dx * dx < rf.eps2) {
              sti[ST_MODE * WALK_WAVES + wave] = MODE_MEASURE;
            } else if (niter == rf.max_iter) {
              flags |= FLAG_NOT_CONVERGED, sti[ST_MODE * WALK_WAVES + wave] = MODE_MEASURE;
            }
          }
        }
        sti[ST_FLAGS * WALK_WAVES + wave] = flags, sti[ST_NITER * WALK_WAVES + wave] = niter;
      }
      if (!deliver) return;
      sti[ST_MODE * WALK_WAVES + wave] = MODE_DONE;
      const double nan = std::nan("");
      double* o = out + (size_t)REFINE_COLUMNS * i;
      o[COL_Y0] = pos[2 * i], o[COL_X0] = pos[2 * i + 1], o[COL_Y] = y, o[COL_X] = x, o[COL_SIGMA] = sigma[i];
      o[COL_NITER] = (double)niter, o[COL_FLAGS] = (double)flags;
      o[COL_DY] = st[ST_DY * WALK_WAVES + wave], o[COL_DX] = st[ST_DX * WALK_WAVES + wave];
      o[COL_N_USE] = (double)cnt[0], o[COL_N_ALL] = (double)cnt[1];
      for (int f = 0; f < W_SUMS; ++f) o[COL_SUMS + f] = no_mesh ? nan : s[f];
    });
  }
}

}  // namespace rpsfr
