// rpsf_core_stars_fitpos.hpp - star positions fitted with a cell of a PSF model (DESIGN.md 3.7 "Fitted positions", S9), shared with the
// CPU lane emulator tests/emu/emu_fitpos.cpp.  A driver over a context as in rpsf_core_stars.hpp.
//
//   S9  s9_fit_positions   one wave per position: the Gauss-Newton iteration of (y, x) around S8's linear fit.  A walk over S8's disc takes
//                          the thirteen sums of the linearised problem d ~ f m + bg + a_u g_u + a_v g_v (g the exact gradient of the
//                          bilinear interpolant), the wave's first lane solves the symmetric 4 x 4 (3 x 3) system by an LDL^T elimination
//                          and steps by (-a_u / f, -a_v / f), until the step is below eps, the cap of iterations, a singular system or a
//                          run-away.  It delivers the iteration's row and the position; S8 itself (s8_fit) then fits there.
//
// It reads the finder's frame, mask and filtered mesh, the positions, the cell indices and the cube, and writes its own output rows and
// nothing else: nothing S1 - S8 or D1 - D4 read or wrote changes.  No atomics at all, no workgroup waits for another.  Two runs on one input
// agree bit for bit.  This is NOT a PSF-photometry package's fit: the weights are uniform (no error column, no variance weighting), the
// interpolation is bilinear, the cell is fixed for the whole iteration, one star is fitted at a time (neighbours are not fitted together),
// and masked pixels are left out, not corrected for.
#pragma once
#include "rpsf_core_stars_fit.hpp"

#pragma clang fp contract(off)

namespace rpsfg {
using namespace rpsff;

constexpr int FITPOS_COLUMNS = 8;
enum { POS_RAN_AWAY = 1, POS_NOT_CONVERGED = 2, POS_SINGULAR = 4, POS_SKIPPED = 8 };
// a row of the output (RPSF_STARS_FITPOS_COLUMNS of include/rpsf.h)
enum { PCOL_Y0, PCOL_X0, PCOL_Y, PCOL_X, PCOL_NITER, PCOL_FLAGS, PCOL_DY, PCOL_DX };
static_assert((int)PCOL_DX + 1 == FITPOS_COLUMNS, "a row is the two positions, niter, the flags and the last step");
// the sums of a walk: the matrix of the normal equations in the basis (m, 1, g_u, g_v) - the entry of (1, 1) is the count n - and the
// right-hand sides
enum { P_SMM, P_SM, P_SMU, P_SMV, P_SU, P_SV, P_SUU, P_SUV, P_SVV, P_SDM, P_SD, P_SDU, P_SDV, P_SUMS };
static_assert((int)P_SUMS == 13, "thirteen sums and a count");

struct FitPos {
  int max_iter;
  double eps2, max_shift2, max_step;  // eps eps, max_shift max_shift
};

// what is wrong with the iteration's arguments (null: nothing)
inline const char* fitpos_problem(int max_iter, double eps, double max_shift, double max_step) {
  if (const char* why = refine_problem(max_iter, eps, max_shift)) return why;
  if (!(max_step > 0.0) || !(max_step <= MAX_RADIUS)) return "max_step must lie in 0 < max_step <= 64";
  return nullptr;
}
inline FitPos make_fitpos(int max_iter, double eps, double max_shift, double max_step) {
  return FitPos{max_iter, eps * eps, max_shift * max_shift, max_step};
}

// The model and its gradient at pixel offset (pr, pc) from the star, in exactly this order of operations: u, v, i, j, a, b
// and m are model_at's; g_u and g_v are the derivatives of the bilinear interpolant inside its cell.
struct Sample {
  double m, gu, gv;
};
RPSFS_HD Sample sample_at(const double* C, int N, double h, double pr, double pc) {
  const double u = pr + h, v = pc + h;
  const double fu = std::floor(u), fv = std::floor(v);
  const int i = (int)fu, j = (int)fv;
  const double a = u - fu, b = v - fv;
  const double* p = C + (size_t)i * N + j;
  Sample s;
  s.m = ((1.0 - a) * ((1.0 - b) * p[0] + b * p[1])) + (a * ((1.0 - b) * p[N] + b * p[N + 1]));
  s.gu = ((1.0 - b) * (p[N] - p[0])) + (b * (p[N + 1] - p[1]));
  s.gv = ((1.0 - a) * (p[1] - p[0])) + (a * (p[N + 1] - p[N]));
  return s;
}

// THE SOLVE.  A is the symmetric K x K matrix (its upper triangle is read and overwritten), b the right-hand side, K = 3 or 4.  An LDL^T
// elimination without pivoting and without square roots, in this order: for j = 0 .. K - 1: the pivot A[j][j] must be finite and > 0
// (else false); for i = j + 1 .. K - 1: l = A[j][i] / A[j][j]; for c = i .. K - 1: A[i][c] = A[i][c] - l A[j][c]; b[i] = b[i] - l b[j].
// Then back: for j = K - 1 .. 0: s = b[j]; for c = j + 1 .. K - 1: s = s - A[j][c] x[c]; x[j] = s / A[j][j].  (K is a template
// argument so that every index is a constant and the arrays stay in registers.)
template <int K>
RPSFS_HD bool solve_ldl(double (&A)[K][K], double (&b)[K], double (&x)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const double pivot = A[j][j];
    if (!finite_d(pivot) || pivot <= 0.0) return false;
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
      const double l = A[j][i] / pivot;
#pragma unroll
      for (int c = i; c < K; ++c) A[i][c] = A[i][c] - l * A[j][c];
      b[i] = b[i] - l * b[j];
    }
  }
#pragma unroll
  for (int j = K - 1; j >= 0; --j) {
    double s = b[j];
#pragma unroll
    for (int c = j + 1; c < K; ++c) s = s - A[j][c] * x[c];
    x[j] = s / A[j][j];
  }
  return true;
}

// The Gauss-Newton step of the sums `s` and the count n: false when n is below the number of unknowns or the solve fails.  With the
// constant (K = 4) the unknowns are (f, bg, a_u, a_v), without it (K = 3) (f, a_u, a_v); dy = -a_u / f, dx = -a_v / f, not yet clamped.
template <int K>
RPSFS_HD bool newton_step(const double* s, int n, double& dy, double& dx) {
  if (n < K) return false;
  double A[K][K], b[K], x[K];
  if constexpr (K == 4) {
    A[0][0] = s[P_SMM], A[0][1] = s[P_SM], A[0][2] = s[P_SMU], A[0][3] = s[P_SMV];
    A[1][1] = (double)n, A[1][2] = s[P_SU], A[1][3] = s[P_SV];
    A[2][2] = s[P_SUU], A[2][3] = s[P_SUV], A[3][3] = s[P_SVV];
    A[1][0] = A[2][0] = A[2][1] = A[3][0] = A[3][1] = A[3][2] = 0.0;  // (never read)
    b[0] = s[P_SDM], b[1] = s[P_SD], b[2] = s[P_SDU], b[3] = s[P_SDV];
  } else {
    A[0][0] = s[P_SMM], A[0][1] = s[P_SMU], A[0][2] = s[P_SMV];
    A[1][1] = s[P_SUU], A[1][2] = s[P_SUV], A[2][2] = s[P_SVV];
    A[1][0] = A[2][0] = A[2][1] = 0.0;  // (never read)
    b[0] = s[P_SDM], b[1] = s[P_SDU], b[2] = s[P_SDV];
  }
  if (!solve_ldl<K>(A, b, x)) return false;
  dy = -x[K - 2] / x[0], dx = -x[K - 1] / x[0];
  return true;
}

// ------------------------------------------------------------------------------------------------ the records in LDS
// LaneRecords (rpsf_core_stars_disc.hpp) of the P_SUMS sums, then the count n.  Behind them the state of the workgroup's WALK_WAVES stars,
// which the first lane of each wave writes and every lane of the wave reads after the barrier: the position, the last step, niter, the
// flags and the mode (S7's MODE_DONE / MODE_ITERATE).
enum { PS_Y, PS_X, PS_DY, PS_DX, PS_DOUBLES };
enum { PS_NITER, PS_FLAGS, PS_MODE, PS_INTS };
using PRecords = LaneRecords<P_SUMS, false, 1>;
RPSFS_HD constexpr size_t s9_record_bytes() { return PRecords::bytes(); }
constexpr size_t S9_STATE_BYTES = ((size_t)WALK_WAVES * (PS_DOUBLES * 8 + PS_INTS * 4) + 15) & ~(size_t)15;
RPSFS_HD constexpr size_t s9_lds_bytes() { return walk_records_bytes<PRecords>() + S9_STATE_BYTES; }
static_assert(s9_lds_bytes() <= 64 * 1024 && s9_lds_bytes() % 16 == 0, "S9's records fit the LDS a launch gets without asking");
static_assert((WALK_THREADS * s9_record_bytes()) % 16 == 0 && ((WALK_THREADS + WALK_WAVES * 8) * s9_record_bytes()) % 16 == 0,
              "the group records and the state start at multiples of 16 bytes");

// One workgroup, WALK_WAVES positions from `first` on, one wave each.  pos[2 i ..] = (y, x), cell[i] its cell of the cube, fixed for the
// whole iteration.  A WALK at p = (y, x) is walk_disc over disc_box(y, x, R) (rpsf_core_stars_disc.hpp), S8's.  For a pixel of the disc
// that lies on the frame and is usable (n), with d the residual against the mesh (use_mesh) or the pixel itself and (m, g_u, g_v) =
// sample_at:  Smm += m m, Sm += m, Smu += m g_u, Smv += m g_v, Su += g_u, Sv += g_v, Suu += g_u g_u, Suv += g_u g_v, Svv += g_v g_v, Sdm +=
// d m, Sd += d, Sdu += d g_u, Sdv += d g_v.  The fold is the disc header's.  THE DECISION, in the wave's first lane: with background the
// unknowns are (f, bg, a_u, a_v), the matrix rows (Smm Sm Smu Smv), (. n Su Sv), (. . Suu Suv), (. . . Svv) and the right-hand side (Sdm Sd
// Sdu Sdv); without it the row and column of the constant drop out.  SINGULAR: n below the number of unknowns, solve_ldl fails, or dy =
// -a_u / f, dx = -a_v / f is not finite; the star stops where it is and the last step stays what it was.  Else each of dy, dx is clamped to
// [-max_step, max_step] and becomes the last step; p' = p + (dy, dx); RAN_AWAY: (p' - p_0)^2 > max_shift^2, the star stops at p.  Else p'
// is accepted, niter += 1; dy dy + dx dx < eps eps: converged; else niter == max_iter: NOT_CONVERGED.
//
// THE ITERATION runs in ROUNDS of three each(), as S7's: the walk, the fold, and the decision of the wave's first lane, which publishes
// the new position through LDS.  Every round ends in barriers, so its trip count is the same for every thread: a round starts only while
// one of the WALK_WAVES mode words - LDS words that every thread reads alike, after a barrier and two barriers before they are written
// again - is not MODE_DONE, and there are at most max_iter rounds.  A wave whose star is finished, skipped (NO_MESH, or a cell outside
// 0 .. n_cells - 1: SKIPPED) or absent (i >= count) keeps its state and sits the remaining rounds out INSIDE the each() bodies; no thread
// skips an each().  After the rounds the first lane of every wave with a star writes its row of `out` and its position into
// final_pos[2 i ..], where S8 then fits.
template <class Ctx>
RPSFS_HD void s9_fit_positions(Ctx& ctx, const Frame& fr, const double* L, const int* none, int use_mesh, const Model& model, const Fit& fit,
                               const FitPos& fp, const double* pos, const int* cell, long count, long first, void* lds, double* out,
                               double* final_pos) {
  const PRecords acc(lds, WALK_THREADS);
  const PRecords acc2(static_cast<char*>(lds) + WALK_THREADS * s9_record_bytes(), WALK_GROUPS);
  double* st = reinterpret_cast<double*>(static_cast<char*>(lds) + walk_records_bytes<PRecords>());
  int* sti = reinterpret_cast<int*>(st + PS_DOUBLES * WALK_WAVES);
  const bool no_mesh = use_mesh && none[0] != 0;
  const bool subtract = use_mesh && !no_mesh;
  const Mesh mesh{L, fr.nbx, 0, 0};
  const int N = model.N;
  const size_t cell_words = (size_t)N * N;
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES;
    const long i = first + wave;
    if (tid % WALK_LANES != 0) return;
    const bool have = i < count;
    const bool skipped = have && (no_mesh || cell[i] < 0 || cell[i] >= model.n_cells);
    st[PS_Y * WALK_WAVES + wave] = have ? pos[2 * i] : 0.0, st[PS_X * WALK_WAVES + wave] = have ? pos[2 * i + 1] : 0.0;
    st[PS_DY * WALK_WAVES + wave] = st[PS_DX * WALK_WAVES + wave] = std::nan("");
    sti[PS_NITER * WALK_WAVES + wave] = 0;
    sti[PS_FLAGS * WALK_WAVES + wave] = skipped ? POS_SKIPPED : 0;
    sti[PS_MODE * WALK_WAVES + wave] = !have || skipped || fp.max_iter == 0 ? MODE_DONE : MODE_ITERATE;
  });
  for (int round = 0; round < fp.max_iter; ++round) {
    int active = 0;
    for (int w = 0; w < WALK_WAVES; ++w) active += sti[PS_MODE * WALK_WAVES + w] != MODE_DONE;
    if (active == 0) break;
    ctx.each([&](int tid) {  // the walk
      const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
      if (sti[PS_MODE * WALK_WAVES + wave] == MODE_DONE) return;
      const long i = first + wave;
      const double y = st[PS_Y * WALK_WAVES + wave], x = st[PS_X * WALK_WAVES + wave];
      const double* C = model.cube + (size_t)cell[i] * cell_words;
      double s[P_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      int n_use = 0;
      walk_disc(fr, disc_box(y, x, fit.R), y, x, fit.R2, lane, [&](int r, int c, size_t p, double pr, double pc, double) {
        ++n_use;
        const Sample t = sample_at(C, N, fit.h, pr, pc);
        const double d = subtract ? (double)fr.img[p] - background_at(fr, mesh, r, c) : (double)fr.img[p];
        s[P_SMM] += t.m * t.m, s[P_SM] += t.m, s[P_SMU] += t.m * t.gu, s[P_SMV] += t.m * t.gv;
        s[P_SU] += t.gu, s[P_SV] += t.gv, s[P_SUU] += t.gu * t.gu, s[P_SUV] += t.gu * t.gv, s[P_SVV] += t.gv * t.gv;
        s[P_SDM] += d * t.m, s[P_SD] += d, s[P_SDU] += d * t.gu, s[P_SDV] += d * t.gv;
      });
#pragma unroll
      for (int f = 0; f < P_SUMS; ++f) acc.d[f * WALK_THREADS + tid] = s[f];
      acc.cnt[tid] = n_use;
    });
    ctx.each([&](int tid) {  // 64 partials to 8
      const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
      if (lane >= 8 || sti[PS_MODE * WALK_WAVES + wave] == MODE_DONE) return;
      fold_sums_64to8(acc, acc2, tid, P_SUMS), fold_counts_64to8(acc, acc2, tid, 1);
    });
    ctx.each([&](int tid) {  // 8 to 1, and the wave's first lane decides
      const int wave = tid / WALK_LANES;
      if (tid % WALK_LANES != 0 || sti[PS_MODE * WALK_WAVES + wave] == MODE_DONE) return;
      const long i = first + wave;
      double s[P_SUMS];
      int n = 0;
      fold_sums_8to1(acc2, wave, P_SUMS, s), fold_counts_8to1(acc2, wave, 1, &n);
      const double y = st[PS_Y * WALK_WAVES + wave], x = st[PS_X * WALK_WAVES + wave];
      int flags = sti[PS_FLAGS * WALK_WAVES + wave], niter = sti[PS_NITER * WALK_WAVES + wave];
      bool stop = true;
      double dy = 0.0, dx = 0.0;
      const bool solved = fit.background ? newton_step<4>(s, n, dy, dx) : newton_step<3>(s, n, dy, dx);
      if (!solved || !finite_d(dy) || !finite_d(dx)) {
        flags |= POS_SINGULAR;
      } else {
        dy = dy > fp.max_step ? fp.max_step : dy < -fp.max_step ? -fp.max_step : dy;
        dx = dx > fp.max_step ? fp.max_step : dx < -fp.max_step ? -fp.max_step : dx;
        st[PS_DY * WALK_WAVES + wave] = dy, st[PS_DX * WALK_WAVES + wave] = dx;
        const double ny = y + dy, nx = x + dx;
        const double ey = ny - pos[2 * i], ex = nx - pos[2 * i + 1];
        if (ey * ey + ex * ex > fp.max_shift2) {
          flags |= POS_RAN_AWAY;
        } else {
          st[PS_Y * WALK_WAVES + wave] = ny, st[PS_X * WALK_WAVES + wave] = nx;
          ++niter;
          if (dy * dy + dx * dx < fp.eps2) {
            // converged
          } else if (niter == fp.max_iter) {
            flags |= POS_NOT_CONVERGED;
          } else {
            stop = false;
          }
        }
      }
      sti[PS_FLAGS * WALK_WAVES + wave] = flags, sti[PS_NITER * WALK_WAVES + wave] = niter;
      if (stop) sti[PS_MODE * WALK_WAVES + wave] = MODE_DONE;
    });
  }
  ctx.each([&](int tid) {  // the rows
    const int wave = tid / WALK_LANES;
    const long i = first + wave;
    if (tid % WALK_LANES != 0 || i >= count) return;
    double* o = out + (size_t)FITPOS_COLUMNS * i;
    o[PCOL_Y0] = pos[2 * i], o[PCOL_X0] = pos[2 * i + 1];
    o[PCOL_Y] = st[PS_Y * WALK_WAVES + wave], o[PCOL_X] = st[PS_X * WALK_WAVES + wave];
    o[PCOL_NITER] = (double)sti[PS_NITER * WALK_WAVES + wave], o[PCOL_FLAGS] = (double)sti[PS_FLAGS * WALK_WAVES + wave];
    o[PCOL_DY] = st[PS_DY * WALK_WAVES + wave], o[PCOL_DX] = st[PS_DX * WALK_WAVES + wave];
    final_pos[2 * i] = st[PS_Y * WALK_WAVES + wave], final_pos[2 * i + 1] = st[PS_X * WALK_WAVES + wave];
  });
}

}  // namespace rpsfg
