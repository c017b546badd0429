// rpsf_core_stars_fit_group.hpp - joint linear least-squares fits of blended neighbours with their cells of a PSF model (DESIGN.md 3.7
// "Group fits", S11), shared with the CPU lane emulator tests/emu/emu_group.cpp.  A driver over a context as in rpsf_core_stars.hpp; the
// context also keeps a Lane of registers per thread (ctx.regs(tid)), because a lane's sums outlive an each().
//
//   S11 s11_fit_group   one wave per group of g = 2 .. MAX_GROUP stars whose fit discs overlap (rpsf_core_stars_group.hpp): one flux per
//                       star and one shared constant, positions fixed.  Pass 1 walks the union of the discs for the normal equations,
//                       the wave's first lane solves them by S9's LDL^T elimination at a runtime order, and pass 2 walks every member's
//                       disc for S8's own sums and the residual against the sum of the members' models
//
// It reads the finder's frame, mask and filtered mesh, the positions, the cell indices, the groups and the cube, and writes its own
// output rows and nothing else.  No atomics at all, no workgroup waits for another.  Two runs on one input agree bit for bit.  The model,
// the usable-pixel rule, d, the box, the disc test and the fold are S8's, the sum of the members' models at a pixel is S10's.  This is NOT
// a PSF-photometry package's fit: the weights are uniform (no error column, no variance weighting), the positions are given and not
// fitted, the interpolation is bilinear, the model is cut at R, the cell of a star is fixed, and nothing guards near-coincident stars -
// their system is near-singular and the fluxes come out huge and of opposite sign - but DEGENERATE at a pivot that is not positive.
#pragma once
#include "rpsf_core_stars_fit.hpp"
#include "rpsf_core_stars_group.hpp"

#pragma clang fp contract(off)

namespace rpsfj {
using namespace rpsff;
using rpsfq::MAX_GROUP;

constexpr int GROUP_COLUMNS = FIT_COLUMNS + 5, MAX_UNKNOWNS = MAX_GROUP + 1;
// a row of the output (RPSF_STARS_FIT_GROUPS_COLUMNS of include/rpsf.h): S8's columns with S8's meanings, then these
enum { COL_GROUP = FIT_COLUMNS, COL_GROUP_SIZE, COL_GROUP_N, COL_GROUP_CHI2, COL_GROUP_ABS };
static_assert((int)COL_GROUP_ABS + 1 == GROUP_COLUMNS, "a row is S8's row, the group's label and size, and the group's n, chi2 and abs_res");

// the sums of pass 1 that a lane carries: the upper triangle of A row by row, Sm[b], Sdm[b], Sd, Sdd; and the count n
constexpr int TRIANGLE = MAX_GROUP * (MAX_GROUP + 1) / 2;
RPSFS_HD constexpr int tri(int b, int c) { return b * MAX_GROUP - b * (b - 1) / 2 + (c - b); }  // b <= c
enum { G_A = 0, G_SM = TRIANGLE, G_SDM = G_SM + MAX_GROUP, G_SD = G_SDM + MAX_GROUP, G_SDD, G_FIELDS };
static_assert(tri(MAX_GROUP - 1, MAX_GROUP - 1) + 1 == TRIANGLE && (int)G_FIELDS == 36 + 8 + 8 + 2, "36 + 8 + 8 + 2 doubles and a count");
struct Lane {
  double v[G_FIELDS];  // pass 2 keeps the group's running sum e e in v[0] and sum |e| in v[1]
  int n;
};
// pass 2's fields of a member in the fold's records: S8's six sums, then sum e e, sum |e| and the signed e of the peak
enum { M_CHI2 = F_SUMS, M_ABS, M_PEAK, M_FIELDS };

// the groups of a call: group k has the stars members[starts[k] .. starts[k + 1]), ascending, 2 .. MAX_GROUP of them
struct GroupList {
  const long long* starts;
  const int* members;
  long count;
};

// ------------------------------------------------------------------------------------------------ the records in LDS
// The fold's records are LaneRecords (rpsf_core_stars_disc.hpp): FOLD_BATCH doubles per lane and per group of 8 lanes - pass 1's
// G_FIELDS sums go through them FOLD_BATCH at a time -, the peak's linear index and two counts.  Behind them the state
// of the workgroup's WALK_WAVES groups: pass 1's totals, the system of the solve (the matrix, the right-hand side, the unknowns: they are
// indexed at run time, which registers cannot be), the constant, and g, n, the flags and whether pass 2 takes residuals.
constexpr int FOLD_BATCH = 18;
static_assert(G_FIELDS % FOLD_BATCH == 0 && (int)M_FIELDS <= FOLD_BATCH, "pass 1 folds in whole batches, pass 2 in one");
enum { GS_TOTALS = 0, GS_MATRIX = G_FIELDS, GS_RHS = GS_MATRIX + MAX_UNKNOWNS * MAX_UNKNOWNS, GS_X = GS_RHS + MAX_UNKNOWNS, GS_BG = GS_X + MAX_UNKNOWNS, GS_DOUBLES };
enum { GI_G, GI_N, GI_FLAGS, GI_GO, GI_INTS };
using GRecords = LaneRecords<FOLD_BATCH, true, 2>;
RPSFS_HD constexpr size_t s11_record_bytes() { return GRecords::bytes(); }
constexpr size_t S11_STATE_BYTES = ((size_t)WALK_WAVES * (GS_DOUBLES * 8 + GI_INTS * 4) + 15) & ~(size_t)15;
RPSFS_HD constexpr size_t s11_lds_bytes() { return walk_records_bytes<GRecords>() + S11_STATE_BYTES; }
static_assert(s11_lds_bytes() <= 64 * 1024 && s11_lds_bytes() % 16 == 0, "S11's records fit the LDS a launch gets without asking");

// THE SOLVE at a runtime order K <= MAX_UNKNOWNS: S9's solve_ldl with the same order of elimination and substitution.  A is the
// symmetric matrix in rows of MAX_UNKNOWNS (its upper triangle is read and overwritten), b the right-hand side.  False at a pivot that is
// not finite or <= 0.
RPSFS_HD bool solve_ldl_n(int K, double* A, double* b, double* x) {
  for (int j = 0; j < K; ++j) {
    const double pivot = A[j * MAX_UNKNOWNS + j];
    if (!finite_d(pivot) || pivot <= 0.0) return false;
    for (int i = j + 1; i < K; ++i) {
      const double l = A[j * MAX_UNKNOWNS + i] / pivot;
      for (int c = i; c < K; ++c) A[i * MAX_UNKNOWNS + c] = A[i * MAX_UNKNOWNS + c] - l * A[j * MAX_UNKNOWNS + c];
      b[i] = b[i] - l * b[j];
    }
  }
  for (int j = K - 1; j >= 0; --j) {
    double s = b[j];
    for (int c = j + 1; c < K; ++c) s = s - A[j * MAX_UNKNOWNS + c] * x[c];
    x[j] = s / A[j * MAX_UNKNOWNS + j];
  }
  return true;
}

// The fold of pass 1's fields F0 .. F0 + FOLD_BATCH - 1 (F0 is a template argument so that every index into a lane's registers is a
// constant): the lanes' partials into the records, 64 partials to 8, 8 to 1 into the wave's totals; the count goes with the first batch.
template <int f0, class Ctx>
RPSFS_HD void s11_fold(Ctx& ctx, const GRecords& acc, const GRecords& acc2, double* st, int* sti) {
  ctx.each([&](int tid) {
    const Lane& s = ctx.regs(tid);
#pragma unroll
    for (int f = 0; f < FOLD_BATCH; ++f) acc.d[f * WALK_THREADS + tid] = s.v[f0 + f];
    if (f0 == 0) acc.cnt[tid] = s.n;
  });
  ctx.each([&](int tid) {  // 64 partials to 8
    if (tid % WALK_LANES >= 8) return;
    fold_sums_64to8(acc, acc2, tid, FOLD_BATCH);
    if (f0 == 0) fold_counts_64to8(acc, acc2, tid, 1);
  });
  ctx.each([&](int tid) {  // 8 to 1, into the wave's totals
    const int wave = tid / WALK_LANES;
    if (tid % WALK_LANES != 0) return;
    fold_sums_8to1(acc2, wave, FOLD_BATCH, st + (size_t)wave * GS_DOUBLES + GS_TOTALS + f0);
    if (f0 == 0) fold_counts_8to1(acc2, wave, 1, sti + GI_N * WALK_WAVES + wave);
  });
}

// One workgroup, WALK_WAVES groups from `first` on, one wave each.  pos[2 i ..] = (y, x) and cell[i] of EVERY star of the call; the
// members of a group index them.  Every member's cell lies inside the model and use_mesh comes with a valid mesh (the driver sends every
// other star through S8).  Member b's disc HOLDS pixel (r, c) when, with pr = r - y_b, pc = c - x_b, q = pr pr + pc pc: q <= R R.
//
// PASS 1.  For a = 0 .. g - 1: member a's disc_box (rpsf_core_stars_disc.hpp), lane j takes its pixels j, j + 64, ... in raster order.  A
// pixel counts when disc a holds it, no disc b < a does - every pixel of the union is OWNED by the first member that holds it -, it lies on
// the frame and is usable.  With d S8's d and m_b = model_at of member b for the members (ascending) that hold it: n += 1, Sd += d, Sdd +=
// d d, Sm[b] += m_b, Sdm[b] += d m_b, and for c >= b, both holding: A[b][c] += m_b m_c.  A lane's partial sums run on across the members.
// They fold by the disc header's steps.
// THE SOLVE, in the wave's first lane.  The unknowns are f_0 .. f_{g-1}, then the constant when fit.background: p = g + background.
// The matrix is A bordered by Sm and n, the right-hand side Sdm, then Sd.  TOO_FEW: n < p.  Else solve_ldl_n; DEGENERATE: a pivot not
// finite or <= 0, or an unknown not finite.  Either flag goes to every member and leaves NaN in f, bg and the residual's columns.
// PASS 2.  For a = 0 .. g - 1, walk_disc over member a's disc as S8's pass 1 walks that star alone: n_all and Sm_all over the disc, and on
// its usable pixels n_use and, through UniformWeights::add - the function S8's pass 1 calls -, Sm, Smm, Sd, Sdm, Sdd: S8's row of that
// star, bit for bit.  Without a flag also e = d - (S + bg) with S = 0.0,
// then S += f_b * m_b over the members b (ascending) that hold the pixel - S10's sum -: chi2 += e e, abs_res += |e|, the peak by
// see_residual; and on the pixels a owns the group's gchi2 += e e, gabs += |e|, whose lane partials run on across the members and fold
// once, after the last.  A member without a usable pixel has no peak: peak_res and peak_e NaN at (-1, -1).
// The rows of `out` are in the order of `members` (row starts[k] + a is member a of group k); the host puts them where the stars are.
// Every each() is passed by every thread: the member loop of pass 2 runs to the largest g of the workgroup's waves, read from LDS.
template <class Ctx>
RPSFS_HD void s11_fit_group(Ctx& ctx, const Frame& fr, const double* L, int use_mesh, const Model& model, const Fit& fit, const double* pos,
                            const int* cell, const GroupList& groups, long first, void* lds, double* out) {
  const GRecords acc(lds, WALK_THREADS);
  const GRecords acc2(static_cast<char*>(lds) + WALK_THREADS * s11_record_bytes(), WALK_GROUPS);
  double* st = reinterpret_cast<double*>(static_cast<char*>(lds) + walk_records_bytes<GRecords>());
  int* sti = reinterpret_cast<int*>(st + (size_t)GS_DOUBLES * WALK_WAVES);
  const bool subtract = use_mesh != 0;
  const Mesh mesh{L, fr.nbx, 0, 0};
  const int N = model.N;
  const size_t cell_words = (size_t)N * N;
  ctx.each([&](int tid) {  // pass 1
    const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
    Lane& s = ctx.regs(tid);
#pragma unroll
    for (int f = 0; f < G_FIELDS; ++f) s.v[f] = 0.0;
    s.n = 0;
    const long k = first + wave;
    if (k >= groups.count) return;
    const long long m0 = groups.starts[k];
    const int g = (int)(groups.starts[k + 1] - m0);
    double y[MAX_GROUP], x[MAX_GROUP];
    const double* C[MAX_GROUP];
#pragma unroll
    for (int b = 0; b < MAX_GROUP; ++b) {
      const int i = groups.members[m0 + (b < g ? b : 0)];
      y[b] = pos[2 * (size_t)i], x[b] = pos[2 * (size_t)i + 1], C[b] = model.cube + (size_t)cell[i] * cell_words;
    }
    for (int a = 0; a < g; ++a) {
      const int ia = groups.members[m0 + a];
      const double ya = pos[2 * (size_t)ia], xa = pos[2 * (size_t)ia + 1];
      const DiscBox box = disc_box(ya, xa, fit.R);
      for (long j = lane; j < box.npx; j += WALK_LANES) {
        const int r = box.r0 + (int)(j / box.bw), c = box.c0 + (int)(j % box.bw);
        const double pra = (double)r - ya, pca = (double)c - xa;
        const double qa = pra * pra + pca * pca;
        if (!(qa <= fit.R2)) continue;
        bool in[MAX_GROUP], owned = true;
#pragma unroll
        for (int b = 0; b < MAX_GROUP; ++b) {
          const double pr = (double)r - y[b], pc = (double)c - x[b];
          const double q = pr * pr + pc * pc;
          in[b] = b < g && q <= fit.R2;
          if (b < a && in[b]) owned = false;
        }
        if (!owned) continue;
        if (r < 0 || r >= fr.H || c < 0 || c >= fr.W) continue;
        const size_t p = (size_t)r * fr.W + c;
        if (!usable(fr.img, fr.mask, p)) continue;
        const double d = subtract ? (double)fr.img[p] - background_at(fr, mesh, r, c) : (double)fr.img[p];
        double m[MAX_GROUP];
#pragma unroll
        for (int b = 0; b < MAX_GROUP; ++b) m[b] = in[b] ? model_at(C[b], N, fit.h, (double)r - y[b], (double)c - x[b]) : 0.0;
        s.n += 1, s.v[G_SD] += d, s.v[G_SDD] += d * d;
#pragma unroll
        for (int b = 0; b < MAX_GROUP; ++b) {
          if (!in[b]) continue;
          s.v[G_SM + b] += m[b], s.v[G_SDM + b] += d * m[b];
#pragma unroll
          for (int c2 = b; c2 < MAX_GROUP; ++c2)
            if (in[c2]) s.v[G_A + tri(b, c2)] += m[b] * m[c2];
        }
      }
    }
  });
  s11_fold<0>(ctx, acc, acc2, st, sti), s11_fold<FOLD_BATCH>(ctx, acc, acc2, st, sti), s11_fold<2 * FOLD_BATCH>(ctx, acc, acc2, st, sti);
  static_assert(3 * FOLD_BATCH == G_FIELDS, "three batches");
  ctx.each([&](int tid) {  // the wave's first lane solves
    const int wave = tid / WALK_LANES;
    if (tid % WALK_LANES != 0) return;
    const long k = first + wave;
    sti[GI_G * WALK_WAVES + wave] = 0, sti[GI_GO * WALK_WAVES + wave] = 0, sti[GI_FLAGS * WALK_WAVES + wave] = 0;
    if (k >= groups.count) return;
    const int g = (int)(groups.starts[k + 1] - groups.starts[k]);
    double* w = st + (size_t)wave * GS_DOUBLES;
    const double* tot = w + GS_TOTALS;
    double *A = w + GS_MATRIX, *b = w + GS_RHS, *x = w + GS_X;
    const int n = sti[GI_N * WALK_WAVES + wave], p = g + fit.background;
    int flags = 0;
    if (n < p) {
      flags = FLAG_TOO_FEW;
    } else {
      for (int i = 0; i < g; ++i) {
        for (int c = i; c < g; ++c) A[i * MAX_UNKNOWNS + c] = tot[G_A + tri(i, c)];
        b[i] = tot[G_SDM + i];
        if (fit.background) A[i * MAX_UNKNOWNS + g] = tot[G_SM + i];
      }
      if (fit.background) A[g * MAX_UNKNOWNS + g] = (double)n, b[g] = tot[G_SD];
      bool solved = solve_ldl_n(p, A, b, x);
      for (int i = 0; solved && i < p; ++i) solved = finite_d(x[i]);
      if (!solved) flags = FLAG_DEGENERATE;
    }
    w[GS_BG] = flags ? std::nan("") : fit.background ? x[g] : 0.0;
    sti[GI_G * WALK_WAVES + wave] = g, sti[GI_FLAGS * WALK_WAVES + wave] = flags, sti[GI_GO * WALK_WAVES + wave] = flags == 0;
  });
  int g_max = 0;
  for (int w = 0; w < WALK_WAVES; ++w) g_max = sti[GI_G * WALK_WAVES + w] > g_max ? sti[GI_G * WALK_WAVES + w] : g_max;
  for (int a = 0; a < g_max; ++a) {  // pass 2, member a of every wave's group
    ctx.each([&](int tid) {
      const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
      Lane& keep = ctx.regs(tid);
      if (a == 0) keep.v[0] = keep.v[1] = 0.0;
      const int g = sti[GI_G * WALK_WAVES + wave];
      if (a >= g) return;
      const bool go = sti[GI_GO * WALK_WAVES + wave] != 0;
      const double* w = st + (size_t)wave * GS_DOUBLES;
      const double bg = w[GS_BG];
      const int* members = groups.members + groups.starts[first + wave];
      const int ia = members[a];
      const double y = pos[2 * (size_t)ia], x = pos[2 * (size_t)ia + 1];
      const double* C = model.cube + (size_t)cell[ia] * cell_words;
      double s[F_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      int n_use = 0, n_all = 0;
      double chi2 = 0.0, abs_res = 0.0, gchi2 = keep.v[0], gabs = keep.v[1];
      Peak seen{0.0, -1};
      double m = 0.0;
      walk_disc(
          fr, disc_box(y, x, fit.R), y, x, fit.R2, lane,
          [&](double pr, double pc) {
            ++n_all;
            m = model_at(C, N, fit.h, pr, pc), s[F_SM_ALL] += m;
          },
          [&](int r, int c, size_t p, double, double, double) {
            ++n_use;
            const double d = subtract ? (double)fr.img[p] - background_at(fr, mesh, r, c) : (double)fr.img[p];
            UniformWeights::add(s, {}, m, d);  // S8's own sums
            if (!go) return;
            double S = 0.0;
            bool owned = true;
            for (int b = 0; b < g; ++b) {
              if (b == a) {
                S += w[GS_X + b] * m;
                continue;
              }
              const int ib = members[b];
              const double prb = (double)r - pos[2 * (size_t)ib], pcb = (double)c - pos[2 * (size_t)ib + 1];
              const double qb = prb * prb + pcb * pcb;
              if (!(qb <= fit.R2)) continue;
              S += w[GS_X + b] * model_at(model.cube + (size_t)cell[ib] * cell_words, N, fit.h, prb, pcb);
              if (b < a) owned = false;
            }
            const double e = d - (S + bg);
            chi2 += e * e, abs_res += std::fabs(e);
            see_residual(seen, e, (long long)p);
            if (owned) gchi2 += e * e, gabs += std::fabs(e);
          });
      keep.v[0] = gchi2, keep.v[1] = gabs;
#pragma unroll
      for (int f = 0; f < F_SUMS; ++f) acc.d[f * WALK_THREADS + tid] = s[f];
      acc.d[M_CHI2 * WALK_THREADS + tid] = chi2, acc.d[M_ABS * WALK_THREADS + tid] = abs_res;
      acc.d[M_PEAK * WALK_THREADS + tid] = seen.e, acc.at[tid] = seen.at;
      acc.cnt[tid] = n_use, acc.cnt[WALK_THREADS + tid] = n_all;
    });
    ctx.each([&](int tid) {  // 64 partials to 8
      const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
      if (lane >= 8 || a >= sti[GI_G * WALK_WAVES + wave]) return;
      fold_sums_64to8(acc, acc2, tid, M_PEAK), fold_counts_64to8(acc, acc2, tid, 2), fold_peak_64to8(acc, acc2, tid, M_PEAK);
    });
    ctx.each([&](int tid) {  // 8 to 1, and member a's row
      const int wave = tid / WALK_LANES;
      const int g = sti[GI_G * WALK_WAVES + wave];
      if (tid % WALK_LANES != 0 || a >= g) return;
      const int flags = sti[GI_FLAGS * WALK_WAVES + wave];
      const double* w = st + (size_t)wave * GS_DOUBLES;
      const long long m0 = groups.starts[first + wave];
      const int ia = groups.members[m0 + a];
      double* o = out + (size_t)GROUP_COLUMNS * (size_t)(m0 + a);
      double s[M_PEAK];
      int cnt[2];
      fold_sums_8to1(acc2, wave, M_PEAK, s), fold_counts_8to1(acc2, wave, 2, cnt);
      const Peak seen = fold_peak_8to1(acc2, wave, M_PEAK);
      const double nan = std::nan("");
      o[COL_FY] = pos[2 * (size_t)ia], o[COL_FX] = pos[2 * (size_t)ia + 1], o[COL_CELL] = (double)cell[ia], o[COL_FFLAGS] = (double)flags;
      o[COL_N] = (double)cnt[0], o[COL_NALL] = (double)cnt[1];
      for (int c = 0; c < F_SUMS; ++c) o[COL_FSUMS + c] = s[c];
      o[COL_GROUP] = (double)groups.members[m0], o[COL_GROUP_SIZE] = (double)g, o[COL_GROUP_N] = (double)sti[GI_N * WALK_WAVES + wave];
      if (flags == 0) {
        o[COL_F] = w[GS_X + a], o[COL_BG] = w[GS_BG], o[COL_CHI2] = s[M_CHI2], o[COL_ABS_RES] = s[M_ABS];
      } else {
        o[COL_F] = o[COL_BG] = o[COL_CHI2] = o[COL_ABS_RES] = nan;
        o[COL_GROUP_CHI2] = o[COL_GROUP_ABS] = nan;
      }
      if (flags == 0 && seen.at >= 0) {
        o[COL_PEAK_RES] = std::fabs(seen.e), o[COL_PEAK_E] = seen.e;
        o[COL_PEAK_ROW] = (double)(seen.at / fr.W), o[COL_PEAK_COL] = (double)(seen.at % fr.W);
      } else {
        o[COL_PEAK_RES] = o[COL_PEAK_E] = nan;
        o[COL_PEAK_ROW] = o[COL_PEAK_COL] = -1.0;
      }
    });
  }
  ctx.each([&](int tid) {  // the group's residual: the lanes' running sums fold once
    const Lane& keep = ctx.regs(tid);
    acc.d[0 * WALK_THREADS + tid] = keep.v[0], acc.d[1 * WALK_THREADS + tid] = keep.v[1];
  });
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
    if (lane >= 8 || !sti[GI_GO * WALK_WAVES + wave]) return;
    fold_sums_64to8(acc, acc2, tid, 2);
  });
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES;
    if (tid % WALK_LANES != 0 || !sti[GI_GO * WALK_WAVES + wave]) return;
    double v[2];
    fold_sums_8to1(acc2, wave, 2, v);
    const long long m0 = groups.starts[first + wave];
    for (int a = 0; a < sti[GI_G * WALK_WAVES + wave]; ++a) {
      double* o = out + (size_t)GROUP_COLUMNS * (size_t)(m0 + a);
      o[COL_GROUP_CHI2] = v[0], o[COL_GROUP_ABS] = v[1];
    }
  });
}

}  // namespace rpsfj
