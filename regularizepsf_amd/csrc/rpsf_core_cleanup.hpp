// rpsf_core_cleanup.hpp - kernel B3 of the PSF builder (csrc/builder.hip), shared with the CPU lane emulator
// tests/emu/emu_cleanup.cpp: the per-cell clean-up of regularizepsf/builder.py:231-260 (builder.clean_cell of this package), one
// workgroup per averaged cell, float64 throughout.
//
// The kernel is a DRIVER over a context, as the star finder's are (rpsf_core_stars.hpp): `ctx.each(f)` runs f(tid) for every thread
// of the workgroup and then a barrier; `ctx.regs(tid)` is what thread tid keeps in registers between two each() calls.  Everything
// else the driver keeps between two each() calls is computed from words all threads read alike.
//
// A thread owns pixels tid, tid + T, ... (at most MAX_PPT) and keeps their VALUES in registers, read once from global memory:
// neighbours only ever read masks and labels, which live in LDS - two byte masks that are reused from step to step and one 32-bit
// word per pixel that holds the union-find parents and, before and after the labelling, the partial sums of the reductions.
//   N = 128: 64 KiB + 2 x 16 KiB + 64 B = 96.1 KiB of the 160 KiB.
// Sums run in one fixed order: per thread over its pixels in index order, then groups of 16 partial sums in index order until at
// most 16 are left, which every thread folds in index order.  The only atomics are the integer atomicMin of the union-find.
#pragma once
#include <cmath>
#include <cstdint>

#include "rpsf_core_builder.hpp"  // MIN_N, MAX_N, MAX_PPT, threads_for
#include "rpsf_core_stars.hpp"    // uf_find, uf_unite

#if defined(__HIPCC__)
#define RPSFC_HD __host__ __device__ __forceinline__
#else
#define RPSFC_HD inline
#endif

// compared with the float64 SciPy / NumPy clean-up at 1e-12, and bit for bit between the GPU and the emulator
#pragma clang fp contract(off)

namespace rpsfc {

using rpsfb::MAX_PPT;
using rpsfb::threads_for;

// flags of a cell after B3
constexpr uint8_t CLEANED = 0, DEGENERATE_RING = 1;

struct Regs {  // one thread's registers
  double v[MAX_PPT];  // the cell's values, later p of the definition
  unsigned ring;      // bit k: pixel k of the thread is in the fit mask
  unsigned keep;      // bit k: p is a finite non-zero number (everything else ends as 0)
};
struct Sums {
  double s[5];
};

RPSFC_HD size_t work_bytes(int N) {  // union-find parents, or the partial sums of a reduction: T, then T / 16, then at most 16 more
  const int T = threads_for(N);
  const size_t labels = (size_t)N * N * sizeof(int), sums = (size_t)(T + T / 16 + 16) * sizeof(Sums);
  return ((labels > sums ? labels : sums) + 7) / 8 * 8;
}
RPSFC_HD size_t mask_bytes(int N) { return ((size_t)N * N + 7) / 8 * 8; }
RPSFC_HD size_t lds_bytes(int N) { return work_bytes(N) + 8 * sizeof(double) + 2 * mask_bytes(N); }

struct Lds {
  int* parent;    // [N * N]
  Sums* part;     // the same bytes
  double* share;  // [0] p at the centre (NaN: none)
  int* any;       // the last of the 8 doubles: a pixel of the cell is not zero
  uint8_t* a;     // nz -> low -> core
  uint8_t* b;     // inner -> non-zero pixels of p
};
RPSFC_HD Lds carve(void* base, int N) {
  Lds s;
  char* at = static_cast<char*>(base);
  s.parent = reinterpret_cast<int*>(at);
  s.part = reinterpret_cast<Sums*>(at);
  s.share = reinterpret_cast<double*>(at + work_bytes(N));
  s.any = reinterpret_cast<int*>(s.share + 7);
  s.a = reinterpret_cast<uint8_t*>(s.share + 8);
  s.b = s.a + mask_bytes(N);
  return s;
}

// f(k, p) for the thread's pixels in index order: unrolled, so that v[k] is a register
template <class F>
RPSFC_HD void own_pixels(int tid, int T, int NN, F&& f) {
#pragma unroll
  for (int k = 0; k < MAX_PPT; ++k) {
    const int p = tid + k * T;
    if (p < NN) f(k, p);
  }
}
// f(p) for the same pixels where no register is indexed: a loop
template <class F>
RPSFC_HD void own_indices(int tid, int T, int NN, F&& f) {
#pragma unroll 1
  for (int p = tid; p < NN; p += T) f(p);
}

// binary erosion / dilation by the cross (the pixel and its 4-neighbourhood) at pixel (r, c) of a mask of 0 / 1 bytes; pixels outside
// the cell count as `outside`.  Every load is unconditional (a neighbour outside the cell reads the pixel itself): no divergence.
RPSFC_HD unsigned cross(const uint8_t* m, int N, int r, int c, unsigned outside, bool all) {
  const int p = r * N + c;
  const bool cl = c > 0, cr = c < N - 1, ru = r > 0, rd = r < N - 1;
  const unsigned here = m[p], left = m[cl ? p - 1 : p], right = m[cr ? p + 1 : p], up = m[ru ? p - N : p], down = m[rd ? p + N : p];
  const unsigned l = cl ? left : outside, rt = cr ? right : outside, u = ru ? up : outside, d = rd ? down : outside;
  return all ? (here & l & rt & u & d) : (here | l | rt | u | d);
}
RPSFC_HD bool erode(const uint8_t* m, int N, int r, int c, bool outside) { return cross(m, N, r, c, outside ? 1u : 0u, true) != 0; }
RPSFC_HD bool dilate(const uint8_t* m, int N, int r, int c) { return cross(m, N, r, c, 0u, false) != 0; }  // outside = 0

RPSFC_HD Sums fold(const Sums* from, int count) {  // in index order
  Sums r{{0.0, 0.0, 0.0, 0.0, 0.0}};
  for (int j = 0; j < count; ++j)
    for (int m = 0; m < 5; ++m) r.s[m] += from[j].s[m];
  return r;
}
// partial(tid) of every thread, summed: T partial sums, groups of 16 of them until at most 16 are left, those folded by everybody.
// What is returned is read before the barrier of the next each(); the words it is read from are not written again before the
// SECOND each() of the next reduction (T = 256) or its third (T = 1024).
template <class Ctx, class F>
RPSFC_HD Sums reduce(Ctx& ctx, int T, Sums* part, F&& partial) {
  ctx.each([&](int tid) { part[tid] = partial(tid); });
  Sums* from = part;
  int count = T;
  while (count > 16) {
    Sums* to = from + count;
    ctx.each([&](int tid) {
      if (tid < count / 16) to[tid] = fold(from + 16 * tid, 16);
    });
    from = to, count /= 16;
  }
  return fold(from, count);
}

// One cell: in, out N x N float64 (in is finite), *flag CLEANED or DEGENERATE_RING; a cell with DEGENERATE_RING leaves as it came.
// T = threads_for(N) threads run it (a parameter, so that the kernel can make it a constant); `lds` holds lds_bytes(N).
// The steps are numbered as in DESIGN.md 3.6.
template <class Ctx>
RPSFC_HD void clean_cell(Ctx& ctx, int N, int T, const double* in, double* out, uint8_t* flag, void* lds) {
  const int NN = N * N, ctr = (N / 2) * N + N / 2;
  const Lds s = carve(lds, N);
  const double nan = std::nan("");

  ctx.each([&](int tid) {
    if (tid == 0) *s.any = 0;
  });
  // step 1: nz
  ctx.each([&](int tid) {
    Regs& g = ctx.regs(tid);
    bool any = false;
    own_pixels(tid, T, NN, [&](int k, int p) {
      g.v[k] = in[p];
      s.a[p] = g.v[k] != 0.0;
      any = any || g.v[k] != 0.0;
    });
    if (any) *s.any = 1;  // everybody who stores, stores the same
  });
  if (!*s.any) {  // a cell without a star: 0 / 0 everywhere
    ctx.each([&](int tid) {
      own_indices(tid, T, NN, [&](int p) { out[p] = nan; });
      if (tid == 0) *flag = CLEANED;
    });
    return;
  }
  // inner
  ctx.each([&](int tid) {
    own_indices(tid, T, NN, [&](int p) {
      const int r = p / N, c = p % N;
      s.b[p] = (r > 0) & (r < N - 1) & (c > 0) & (c < N - 1) & erode(s.a, N, r, c, false);
    });
  });
  // ring, and step 2: the plane through it, with centred coordinates as B1 fits its own (rpsf_core_builder.hpp, phase 4b)
  const double centre_value = in[ctr];
  const Sums first = reduce(ctx, T, s.part, [&](int tid) {
    Regs& g = ctx.regs(tid);
    g.ring = 0;
    Sums t{{0.0, 0.0, 0.0, 0.0, 0.0}};
    own_pixels(tid, T, NN, [&](int k, int p) {
      const int r = p / N, c = p % N;
      if (!s.b[p] & dilate(s.b, N, r, c) & (g.v[k] < centre_value)) {
        g.ring |= 1u << k;
        t.s[0] += 1.0, t.s[1] += (double)c, t.s[2] += (double)r, t.s[3] += g.v[k];
      }
    });
    return t;
  });
  const double n = first.s[0];
  bool degenerate = n < 3.0;
  double pa = 0.0, pb = 0.0, pd = 0.0;
  if (!degenerate) {
    const double mx = first.s[1] / n, my = first.s[2] / n, mv = first.s[3] / n;
    const Sums second = reduce(ctx, T, s.part, [&](int tid) {
      const Regs& g = ctx.regs(tid);
      Sums t{{0.0, 0.0, 0.0, 0.0, 0.0}};
      own_pixels(tid, T, NN, [&](int k, int p) {
        if (!((g.ring >> k) & 1u)) return;
        const double dx = (double)(p % N) - mx, dy = (double)(p / N) - my, dv = g.v[k] - mv;
        t.s[0] += dx * dx, t.s[1] += dx * dy, t.s[2] += dy * dy, t.s[3] += dx * dv, t.s[4] += dy * dv;
      });
      return t;
    });
    const double sxx = second.s[0], sxy = second.s[1], syy = second.s[2], sxv = second.s[3], syv = second.s[4];
    const double det = sxx * syy - sxy * sxy;
    if (!(det > 1e-9 * sxx * syy)) {  // det = sxx syy (1 - rho^2): zero when the pixels share a row, a column or a diagonal
      degenerate = true;
    } else {
      pa = (sxv * syy - syv * sxy) / det, pb = (syv * sxx - sxv * sxy) / det;
      pd = mv - pa * mx - pb * my;
    }
  }
  if (degenerate) {  // SciPy's minimum-norm answer is the caller's business: it gets the cell back
    ctx.each([&](int tid) {
      const Regs& g = ctx.regs(tid);
      own_pixels(tid, T, NN, [&](int k, int p) { out[p] = g.v[k]; });
      if (tid == 0) *flag = DEGENERATE_RING;
    });
    return;
  }
  // step 3: p = c - plane; not a number where c is zero or p is zero (or not finite: it ends as 0 either way)
  ctx.each([&](int tid) {
    Regs& g = ctx.regs(tid);
    g.keep = 0;
    own_pixels(tid, T, NN, [&](int k, int p) {
      const double c = g.v[k];
      const double v = c - (pa * (double)(p % N) + pb * (double)(p / N) + pd);
      const bool keep = c != 0.0 && v != 0.0 && std::fabs(v) <= 1.79769313486231570815e308;
      g.v[k] = v;
      if (keep) g.keep |= 1u << k;
      if (p == ctr) s.share[0] = keep ? v : nan;
    });
  });
  // step 4: below 0.5 % of the centre (a NaN centre: nothing is)
  const double cut = 0.005 * s.share[0];
  ctx.each([&](int tid) {
    const Regs& g = ctx.regs(tid);
    own_pixels(tid, T, NN, [&](int k, int p) { s.a[p] = ((g.keep >> k) & 1u) && g.v[k] < cut; });
  });
  // drop what lies inside `low`; what is left and is a number is the non-zero set of p.  Step 5: every such pixel its own root
  ctx.each([&](int tid) {
    Regs& g = ctx.regs(tid);
    own_pixels(tid, T, NN, [&](int k, int p) {
      if (erode(s.a, N, p / N, p % N, true)) g.keep &= ~(1u << k);
      const bool keep = (g.keep >> k) & 1u;
      if (!keep) g.v[k] = 0.0;
      s.b[p] = keep;
      s.parent[p] = keep ? p : -1;
    });
  });
  // 4-connectivity: links to the left and to the upper neighbour.  Parent <= child throughout (rpsf_core_stars.hpp, S3), so every
  // loop of uf_find / uf_unite ends whatever the other threads do, and a root is the smallest index of its component.
  ctx.each([&](int tid) {
    own_indices(tid, T, NN, [&](int p) {
      if (!s.b[p]) return;
      if (p % N > 0 && s.b[p - 1]) rpsfs::uf_unite(s.parent, p, p - 1);
      if (p >= N && s.b[p - N]) rpsfs::uf_unite(s.parent, p, p - N);
    });
  });
  // core: the centre's component - or, with a zero centre, the background: all zero pixels (scipy.ndimage.label gives them label 0)
  const int centre_root = s.b[ctr] ? rpsfs::uf_find(s.parent, ctr) : -1;
  ctx.each([&](int tid) {
    own_indices(tid, T, NN, [&](int p) {
      s.a[p] = centre_root < 0 ? !s.b[p] : (s.b[p] && rpsfs::uf_find(s.parent, p) == centre_root);
    });
  });
  // p * dilate(core), and step 6: its sum
  const Sums total = reduce(ctx, T, s.part, [&](int tid) {
    Regs& g = ctx.regs(tid);
    Sums t{{0.0, 0.0, 0.0, 0.0, 0.0}};
    own_pixels(tid, T, NN, [&](int k, int p) {
      g.v[k] = g.v[k] * (dilate(s.a, N, p / N, p % N) ? 1.0 : 0.0);
      t.s[0] += g.v[k];
    });
    return t;
  });
  ctx.each([&](int tid) {
    const Regs& g = ctx.regs(tid);
    own_pixels(tid, T, NN, [&](int k, int p) { out[p] = g.v[k] / total.s[0]; });
    if (tid == 0) *flag = CLEANED;
  });
}

}  // namespace rpsfc
