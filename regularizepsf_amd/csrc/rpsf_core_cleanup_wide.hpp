// rpsf_core_cleanup_wide.hpp - kernel B3w of the PSF builder (csrc/builder.hip): kernel B3 (rpsf_core_cleanup.hpp) at the wide sizes
// 129 <= N <= 256, shared with the CPU lane emulator tests/emu/emu_cleanup_wide.cpp.  The definition is DESIGN.md 3.6 steps 1-7
// (builder.clean_cell), float64 throughout, one workgroup of 1024 threads per cell; the driver runs over the same kind of context as
// B3's (`ctx.each(f)`: f(tid) for every thread, then a barrier) but keeps nothing in registers between two each() calls.
//
// Storage.  A thread owns pixels tid, tid + 1024, ... (up to 64 of them): their values cannot stay in registers.
//   - The cell is read where it lies in global memory, as often as it is needed.  p = c - (a col + b row + d) is ONE expression
//     (plane_subtracted below), recomputed from c and the three coefficients wherever p is needed: the same bits every time.
//   - The two byte masks are B3's, reused from step to step the same way, in LDS: 2 x 64 KiB + 64 B = 128.1 KiB at N = 256.
//   - The 32-bit union-find parents (256 KiB) and the partial sums of the reductions (1104 records of 40 B) lie in the workgroup's
//     SLOT of a workspace in global memory: slot_bytes(256) = 299.1 KiB.  The two do not share bytes.  The slots are those of
//     kernel B1w's workspace (rpsfbw::slots_for(N) of them, each at least as large from N = 61 on), which a handle owns once.
//     uf_find / uf_unite of rpsf_core_stars.hpp work on the global pointer; the only atomics are their integer atomicMin, whose
//     result (the smallest index of a component) does not depend on the order.
// Sums run in ONE fixed order, B3's (rpsfc::reduce): per thread over its pixels in index order (tid, tid + 1024, ...), then groups of
// 16 partial sums in index order (1024 -> 64 -> 4), and the last 4 folded in index order by every thread.  Nothing in it depends on
// the slot, on the other cells of the launch or on the order in which threads run.
#pragma once
#include "rpsf_core_builder_wide.hpp"  // slots_for
#include "rpsf_core_cleanup.hpp"

#pragma clang fp contract(off)

namespace rpsfcw {

using rpsfc::CLEANED;
using rpsfc::DEGENERATE_RING;
using rpsfc::dilate;
using rpsfc::erode;
using rpsfc::own_indices;
using rpsfc::Sums;

constexpr int MIN_N = rpsfb::MAX_N + 1, MAX_N = 256;
constexpr int EMU_MIN_N = rpsfb::MIN_N;  // the driver itself takes any size
constexpr int THREADS = 1024;
using rpsfbw::slots_for;

RPSFC_HD size_t mask_bytes(int N) { return ((size_t)N * N + 7) / 8 * 8; }
RPSFC_HD size_t lds_bytes(int N) { return 8 * sizeof(double) + 2 * mask_bytes(N); }
RPSFC_HD size_t parent_bytes(int N) { return ((size_t)N * N * sizeof(int) + 7) / 8 * 8; }
RPSFC_HD size_t slot_bytes(int N) { return parent_bytes(N) + (size_t)(THREADS + THREADS / 16 + 16) * sizeof(Sums); }

struct Wide {
  int* parent;  // [N * N], global
  Sums* part;   // after them, global
  int* any;     // LDS: a pixel of the cell is not zero
  uint8_t* a;   // LDS: nz -> low -> core
  uint8_t* b;   // LDS: inner -> non-zero pixels of p
};
RPSFC_HD Wide carve(void* lds, void* slot, int N) {
  Wide s;
  s.parent = static_cast<int*>(slot);
  s.part = reinterpret_cast<Sums*>(static_cast<char*>(slot) + parent_bytes(N));
  s.any = static_cast<int*>(lds);
  s.a = static_cast<uint8_t*>(lds) + 8 * sizeof(double);
  s.b = s.a + mask_bytes(N);
  return s;
}

struct Plane {
  double a, b, d;
};
// step 3's p at pixel `p` of a cell with value c there
RPSFC_HD double plane_subtracted(double c, int p, int N, const Plane& f) { return c - (f.a * (double)(p % N) + f.b * (double)(p / N) + f.d); }
// ... and whether it is a finite non-zero number of a non-zero pixel (everything else ends as 0)
RPSFC_HD bool kept(double c, double v) { return c != 0.0 && v != 0.0 && std::fabs(v) <= 1.79769313486231570815e308; }

// One cell: in, out N x N float64 (in is finite), *flag CLEANED or DEGENERATE_RING; a cell with DEGENERATE_RING leaves as it came.
// THREADS threads run it; `lds` holds lds_bytes(N), `slot` slot_bytes(N).  The steps are numbered as in DESIGN.md 3.6.
template <class Ctx>
RPSFC_HD void clean_cell_wide(Ctx& ctx, int N, const double* in, double* out, uint8_t* flag, void* lds, void* slot) {
  const int T = THREADS, NN = N * N, ctr = (N / 2) * N + N / 2;
  const Wide s = carve(lds, slot, N);
  const double nan = std::nan("");

  ctx.each([&](int tid) {
    if (tid == 0) *s.any = 0;
  });
  // step 1: nz
  ctx.each([&](int tid) {
    bool any = false;
    own_indices(tid, T, NN, [&](int p) {
      const bool nz = in[p] != 0.0;
      s.a[p] = nz;
      any = any || nz;
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
  // ring (recomputed from `inner` by whoever needs it: the mask is not written again before step 5), and step 2: the plane through it
  const double centre_value = in[ctr];
  const auto in_ring = [&](int p) { return !s.b[p] & dilate(s.b, N, p / N, p % N) & (in[p] < centre_value); };
  const Sums first = rpsfc::reduce(ctx, T, s.part, [&](int tid) {
    Sums t{{0.0, 0.0, 0.0, 0.0, 0.0}};
    own_indices(tid, T, NN, [&](int p) {
      if (in_ring(p)) t.s[0] += 1.0, t.s[1] += (double)(p % N), t.s[2] += (double)(p / N), t.s[3] += in[p];
    });
    return t;
  });
  const double n = first.s[0];
  bool degenerate = n < 3.0;
  Plane f{0.0, 0.0, 0.0};
  if (!degenerate) {
    const double mx = first.s[1] / n, my = first.s[2] / n, mv = first.s[3] / n;
    const Sums second = rpsfc::reduce(ctx, T, s.part, [&](int tid) {
      Sums t{{0.0, 0.0, 0.0, 0.0, 0.0}};
      own_indices(tid, T, NN, [&](int p) {
        if (!in_ring(p)) return;
        const double dx = (double)(p % N) - mx, dy = (double)(p / N) - my, dv = in[p] - mv;
        t.s[0] += dx * dx, t.s[1] += dx * dy, t.s[2] += dy * dy, t.s[3] += dx * dv, t.s[4] += dy * dv;
      });
      return t;
    });
    const double sxx = second.s[0], sxy = second.s[1], syy = second.s[2], sxv = second.s[3], syv = second.s[4];
    const double det = sxx * syy - sxy * sxy;
    if (!(det > 1e-9 * sxx * syy)) {  // det = sxx syy (1 - rho^2): zero when the pixels share a row, a column or a diagonal
      degenerate = true;
    } else {
      f.a = (sxv * syy - syv * sxy) / det, f.b = (syv * sxx - sxv * sxy) / det;
      f.d = mv - f.a * mx - f.b * my;
    }
  }
  if (degenerate) {  // SciPy's minimum-norm answer is the caller's business: it gets the cell back
    ctx.each([&](int tid) {
      own_indices(tid, T, NN, [&](int p) { out[p] = in[p]; });
      if (tid == 0) *flag = DEGENERATE_RING;
    });
    return;
  }
  // step 3: p = c - plane; not a number where c is zero or p is zero (or not finite: it ends as 0 either way).
  // step 4: below 0.5 % of the centre (a NaN centre: nothing is)
  const double centre_p = plane_subtracted(in[ctr], ctr, N, f);
  const double cut = 0.005 * (kept(in[ctr], centre_p) ? centre_p : nan);
  ctx.each([&](int tid) {
    own_indices(tid, T, NN, [&](int p) {
      const double c = in[p], v = plane_subtracted(c, p, N, f);
      s.a[p] = kept(c, v) && v < cut;
    });
  });
  // drop what lies inside `low`; what is left and is a number is the non-zero set of p.  Step 5: every such pixel its own root
  ctx.each([&](int tid) {
    own_indices(tid, T, NN, [&](int p) {
      const double c = in[p], v = plane_subtracted(c, p, N, f);
      const bool keep = kept(c, v) && !erode(s.a, N, p / N, p % N, true);
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
  const auto final_value = [&](int p) {
    const double v = s.b[p] ? plane_subtracted(in[p], p, N, f) : 0.0;
    return v * (dilate(s.a, N, p / N, p % N) ? 1.0 : 0.0);
  };
  const Sums total = rpsfc::reduce(ctx, T, s.part, [&](int tid) {
    Sums t{{0.0, 0.0, 0.0, 0.0, 0.0}};
    own_indices(tid, T, NN, [&](int p) { t.s[0] += final_value(p); });
    return t;
  });
  ctx.each([&](int tid) {
    own_indices(tid, T, NN, [&](int p) { out[p] = final_value(p) / total.s[0]; });
    if (tid == 0) *flag = CLEANED;
  });
}

}  // namespace rpsfcw
