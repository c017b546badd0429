// rpsf_core_builder_wide.hpp - per-thread phases of kernel B1w (csrc/builder.hip), kernel B1 at the wide sizes 129 <= N <= 256, shared
// with the CPU lane emulator tests/emu/emu_builder_wide.cpp.  As in rpsf_core_builder.hpp every function does the work of ONE thread
// of a workgroup between two barriers, on plain pointers.
//
// The arithmetic is B1's, operation for operation and in the same order: b1_tables, b1_gather, b1_scan, b1_finish and b1_verdict
// are B1's own functions, called on an rpsfb::Lds whose `patch` points at a slab in global memory; the prefilter, the taps and the
// plane are restated here because of where the patch lives, and only for that (tests/test_builder_wide_host.py pins that the
// restatement gives B1's bits at N = 64 and 128).
//
// Storage.  A float64 patch of 256 x 257 is 514 KiB: it does not fit LDS (160 KiB).  The workgroup (1024 threads) owns one SLOT of a
// workspace in global memory: two slabs A and B of N x ld doubles each (ld = N | 1, as in B1), resident in L2 while the star is
// worked on.  LDS holds what is small and read by everybody: the tap tables, the border ring of the shifted patch (4 N + 1 doubles,
// staged for the one thread that fits the plane), the plane and the three flag words.
//   N = 256: LDS 16 KiB + 8 KiB + 8 KiB + 128 B = 32.2 KiB; a slot is 2 x 514 KiB = 1028 KiB.
// The workspace holds slots_for(N) slots: one per compute unit of the MI355X (256) where they fit WORKSPACE_MAX = 256 MiB, which is up
// to N = 255; at N = 256, 255 slots (255.996 MiB).
// A slab holds the patch either as it is, element (r, c) at r * ld + c, or TRANSPOSED, (r, c) at c * ld + r: a phase that walks lines
// (the prefilter) always gets the layout in which the lanes of a wave hold adjacent lines, so that every load of a wave is one
// contiguous run of doubles.
//   gather            -> A as it is
//   prefilter axis 0     A in place          lane = column, walking down the rows
//   transpose         A -> B transposed
//   prefilter axis 1     B in place          lane = row, walking along the columns (down the rows of the transposed slab)
//   taps axis 0       B -> A transposed      out of place: nobody reads what anybody writes
//   taps axis 1       A -> B as it is        likewise
//   scan, ring, plane, finish on B
// The prefilter walks its line in chunks of CHUNK samples: the loads of a chunk are independent (issued together), the recurrence
// runs in registers, the stores follow - a line costs 3 N / CHUNK round trips to L2 and not 5 N.  The gain is not stored by a pass of
// its own: c[i] * gain is one correctly rounded product wherever it is formed, so forming it where it is used gives B1's bits.
#pragma once
#include "rpsf_core_builder.hpp"

#pragma clang fp contract(off)

namespace rpsfbw {

using rpsfb::ld_for;
using rpsfb::Lds;
using rpsfb::POLE;

constexpr int MIN_N = rpsfb::MAX_N + 1, MAX_N = 256;  // the wide sizes
constexpr int EMU_MIN_N = rpsfb::MIN_N;                // the phases themselves take any size (the emulator runs them at B1's)
constexpr int THREADS = 1024;
constexpr int MAX_SLOTS = 256;
constexpr size_t WORKSPACE_MAX = (size_t)256 << 20;
constexpr int CHUNK = 8;

RPSFB_HD size_t slab_doubles(int N) { return (size_t)N * ld_for(N); }
RPSFB_HD size_t slot_doubles(int N) { return 2 * slab_doubles(N); }
RPSFB_HD int slots_for(int N) {
  const size_t fit = WORKSPACE_MAX / (slot_doubles(N) * sizeof(double));
  return fit < (size_t)MAX_SLOTS ? (int)fit : MAX_SLOTS;
}
// LDS of one B1w workgroup: per axis and output index 4 tap weights, the ring (top row, bottom row, left column, right column, N each,
// then the centre, padded to 8), the plane, then the tap indices and the flags
RPSFB_HD size_t lds_bytes(int N) { return (size_t)(2 * 4 * N + 4 * N + 8 + 8) * sizeof(double) + (size_t)(2 * 4 * N + 8) * sizeof(int); }

struct Wide {
  Lds s;         // w, plane, tap, flag in LDS; patch is set to the slab a phase works on
  double* ring;  // [4][N], then the centre
  double *a, *b;
};
RPSFB_HD Wide carve(void* lds, double* slot, int N) {
  Wide q;
  q.s.w = static_cast<double*>(lds);
  q.ring = q.s.w + 2 * 4 * N;
  q.s.plane = q.ring + 4 * N + 8;
  q.s.tap = reinterpret_cast<int*>(q.s.plane + 8);
  q.s.flag = q.s.tap + 2 * 4 * N;
  q.a = slot, q.b = slot + slab_doubles(N);
  q.s.patch = q.a;
  return q;
}
RPSFB_HD Lds on(const Wide& q, double* slab) {
  Lds s = q.s;
  s.patch = slab;
  return s;
}

// b1_prefilter for line `tid` of a slab whose lines run down the rows (stride ld): c[i] is at slab[i * ld + tid]
RPSFB_HD void b1w_prefilter(int tid, int N, double* slab) {
  if (tid >= N) return;
  const long st = ld_for(N);
  double* c = slab + tid;
  const double z = POLE;
  const double gain = (1.0 - z) * (1.0 - 1.0 / z);
  double z_n_1 = 1.0;
  for (int i = 0; i < N - 1; ++i) z_n_1 *= z;
  double lo[CHUNK], hi[CHUNK];
  // _init_causal_mirror on the samples times the gain
  double z_i = z;
  double c0 = c[0] * gain + z_n_1 * (c[(long)(N - 1) * st] * gain);
  for (int base = 1; base < N - 1; base += CHUNK) {
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) {
      const int i = base + k;
      if (i < N - 1) lo[k] = c[i * st], hi[k] = c[(N - 1 - i) * st];
    }
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) {
      const int i = base + k;
      if (i < N - 1) {
        c0 += z_i * (lo[k] * gain + z_n_1 * (hi[k] * gain));
        z_i *= z;
      }
    }
  }
  // the causal pass
  double prev = c0 / (1.0 - z_n_1 * z_n_1);
  c[0] = prev;
  for (int base = 1; base < N; base += CHUNK) {
#pragma unroll
    for (int k = 0; k < CHUNK; ++k)
      if (base + k < N) lo[k] = c[(base + k) * st];
#pragma unroll
    for (int k = 0; k < CHUNK; ++k)
      if (base + k < N) lo[k] = prev = lo[k] * gain + z * prev;
#pragma unroll
    for (int k = 0; k < CHUNK; ++k)
      if (base + k < N) c[(base + k) * st] = lo[k];
  }
  // _init_anticausal_mirror (prev is c[N - 1] of the causal pass, c[N - 2] is read back) and the anticausal pass
  prev = (z * c[(long)(N - 2) * st] + prev) * z / (z * z - 1.0);
  c[(long)(N - 1) * st] = prev;
  for (int base = N - 2; base >= 0; base -= CHUNK) {
#pragma unroll
    for (int k = 0; k < CHUNK; ++k)
      if (base - k >= 0) lo[k] = c[(base - k) * st];
#pragma unroll
    for (int k = 0; k < CHUNK; ++k)
      if (base - k >= 0) lo[k] = prev = z * (prev - lo[k]);
#pragma unroll
    for (int k = 0; k < CHUNK; ++k)
      if (base - k >= 0) c[(base - k) * st] = lo[k];
  }
}

// from[r * ld + c] -> to[c * ld + r].  Lanes run along c: the loads are contiguous, the stores one cache line per lane.
RPSFB_HD void b1w_transpose(int tid, int nthreads, int N, const double* from, double* to) {
  const int ld = ld_for(N);
  for (int p = tid; p < N * N; p += nthreads) {
    const int r = p / N, c = p % N;
    to[c * ld + r] = from[r * ld + c];
  }
}

// b1_taps_read and b1_taps_write as one pass out of place: the 4 taps along `axis` of every pixel of the thread.  Element (r, c) of
// `in` is at r * irs + c * ics, of `out` at r * ors + c * ocs.  The lanes of a wave run along r (pixel p is (p % N, p / N)): both
// transposed slabs are then read and written in contiguous runs, and the one slab that leaves as it is is written a line per lane.
RPSFB_HD void b1w_taps(int tid, int nthreads, int N, int axis, const Lds& s, const double* in, int irs, int ics, double* out, int ors,
                       int ocs) {
  for (int p = tid; p < N * N; p += nthreads) {
    const int c = p / N, r = p % N;
    const int line = axis == 0 ? r : c;
    const double* w = s.w + ((size_t)axis * N + line) * 4;
    const int* t = s.tap + ((size_t)axis * N + line) * 4;
    double acc = 0.0;
    for (int j = 0; j < 4; ++j) acc += w[j] * (axis == 0 ? in[t[j] * irs + c * ics] : in[r * irs + t[j] * ics]);
    out[r * ors + c * ocs] = acc;
  }
}

// the border of the shifted patch and its centre into LDS, for b1w_plane: ring[0][c] = (0, c), ring[1][c] = (N - 1, c),
// ring[2][r] = (r, 0), ring[3][r] = (r, N - 1), ring[4][0] = the centre
RPSFB_HD void b1w_ring_stage(int tid, int nthreads, int N, const Wide& q, const double* patch) {
  const int ld = ld_for(N);
  for (int k = tid; k <= 4 * N; k += nthreads) {
    const int side = k / N, i = k % N;
    q.ring[k] = k == 4 * N  ? patch[(N / 2) * ld + N / 2]
                : side == 0 ? patch[i]
                : side == 1 ? patch[(N - 1) * ld + i]
                : side == 2 ? patch[i * ld]
                            : patch[i * ld + N - 1];
  }
}

// b1_plane on the staged ring: the same walk (b1_ring), the same sums in the same order, the same tests
RPSFB_HD void b1w_plane(int tid, int N, const Wide& q) {
  const Lds& s = q.s;
  if (tid != 0 || s.flag[0]) return;
  const double* ring = q.ring;
  const auto at = [&](int r, int c) { return r == 0 ? ring[c] : r == N - 1 ? ring[N + c] : c == 0 ? ring[2 * N + r] : ring[3 * N + r]; };
  const double centre = ring[4 * N];
  double n = 0, sx = 0, sy = 0, sv = 0;
  rpsfb::b1_ring(N, [&](int r, int c) {
    const double v = at(r, c);
    if (v < centre) n += 1, sx += c, sy += r, sv += v;
  });
  if (n < 3) {
    s.flag[2] = rpsfb::DEGENERATE_RING;
    return;
  }
  const double mx = sx / n, my = sy / n, mv = sv / n;
  double sxx = 0, sxy = 0, syy = 0, sxv = 0, syv = 0;
  rpsfb::b1_ring(N, [&](int r, int c) {
    const double v = at(r, c);
    if (v < centre) {
      const double dx = c - mx, dy = r - my, dv = v - mv;
      sxx += dx * dx, sxy += dx * dy, syy += dy * dy, sxv += dx * dv, syv += dy * dv;
    }
  });
  const double det = sxx * syy - sxy * sxy;
  if (!(det > 1e-9 * sxx * syy)) {
    s.flag[2] = rpsfb::DEGENERATE_RING;
    return;
  }
  const double a = (sxv * syy - syv * sxy) / det, b = (syv * sxx - sxv * sxy) / det;
  s.plane[0] = a, s.plane[1] = b, s.plane[2] = mv - a * mx - b * my;
}

// One star, as a driver over `each(f)`: f(tid) for every thread of the workgroup, then a barrier.  The kernel and the emulator share
// the order of the phases this way.
template <class Each>
RPSFB_HD uint8_t b1w_star(Each&& each, int N, const float* img, int H, int W, int rr, int rc, double shift_row, double shift_col,
                          double saturation, double star_minimum, double star_maximum, const Wide& q, float* out) {
  const int ld = ld_for(N), T = THREADS;
  const Lds sa = on(q, q.a), sb = on(q, q.b);
  each([&](int tid) {
    rpsfb::b1_tables(tid, N, shift_row, shift_col, sa);
    rpsfb::b1_gather(tid, T, N, img, H, W, rr, rc, sa);
  });
  each([&](int tid) { b1w_prefilter(tid, N, q.a); });
  each([&](int tid) { b1w_transpose(tid, T, N, q.a, q.b); });
  each([&](int tid) { b1w_prefilter(tid, N, q.b); });
  each([&](int tid) { b1w_taps(tid, T, N, 0, sa, q.b, 1, ld, q.a, 1, ld); });
  each([&](int tid) { b1w_taps(tid, T, N, 1, sa, q.a, 1, ld, q.b, ld, 1); });
  each([&](int tid) {
    rpsfb::b1_scan(tid, T, N, sb);
    b1w_ring_stage(tid, T, N, q, q.b);
  });
  each([&](int tid) { b1w_plane(tid, N, q); });
  each([&](int tid) { rpsfb::b1_finish(tid, T, N, saturation, sb, out); });
  return rpsfb::b1_verdict(N, star_minimum, star_maximum, sb);
}

}  // namespace rpsfbw
