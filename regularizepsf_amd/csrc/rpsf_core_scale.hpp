// rpsf_core_scale.hpp - per-thread phases of the frame upscale (kernels U1 / U2) and of the block mean (kernel B4) of csrc/scale.hip,
// shared with the CPU lane emulator tests/emu/emu_scale.cpp: every function does the work of ONE thread between two barriers, on plain
// pointers, so the emulator can run the threads one after the other and check the arithmetic and the index algebra without a GPU.
//
// The upscale is regularizepsf/image_processing.py:49-59: RectBivariateSpline(arange(H), arange(W), z) with its defaults, evaluated on
// 1 + (H - 1) s by 1 + (W - 1) s samples.  That spline is the tensor product of the 1-D not-a-knot interpolating cubic spline, so one
// pass per axis does it.  Per line y[0 .. m) with unit spacing, in the second-derivative form (M[i] = S''(i)):
//     interior rows   M[i-1] + 4 M[i] + M[i+1] = 6 d[i],   d[i] = (y[i+1] - y[i]) - (y[i] - y[i-1]),   i = 1 .. m-2
//     not-a-knot      M[0] = 2 M[1] - M[2]  and  M[m-1] = 2 M[m-2] - M[m-3]   (S''' continuous at 1 and at m-2),
//                     which turns rows 1 and m-2 into M[1] = d[1] and M[m-2] = d[m-2]
// and leaves a (1, 4, 1) system for M[2 .. m-3]: m - 4 unknowns, none at m = 4, one at m = 5.  Its elimination pivots do not depend on the
// data; pivot_table() builds their reciprocals in plain C++ on the host.  On [i, i+1] at t = j / s, u = 1 - t:
//     S = y[i] + t (y[i+1] - y[i]) + ((u^3 - u) M[i] + (t^3 - t) M[i+1]) / 6,      and S = y[i] itself at j = 0.
// All arithmetic is float64 whatever the input type; sums run in a fixed order.
//
// Lane mapping: u_line() gives one lane one whole line of a [line index][lane] array, so a wavefront's loads and stores are coalesced along
// the lanes and nothing is truncated.  The axis-0 pass has that layout as the frame comes; the axis-1 pass gets it from a 32 x 32
// transpose through LDS before and after (t_load / t_store), the second of which also narrows to float32 where the builder wants it.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RPSFS_HD __host__ __device__ __forceinline__
#else
#define RPSFS_HD inline
#endif

namespace rpsfs {

constexpr int MIN_LINE = 4;  // the reference's cubic spline needs four points
constexpr int TILE = 32;     // the transpose tile; TILE x 8 threads move it in 4 passes
constexpr int TILE_ROWS = 8;
constexpr int TILE_LD = TILE + 1;  // odd pitch in doubles: the column walk of t_store meets every bank pair once
constexpr int LINE_THREADS = 256;  // lanes per workgroup of the line kernel

RPSFS_HD long scaled(long m, int s) { return 1 + (m - 1) * (long)s; }

// Reciprocal pivots of the (1, 4, 1) elimination for a line of m samples: ip[0] = 1/4, ip[k] = 1 / (4 - ip[k-1]), k < m - 4.
// Host only, once per line length; ip[k] is also the eliminated super-diagonal of row k.
inline void pivot_table(int m, double* ip) {
  for (int k = 0; k < m - 4; ++k) ip[k] = k == 0 ? 0.25 : 1.0 / (4.0 - ip[k - 1]);
}

// U1 / U2: lane `lane` of `lanes` owns line y[i * lanes + lane], i < m (m >= 4), and writes out[(i * s + j) * lanes + lane].
// work[k * lanes + lane], k < m - 4, holds the forward sweep's right-hand sides until the back-substitution reads them.
template <class T>
RPSFS_HD void u_line(long lane, long lanes, int m, int s, const T* y, const double* ip, double* work, double* out) {
  if (lane >= lanes) return;
  const T* col = y + lane;
  double* w = work + lane;
  double* o = out + lane;
  const size_t ld = (size_t)lanes;
  auto Y = [&](int i) { return (double)col[(size_t)i * ld]; };
  auto second = [&](double a, double b, double c) { return (c - b) - (b - a); };
  const int n = m - 4;
  const double d1 = second(Y(0), Y(1), Y(2));              // M[1]
  const double dl = second(Y(m - 3), Y(m - 2), Y(m - 1));  // M[m-2]
  {  // forward sweep over rows i = 2 .. m-3 (unknown k = i - 2)
    double ya = Y(1), yb = Y(2), r = 0.0;
    for (int k = 0; k < n; ++k) {
      const double yc = Y(k + 3);
      double rhs = 6.0 * second(ya, yb, yc);
      if (k == 0) rhs -= d1;
      if (k == n - 1) rhs -= dl;
      r = (rhs - r) * ip[k];
      w[(size_t)k * ld] = r;
      ya = yb, yb = yc;
    }
  }
  // back-substitution from the far end, one interval [i, i+1] evaluated per step
  const double m3 = n > 0 ? w[(size_t)(n - 1) * ld] : d1;  // M[m-3]
  double hi2 = 0.0, hi = 2.0 * dl - m3, yhi = Y(m - 1);    // M[i+2], M[i+1], y[i+1]
  o[(size_t)(m - 1) * s * ld] = yhi;                       // the last sample is the data point itself
  const double inv = 1.0 / (double)s;
  for (int i = m - 2; i >= 0; --i) {
    double mi;
    if (i == 0) mi = 2.0 * hi - hi2;
    else if (i == 1) mi = d1;
    else if (i == m - 2) mi = dl;
    else if (i == m - 3) mi = m3;
    else mi = w[(size_t)(i - 2) * ld] - ip[i - 2] * hi;
    const double yi = Y(i), dy = yhi - yi;
    double* at = o + (size_t)i * s * ld;
    at[0] = yi;
    for (int j = 1; j < s; ++j) {
      const double t = (double)j * inv, u = 1.0 - t;
      at[(size_t)j * ld] = yi + t * dy + ((u * u * u - u) * mi + (t * t * t - t) * hi) / 6.0;
    }
    hi2 = hi, hi = mi, yhi = yi;
  }
}

// The transpose of a rows x cols float64 array, tile (tr, tc) of it, by TILE x TILE_ROWS threads with a barrier between the two phases;
// tile is TILE x TILE_LD doubles of LDS.  tid = ty * TILE + tx.
RPSFS_HD void t_load(int tid, long tr, long tc, long rows, long cols, const double* in, double* tile) {
  const int tx = tid % TILE, ty = tid / TILE;
  const long c = tc * TILE + tx;
  for (int k = ty; k < TILE; k += TILE_ROWS) {
    const long r = tr * TILE + k;
    if (r < rows && c < cols) tile[k * TILE_LD + tx] = in[(size_t)r * cols + c];
  }
}
// out is cols x rows; Tout is double, or float for the builder's frame buffer (one rounding, of the finished float64 value)
template <class Tout>
RPSFS_HD void t_store(int tid, long tr, long tc, long rows, long cols, const double* tile, Tout* out) {
  const int tx = tid % TILE, ty = tid / TILE;
  const long r = tr * TILE + tx;  // the input row this thread writes, now the fast axis
  for (int k = ty; k < TILE; k += TILE_ROWS) {
    const long c = tc * TILE + k;
    if (r < rows && c < cols) out[(size_t)c * rows + r] = (Tout)tile[tx * TILE_LD + k];
  }
}

// B4, one lane per output pixel: the mean of the s x s block of a P x P cell (P = N s), summed in row-major order
// (skimage.transform.downscale_local_mean for a P that s divides, builder.py:234-235).
RPSFS_HD double b4_pixel(const double* cell, int N, int s, int pixel) {
  const int r = pixel / N, c = pixel % N, P = N * s;
  double sum = 0.0;
  for (int a = 0; a < s; ++a)
    for (int b = 0; b < s; ++b) sum += cell[(size_t)(r * s + a) * P + c * s + b];
  return sum / (double)(s * s);
}

}  // namespace rpsfs
