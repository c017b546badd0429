// rpsf_core_builder.hpp - per-thread phases of the two PSF-builder kernels (csrc/builder.hip), shared with the CPU lane
// emulator tests/emu/emu_builder.cpp: every function does the work of ONE thread of a workgroup between two barriers, on
// plain pointers, so the emulator can run the threads one after the other and check the index algebra without a GPU.
//
// B1, one workgroup per star (regularizepsf/image_processing.py:82-121): gather the N x N patch through np.pad's reflect
// index map, shift it by the sub-pixel remainder exactly as scipy.ndimage.shift(order=3, mode='mirror') does (cubic B-spline
// prefilter with pole sqrt(3) - 2 and SciPy's mirror initialisation, then 4 taps per axis at the one fractional offset the
// patch shares), fit the background plane of calculate_background (:13-46) to the border ring, subtract it and decide
// whether the patch is kept.  All arithmetic is float64; the patch leaves as float32.
// B2, one lane per pixel of a lattice cell (regularizepsf/builder.py:53-102): mean in list order, or the exact median /
// percentile of the cell's samples (double)p / (double)centre, found by bisection on the order-preserving bit pattern.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RPSFB_HD __host__ __device__ __forceinline__
#else
#define RPSFB_HD inline
#endif

// the bit-exactness B2 promises (same additions as NumPy, one correctly rounded division per sample) forbids fused multiply-adds
// the source does not spell out
#pragma clang fp contract(off)

namespace rpsfb {

constexpr int MIN_N = 4, MAX_N = 128;
constexpr int MAX_PPT = 16;  // pixels per thread: 256 threads up to N = 64, 1024 above
constexpr double POLE = -0.26794919243112270647;  // sqrt(3) - 2, the one pole of the cubic B-spline (scipy ni_splines.c)

// flags of a star after B1
constexpr uint8_t REJECTED = 0, ACCEPTED = 1, DEGENERATE_RING = 2;

RPSFB_HD int threads_for(int N) { return N <= 64 ? 256 : 1024; }
RPSFB_HD int ld_for(int N) { return N | 1; }  // odd row pitch (in doubles): a lane per row walks its line without all lanes sharing a bank
// LDS of one B1 workgroup: the patch, then per axis and output index 4 tap weights and 4 tap indices, then the plane and the flags
RPSFB_HD size_t lds_bytes(int N) { return ((size_t)N * ld_for(N) + 2 * 4 * N + 8) * sizeof(double) + (size_t)(2 * 4 * N + 8) * sizeof(int); }

struct Lds {  // views into that block
  double* patch;  // [N][ld]
  double* w;      // [2][N][4]
  double* plane;  // a, b, c (background = a * col + b * row + c), unused
  int* tap;       // [2][N][4]
  int* flag;      // [0] a pixel is zero or not finite, [1] a pixel fails the saturation test or does not fit float32, [2] ring status
};
RPSFB_HD Lds carve(void* base, int N) {
  Lds s;
  s.patch = static_cast<double*>(base);
  s.w = s.patch + (size_t)N * ld_for(N);
  s.plane = s.w + 2 * 4 * N;
  s.tap = reinterpret_cast<int*>(s.plane + 8);
  s.flag = s.tap + 2 * 4 * N;
  return s;
}

// np.pad(mode='reflect') / scipy's 'mirror' as an index map: period 2 (len - 1), the edge sample is not repeated.  Any integer in,
// [0, len) out (len >= 2), so a gather through it cannot leave the frame whatever the corner is.
RPSFB_HD int mirror_index(long i, int len) {
  const long period = 2L * (len - 1);
  long m = i % period;
  if (m < 0) m += period;
  return (int)(m < len ? m : period - m);
}

// scipy ni_interpolation.c map_coordinate, NI_EXTEND_MIRROR: the continuous coordinate folded into [0, len - 1]
RPSFB_HD double mirror_coordinate(double in, int len) {
  const double sz2 = 2.0 * len - 2.0;
  if (in < 0) {
    in = sz2 * (double)(long)(-in / sz2) + in;
    return in <= 1 - len ? in + sz2 : -in;
  }
  if (in > len - 1) {
    in -= sz2 * (double)(long)(in / sz2);
    return in > len - 1 ? sz2 - in : in;
  }
  return in;
}

// phase 0, threads 0 .. 2N-1: taps and weights of output index i along one axis.  scipy.ndimage.shift hands NI_ZoomShift the
// negated shift, so output i samples the spline at i - shift (folded), with taps floor - 1 .. floor + 2, each mirrored.
RPSFB_HD void b1_tables(int tid, int N, double shift_row, double shift_col, const Lds& s) {
  if (tid >= 2 * N) return;
  const int axis = tid / N, i = tid % N;
  const double cc = mirror_coordinate((double)i - (axis ? shift_col : shift_row), N);
  const double fl = std::floor(cc);
  const int start = (int)fl - 1;
  const double x = cc - fl, z = 1.0 - x;
  double* w = s.w + (size_t)tid * 4;
  w[0] = z * z * z / 6.0;
  w[1] = (x * x * (x - 2.0) * 3.0 + 4.0) / 6.0;
  w[2] = (z * z * (z - 2.0) * 3.0 + 4.0) / 6.0;
  w[3] = 1.0 - w[0] - w[1] - w[2];
  for (int k = 0; k < 4; ++k) s.tap[(size_t)tid * 4 + k] = mirror_index(start + k, N);
}

// phase 1: the gather.  (rr, rc) is the rounded corner in frame coordinates; the reference slices the frame padded by N with reflect.
RPSFB_HD void b1_gather(int tid, int nthreads, int N, const float* img, int H, int W, int rr, int rc, const Lds& s) {
  const int ld = ld_for(N);
  for (int p = tid; p < N * N; p += nthreads) {
    const int r = p / N, c = p % N;
    s.patch[r * ld + c] = (double)img[(size_t)mirror_index((long)rr + r, H) * W + mirror_index((long)rc + c, W)];
  }
  if (tid < 3) s.flag[tid] = 0;
}

// phases 2a / 2b: the prefilter of one line (scipy ni_splines.c: gain, _init_causal_mirror, causal pass, _init_anticausal_mirror, anticausal
// pass), lane `tid` owns line `tid` of `axis` (0: a column, walked down the rows; 1: a row).
RPSFB_HD void b1_prefilter(int tid, int N, int axis, const Lds& s) {
  if (tid >= N) return;
  const int ld = ld_for(N);
  double* c = s.patch + (axis == 0 ? tid : (size_t)tid * ld);
  const int st = axis == 0 ? ld : 1;
  const double z = POLE;
  const double gain = (1.0 - z) * (1.0 - 1.0 / z);
  for (int i = 0; i < N; ++i) c[i * st] *= gain;
  double z_n_1 = 1.0;
  for (int i = 0; i < N - 1; ++i) z_n_1 *= z;
  double z_i = z;
  double c0 = c[0] + z_n_1 * c[(N - 1) * st];
  for (int i = 1; i < N - 1; ++i) {
    c0 += z_i * (c[i * st] + z_n_1 * c[(N - 1 - i) * st]);
    z_i *= z;
  }
  c[0] = c0 / (1.0 - z_n_1 * z_n_1);
  for (int i = 1; i < N; ++i) c[i * st] += z * c[(i - 1) * st];
  c[(N - 1) * st] = (z * c[(N - 2) * st] + c[(N - 1) * st]) * z / (z * z - 1.0);
  for (int i = N - 2; i >= 0; --i) c[i * st] = z * (c[(i + 1) * st] - c[i * st]);
}

// phases 3a / 3c: the 4 taps along `axis` for the thread's pixels, into registers (the pass is not in place: every thread reads
// before anybody writes); phases 3b / 3d put them back.
RPSFB_HD void b1_taps_read(int tid, int nthreads, int N, int axis, const Lds& s, double* v) {
  const int ld = ld_for(N);
#pragma unroll
  for (int k = 0; k < MAX_PPT; ++k) {
    const int p = tid + k * nthreads;
    if (p >= N * N) continue;
    const int r = p / N, c = p % N;
    const int line = axis == 0 ? r : c;
    const double* w = s.w + ((size_t)axis * N + line) * 4;
    const int* t = s.tap + ((size_t)axis * N + line) * 4;
    double acc = 0.0;
    for (int j = 0; j < 4; ++j) acc += w[j] * (axis == 0 ? s.patch[t[j] * ld + c] : s.patch[r * ld + t[j]]);
    v[k] = acc;
  }
}
RPSFB_HD void b1_taps_write(int tid, int nthreads, int N, const Lds& s, const double* v) {
  const int ld = ld_for(N);
#pragma unroll
  for (int k = 0; k < MAX_PPT; ++k) {
    const int p = tid + k * nthreads;
    if (p < N * N) s.patch[(p / N) * ld + p % N] = v[k];
  }
}

// phase 4a: a zero or a non-finite pixel anywhere in the shifted patch rejects it (the reference turns zeros into NaN, and NaN fails
// np.all(patch < saturation_threshold), image_processing.py:112-117).  Every thread that finds one stores the same 1: no atomics.
RPSFB_HD void b1_scan(int tid, int nthreads, int N, const Lds& s) {
  const int ld = ld_for(N);
  for (int p = tid; p < N * N; p += nthreads) {
    const double x = s.patch[(p / N) * ld + p % N];
    if (x == 0.0 || !(std::fabs(x) <= 1.79769313486231570815e308)) s.flag[0] = 1;
  }
}

// phase 4b, thread 0: the plane of calculate_background.  Without a zero pixel the fit mask is the border ring minus its corners,
// intersected with patch < centre; three-parameter least squares with centred coordinates, the ring walked in one fixed order
// (top row, bottom row, left column, right column).  Fewer than three ring pixels, or ring pixels on one line, leave no plane.
template <class F>
RPSFB_HD void b1_ring(int N, F&& f) {
  for (int c = 1; c < N - 1; ++c) f(0, c);
  for (int c = 1; c < N - 1; ++c) f(N - 1, c);
  for (int r = 1; r < N - 1; ++r) f(r, 0);
  for (int r = 1; r < N - 1; ++r) f(r, N - 1);
}
RPSFB_HD void b1_plane(int tid, int N, const Lds& s) {
  if (tid != 0 || s.flag[0]) return;
  const int ld = ld_for(N);
  const double centre = s.patch[(N / 2) * ld + N / 2];
  double n = 0, sx = 0, sy = 0, sv = 0;
  b1_ring(N, [&](int r, int c) {
    const double v = s.patch[r * ld + c];
    if (v < centre) n += 1, sx += c, sy += r, sv += v;
  });
  if (n < 3) {
    s.flag[2] = DEGENERATE_RING;
    return;
  }
  const double mx = sx / n, my = sy / n, mv = sv / n;
  double sxx = 0, sxy = 0, syy = 0, sxv = 0, syv = 0;
  b1_ring(N, [&](int r, int c) {
    const double v = s.patch[r * ld + c];
    if (v < centre) {
      const double dx = c - mx, dy = r - my, dv = v - mv;
      sxx += dx * dx, sxy += dx * dy, syy += dy * dy, sxv += dx * dv, syv += dy * dv;
    }
  });
  const double det = sxx * syy - sxy * sxy;
  if (!(det > 1e-9 * sxx * syy)) {  // det = sxx syy (1 - rho^2): zero when the pixels share a row, a column or a diagonal
    s.flag[2] = DEGENERATE_RING;
    return;
  }
  const double a = (sxv * syy - syv * sxy) / det, b = (syv * sxx - sxv * sxy) / det;
  s.plane[0] = a, s.plane[1] = b, s.plane[2] = mv - a * mx - b * my;
}

// phase 5: subtract the plane, test, store.  The tests are the reference's, on the float64 values (:117-119); a value that does not
// fit float32 counts as failing the saturation test, so that the patches kept are finite by construction.
RPSFB_HD void b1_finish(int tid, int nthreads, int N, double saturation, const Lds& s, float* out) {
  if (s.flag[0] || s.flag[2]) return;
  const int ld = ld_for(N);
  for (int p = tid; p < N * N; p += nthreads) {
    const int r = p / N, c = p % N;
    const double v = s.patch[r * ld + c] - (s.plane[0] * c + s.plane[1] * r + s.plane[2]);
    if (!(v < saturation) || !(std::fabs(v) <= 3.40282346638528859812e38)) s.flag[1] = 1;
    s.patch[r * ld + c] = v;
    out[p] = (float)v;
  }
}
// after the last barrier, thread 0: the verdict.  The centre must lie strictly inside (star_minimum, star_maximum) and, as float32,
// must not be zero - B2 divides by it.
RPSFB_HD uint8_t b1_verdict(int N, double star_minimum, double star_maximum, const Lds& s) {
  if (s.flag[0]) return REJECTED;
  if (s.flag[2]) return DEGENERATE_RING;
  const double centre = s.patch[(N / 2) * ld_for(N) + N / 2];
  return (!s.flag[1] && centre > star_minimum && centre < star_maximum && (float)centre != 0.0f) ? ACCEPTED : REJECTED;
}

// ------------------------------------------------------------------------------------------------ B2
constexpr int MEAN = 0, MEDIAN = 1, PERCENTILE = 2;

// order-preserving map of the finite doubles onto unsigned integers
RPSFB_HD uint64_t key_of(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
RPSFB_HD double value_of(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x;
  std::memcpy(&x, &u, 8);
  return x;
}
RPSFB_HD double sample(const float* stack, int member, int npix, int centre, int pixel) {
  const float* q = stack + (size_t)member * npix;
  return (double)q[pixel] / (double)q[centre];
}

// One pixel of one cell: members[0 .. M) are indices into the stack, in list order.  `quantile` is percentile / 100.
// Selection is exact and needs no storage: the k-th smallest key is the largest T with |{key < T}| <= k, built bit by bit (64 passes
// over the samples); one more pass gives the next order statistic.  The result depends on the multiset of samples only.
RPSFB_HD double b2_pixel(const float* stack, const int32_t* members, long M, int N, int pixel, int method, double quantile) {
  const int npix = N * N, centre = (N / 2) * N + N / 2;
  if (M == 0) return 0.0;  // what the reference's NaN -> 0 fill leaves of a cell without a star (builder.py:119-123)
  if (method == MEAN) {  // the additions of the repeated np.nansum([accumulator, patch]) of builder.py:66, in its order
    double acc = 0.0;
    for (long m = 0; m < M; ++m) acc += sample(stack, members[m], npix, centre, pixel);
    return acc / (double)M;
  }
  // NumPy: median = mean of the two middle samples; percentile = default 'linear' method on the virtual index (M - 1) q
  long k;
  double t;
  if (method == MEDIAN) {
    k = (M - 1) / 2;
    t = (M % 2 == 0) ? 0.5 : 0.0;
  } else {
    const double v = (double)(M - 1) * quantile;
    const double fl = std::floor(v);
    k = (long)fl;
    t = v - fl;
    if (k >= M - 1) k = M - 1, t = 0.0;
  }
  uint64_t ans = 0;
  for (int bit = 63; bit >= 0; --bit) {
    const uint64_t trial = ans | (1ull << bit);
    long below = 0;
    for (long m = 0; m < M; ++m) below += key_of(sample(stack, members[m], npix, centre, pixel)) < trial;
    if (below <= k) ans = trial;
  }
  const double a = value_of(ans);
  if (t == 0.0) return a;
  long not_above = 0;
  uint64_t next = ~0ull;
  for (long m = 0; m < M; ++m) {
    const uint64_t key = key_of(sample(stack, members[m], npix, centre, pixel));
    if (key <= ans) ++not_above;
    else if (key < next) next = key;
  }
  const double b = not_above >= k + 2 ? a : value_of(next);
  if (method == MEDIAN) return (a + b) / 2.0;
  const double d = b - a;  // numpy's _lerp
  return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

}  // namespace rpsfb
