// CPU lane emulator for rpsf_core_builder.hpp (test infrastructure, never shipped in the product path).
// Runs the per-thread phases of the two PSF-builder kernels thread by thread, with a phase boundary wherever
// builder_patch_kernel has a barrier, on the same LDS layout - so the reflect gather, the spline prefilter and taps, the
// ring fit, the accept rules and the selection of B2 are checked against the reference's results without a GPU.
#include <cstdint>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_builder.hpp"

using namespace rpsfb;

extern "C" int emub_patches(int N, const float* img, int H, int W, int n_stars, const int32_t* corners, const double* frac,
                            double saturation, double star_minimum, double star_maximum, float* patches, uint8_t* flags) {
  if (N < MIN_N || N > MAX_N || H < 2 || W < 2) return -1;
  const int T = threads_for(N);
  std::vector<double> lds(lds_bytes(N) / sizeof(double) + 1);
  std::vector<double> regs((size_t)T * MAX_PPT);
  for (int star = 0; star < n_stars; ++star) {
    for (double& x : lds) x = std::nan("");  // nothing may depend on what the previous star left
    const Lds s = carve(lds.data(), N);
    float* out = patches + (size_t)star * N * N;
    for (int t = 0; t < T; ++t) {
      b1_tables(t, N, frac[2 * star], frac[2 * star + 1], s);
      b1_gather(t, T, N, img, H, W, corners[2 * star], corners[2 * star + 1], s);
    }
    for (int axis = 0; axis < 2; ++axis)
      for (int t = 0; t < T; ++t) b1_prefilter(t, N, axis, s);
    for (int axis = 0; axis < 2; ++axis) {
      for (int t = 0; t < T; ++t) b1_taps_read(t, T, N, axis, s, &regs[(size_t)t * MAX_PPT]);
      for (int t = 0; t < T; ++t) b1_taps_write(t, T, N, s, &regs[(size_t)t * MAX_PPT]);
    }
    for (int t = 0; t < T; ++t) b1_scan(t, T, N, s);
    for (int t = 0; t < T; ++t) b1_plane(t, N, s);
    for (int t = 0; t < T; ++t) b1_finish(t, T, N, saturation, s, out);
    flags[star] = b1_verdict(N, star_minimum, star_maximum, s);
  }
  return 0;
}

extern "C" int emub_average(const float* stack, int N, int method, double percentile, int n_cells, const int64_t* offsets,
                            const int32_t* members, double* cells) {
  for (int cell = 0; cell < n_cells; ++cell)
    for (int pixel = 0; pixel < N * N; ++pixel)
      cells[(size_t)cell * N * N + pixel] =
          b2_pixel(stack, members + offsets[cell], (long)(offsets[cell + 1] - offsets[cell]), N, pixel, method, percentile / 100.0);
  return 0;
}
