// CPU lane emulator for rpsf_core_stars_fit.hpp (test infrastructure, never shipped in the product path).
// Runs S8 as csrc/stars.hip launches it (rpsf_stars_fit): each() loops over the threads of a workgroup, workgroups run one after the
// other.  The LDS of every workgroup is exactly s8_lds_bytes() and starts with garbage, as does the output.
// With -DEMU_FIT_MAIN the file is a stand-alone program (for a sanitizer build of the driver and its LDS carve): a small frame, positions
// on and off it, every flag; it prints the flags it saw and returns 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_stars_fit.hpp"
#include "emu_ctx.hpp"

using namespace rpsff;

namespace {
long launches = 0;
}  // namespace

// info[3] = WALK_WAVES, the workgroups the last emuft_fit ran, S8's LDS bytes
extern "C" void emuft_info(long* info) { info[0] = WALK_WAVES, info[1] = launches, info[2] = (long)s8_lds_bytes(); }

// what rpsf_stars_model_create says of its arguments: 0, or -1 where the library returns RPSF_E_BADARG
extern "C" int emuft_model(long n_cells, int N, const double* values) {
  if (n_cells < 1 || n_cells > (1L << 24) || !model_size_ok(N) || !values) return -1;
  return 0;
}

// rpsf_stars_fit after a rpsf_stars_background_host: `L` is the filtered mesh S1b left (not read when none != 0), `none` its flag.
// Returns -1 where the library returns RPSF_E_BADARG; out takes n x FIT_COLUMNS doubles.
extern "C" int emuft_fit(const float* img, const uint8_t* mask, int H, int W, int box, const double* L, int none, long n_cells, int N,
                         const double* cube, long n, const double* positions, const int* cells, double radius, int fit_background,
                         int use_mesh, double* out) {
  launches = 0;
  if (H <= 0 || W <= 0 || box < MIN_BOX || box > MAX_BOX || n < 0) return -1;
  if (fit_problem(radius, fit_background) || !(radius <= max_fit_radius(N))) return -1;
  for (long i = 0; i < n; ++i)
    if (!position_ok(positions[2 * i], positions[2 * i + 1])) return -1;
  if (n == 0) return 0;
  const long npix = (long)H * W;
  std::vector<uint8_t> flags(npix, 0);
  if (mask)
    for (long i = 0; i < npix; ++i) flags[i] = mask[i] != 0;
  const Frame fr{img, flags.data(), H, W, box, (H + box - 1) / box, (W + box - 1) / box};
  const Model model{cube, (int)n_cells, N};
  const Fit fit = make_fit(radius, fit_background, N);
  for (long i = 0; i < FIT_COLUMNS * n; ++i) out[i] = -777.0;
  std::vector<char> lds(s8_lds_bytes());
  CpuCtx walk{WALK_THREADS};
  for (long first = 0; first < n; first += WALK_WAVES) {
    std::memset(lds.data(), 0x5A, lds.size());
    s8_fit(walk, fr, L, &none, use_mesh != 0, model, fit, positions, cells, n, first, lds.data(), out);
    ++launches;
  }
  return 0;
}

#if defined(EMU_FIT_MAIN)
int main() {
  const int H = 48, W = 40, box = 16, nby = 3, nbx = 3, N = 9, n_cells = 3;
  std::vector<float> img((size_t)H * W);
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const double a = (r - 20.3) * (r - 20.3) + (c - 17.6) * (c - 17.6);
      img[(size_t)r * W + c] = (float)(10.0 + 500.0 * std::exp(-a / 4.5));
    }
  img[5 * W + 5] = NAN;
  std::vector<uint8_t> mask((size_t)H * W, 0);
  mask[21 * W + 18] = 1;
  const std::vector<double> L((size_t)nby * nbx, 10.0);
  std::vector<double> cube((size_t)n_cells * N * N, 0.0);  // a Gaussian, an all-zero cell, a constant one
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) cube[(size_t)i * N + j] = std::exp(-((i - 4.0) * (i - 4.0) + (j - 4.0) * (j - 4.0)) / 4.5), cube[(size_t)2 * N * N + i * N + j] = 1.0;
  if (emuft_model(n_cells, N, cube.data()) != 0) return 1;
  const double pos[] = {20.0, 18.0, 20.5, 17.5, -100.0, -100.0, 0.0, 0.0, 47.0, 39.0, 21.0, 17.0, 5.0, 5.0, 20.3, 17.6, 60.0, 20.0};
  const int cells[] = {0, 0, 0, 0, 0, 1, 2, -1, 3};
  const long n = 9;
  int seen = 0;
  for (double radius : {1.0, 2.5, 3.5})
    for (int background : {0, 1})
      for (int use_mesh : {0, 1})
        for (int none : {0, 1}) {
          std::vector<double> out((size_t)FIT_COLUMNS * n);
          if (emuft_fit(img.data(), mask.data(), H, W, box, none ? nullptr : L.data(), none, n_cells, N, cube.data(), n, pos, cells, radius,
                        background, use_mesh, out.data()) != 0)
            return 1;
          for (long i = 0; i < n; ++i) seen |= (int)out[FIT_COLUMNS * i + COL_FFLAGS] | (out[FIT_COLUMNS * i + COL_CHI2] >= 0 ? 16 : 0);
        }
  std::printf("emu_fit: flags seen %d (31: every flag and a fit), %ld LDS bytes\n", seen, (long)s8_lds_bytes());
  return seen == 31 ? 0 : 2;
}
#endif
