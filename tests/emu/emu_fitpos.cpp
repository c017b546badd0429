// CPU lane emulator for rpsf_core_stars_fitpos.hpp (test infrastructure, never shipped in the product path).
// Runs S9 and then S8 as csrc/stars.hip launches them (rpsf_stars_fit_positions): each() loops over the threads of a workgroup, workgroups
// run one after the other.  The LDS of every workgroup is exactly s9_lds_bytes() (s8_lds_bytes() for S8) and starts with garbage, as do the
// outputs.
// With -DEMU_FITPOS_MAIN the file is a stand-alone program (for a sanitizer build of the driver and its LDS carve): a small frame, four
// stars of one workgroup with different fates, every stop rule, row counts around a workgroup; it prints the flags it saw and returns 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_stars_fitpos.hpp"
#include "emu_ctx.hpp"

using namespace rpsfg;

namespace {
long launches = 0;
}  // namespace

// info[3] = WALK_WAVES, the workgroups of S9 the last emufp_fit_positions ran, S9's LDS bytes
extern "C" void emufp_info(long* info) { info[0] = WALK_WAVES, info[1] = launches, info[2] = (long)s9_lds_bytes(); }

// rpsf_stars_fit_positions after a rpsf_stars_background_host: `L` is the filtered mesh S1b left (not read when none != 0), `none` its
// flag.  Returns -1 where the library returns RPSF_E_BADARG; iter_out takes n x FITPOS_COLUMNS doubles, fit_out n x FIT_COLUMNS.
extern "C" int emufp_fit_positions(const float* img, const uint8_t* mask, int H, int W, int box, const double* L, int none, long n_cells, int N,
                                   const double* cube, long n, const double* positions, const int* cells, double radius, int fit_background,
                                   int max_iter, double eps, double max_shift, double max_step, int use_mesh, double* iter_out,
                                   double* fit_out) {
  launches = 0;
  if (H <= 0 || W <= 0 || box < MIN_BOX || box > MAX_BOX || n < 0) return -1;
  if (fit_problem(radius, fit_background) || fitpos_problem(max_iter, eps, max_shift, max_step) || !(radius <= max_fit_radius(N))) return -1;
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
  const FitPos fp = make_fitpos(max_iter, eps, max_shift, max_step);
  for (long i = 0; i < FITPOS_COLUMNS * n; ++i) iter_out[i] = -777.0;
  for (long i = 0; i < FIT_COLUMNS * n; ++i) fit_out[i] = -777.0;
  std::vector<double> final_pos(2 * n, -777.0);
  std::vector<char> lds(s9_lds_bytes());
  CpuCtx walk{WALK_THREADS};
  for (long first = 0; first < n; first += WALK_WAVES) {
    std::memset(lds.data(), 0x5A, lds.size());
    s9_fit_positions(walk, fr, L, &none, use_mesh != 0, model, fit, fp, positions, cells, n, first, lds.data(), iter_out, final_pos.data());
    ++launches;
  }
  lds.resize(s8_lds_bytes());
  for (long first = 0; first < n; first += WALK_WAVES) {
    std::memset(lds.data(), 0x5A, lds.size());
    s8_fit(walk, fr, L, &none, use_mesh != 0, model, fit, final_pos.data(), cells, n, first, lds.data(), fit_out);
  }
  return 0;
}

#if defined(EMU_FITPOS_MAIN)
int main() {
  const int H = 48, W = 40, box = 16, nby = 3, nbx = 3, N = 9, n_cells = 4;
  std::vector<float> img((size_t)H * W);
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const double a = (r - 20.3) * (r - 20.3) + (c - 17.6) * (c - 17.6), b = (r - 33.5) * (r - 33.5) + (c - 10.5) * (c - 10.5);
      img[(size_t)r * W + c] = (float)(10.0 + 500.0 * std::exp(-a / 3.38) + 300.0 * std::exp(-b / 3.38));
    }
  img[5 * W + 5] = NAN;
  std::vector<uint8_t> mask((size_t)H * W, 0);
  mask[21 * W + 18] = 1;
  const std::vector<double> L((size_t)nby * nbx, 10.0);
  std::vector<double> cube((size_t)n_cells * N * N, 0.0);  // a Gaussian, an all-zero cell, a constant one, a cell of NaN
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      cube[(size_t)i * N + j] = std::exp(-((i - 4.0) * (i - 4.0) + (j - 4.0) * (j - 4.0)) / 3.38);
      cube[(size_t)2 * N * N + i * N + j] = 1.0, cube[(size_t)3 * N * N + i * N + j] = NAN;
    }
  // converging, capped, running away, skipped; then the singular cells, off the frame, the rim, and a second workgroup's tail
  const double pos[] = {20.0, 18.0, 33.0, 11.0, 21.3, 17.6, 20.0, 18.0, 20.0, 18.0, 20.0, 18.0, 20.0, 18.0, -100.0, -100.0, 0.0, 0.0, 47.0, 39.0, 33.9, 10.1};
  const int cells[] = {0, 0, 0, -1, 1, 2, 3, 0, 0, 0, 0};
  int seen = 0;
  for (long n : {0L, 1L, 3L, 4L, 5L, 9L, 11L})
    for (int max_iter : {0, 2, 16})
      for (double max_shift : {0.25, 2.0})
        for (int background : {0, 1})
          for (int use_mesh : {0, 1})
            for (int none : {0, 1}) {
              std::vector<double> it((size_t)FITPOS_COLUMNS * n + 1), ft((size_t)FIT_COLUMNS * n + 1);
              if (emufp_fit_positions(img.data(), mask.data(), H, W, box, none ? nullptr : L.data(), none, n_cells, N, cube.data(), n, pos, cells,
                                      3.5, background, max_iter, 1e-4, max_shift, 0.5, use_mesh, it.data(), ft.data()) != 0)
                return 1;
              for (long i = 0; i < n; ++i) {
                const double* row = &it[FITPOS_COLUMNS * i];
                seen |= (int)row[PCOL_FLAGS] | (row[PCOL_NITER] > 0 && row[PCOL_FLAGS] == 0 ? 16 : 0);
              }
            }
  std::printf("emu_fitpos: flags seen %d (31: every stop rule and a converged star), %ld LDS bytes\n", seen, (long)s9_lds_bytes());
  return seen == 31 ? 0 : 2;
}
#endif
