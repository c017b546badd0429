// CPU lane emulator for rpsf_core_stars_refine.hpp (test infrastructure, never shipped in the product path).
// Runs S7 as csrc/stars.hip launches it (rpsf_stars_refine): each() loops over the threads of a workgroup, workgroups run one after the
// other.  The LDS of every workgroup is exactly s7_lds_bytes() and starts with garbage, as does the output.
// With -DEMU_REFINE_MAIN the file is a stand-alone program (for a sanitizer build of the driver and its LDS carve): a small frame, positions
// on and off it, every stop rule; it prints the flags it saw and returns 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_stars_refine.hpp"
#include "emu_ctx.hpp"

using namespace rpsfr;

namespace {
long launches = 0;
}  // namespace

// info[3] = WALK_WAVES, the workgroups the last emurf_refine ran, S7's LDS bytes
extern "C" void emurf_info(long* info) { info[0] = WALK_WAVES, info[1] = launches, info[2] = (long)s7_lds_bytes(); }

// the window function alone: out[i] = g(t[i])
extern "C" void emurf_window(long n, const double* t, double* out) {
  for (long i = 0; i < n; ++i) out[i] = window_g(t[i]);
}

// rpsf_stars_refine after a rpsf_stars_background_host: `L` is the filtered mesh S1b left (not read when none != 0), `none` its flag.
// Returns -1 where the library returns RPSF_E_BADARG; out takes n x REFINE_COLUMNS doubles.
extern "C" int emurf_refine(const float* img, const uint8_t* mask, int H, int W, int box, const double* L, int none, long n,
                            const double* positions, const double* sigma, int max_iter, double eps, double max_shift, int use_mesh,
                            double* out) {
  launches = 0;
  if (H <= 0 || W <= 0 || box < MIN_BOX || box > MAX_BOX || n < 0) return -1;
  if (refine_problem(max_iter, eps, max_shift)) return -1;
  for (long i = 0; i < n; ++i)
    if (!position_ok(positions[2 * i], positions[2 * i + 1]) || !sigma_ok(sigma[i])) return -1;
  if (n == 0) return 0;
  const long npix = (long)H * W;
  std::vector<uint8_t> flags(npix, 0);
  if (mask)
    for (long i = 0; i < npix; ++i) flags[i] = mask[i] != 0;
  const Frame fr{img, flags.data(), H, W, box, (H + box - 1) / box, (W + box - 1) / box};
  const Refine rf = make_refine(max_iter, eps, max_shift);
  for (long i = 0; i < REFINE_COLUMNS * n; ++i) out[i] = -777.0;
  std::vector<char> lds(s7_lds_bytes());
  CpuCtx walk{WALK_THREADS};
  for (long first = 0; first < n; first += WALK_WAVES) {
    std::memset(lds.data(), 0x5A, lds.size());
    s7_refine(walk, fr, L, &none, use_mesh != 0, rf, positions, sigma, n, first, lds.data(), out);
    ++launches;
  }
  return 0;
}

#if defined(EMU_REFINE_MAIN)
int main() {
  const int H = 48, W = 40, box = 16, nby = 3, nbx = 3;
  std::vector<float> img((size_t)H * W);
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) {
      const double a = (r - 20.3) * (r - 20.3) + (c - 17.6) * (c - 17.6), b = (r - 22.0) * (r - 22.0) + (c - 30.0) * (c - 30.0);
      img[(size_t)r * W + c] = (float)(10.0 + 500.0 * std::exp(-a / 4.5) - 300.0 * std::exp(-b / 4.5));
    }
  img[5 * W + 5] = NAN;
  std::vector<uint8_t> mask((size_t)H * W, 0);
  mask[21 * W + 18] = 1;
  const std::vector<double> L((size_t)nby * nbx, 10.0);
  const double pos[] = {20.0, 18.0, 22.0, 30.0, -100.0, -100.0, 0.0, 0.0, 47.0, 39.0, 21.0, 17.0, 19.0, 16.0, 20.0, 18.0, 60.0, 20.0};
  const double sigma[] = {1.5, 1.5, 0.5, 16.0, 16.0, 2.5, 1.0, 16.0, 3.0};
  const long n = 9;
  int seen = 0;
  for (int max_iter : {0, 1, 16, 64})
    for (int use_mesh : {0, 1})
      for (int none : {0, 1}) {
        std::vector<double> out((size_t)REFINE_COLUMNS * n);
        if (emurf_refine(img.data(), mask.data(), H, W, box, none ? nullptr : L.data(), none, n, pos, sigma, max_iter, 1e-4, 2.0, use_mesh,
                         out.data()) != 0)
          return 1;
        for (long i = 0; i < n; ++i) seen |= (int)out[REFINE_COLUMNS * i + COL_FLAGS] | (out[REFINE_COLUMNS * i + COL_NITER] > 0 ? 8 : 0);
      }
  std::printf("emu_refine: flags seen %d (15: every stop rule and a step), %ld LDS bytes\n", seen, (long)s7_lds_bytes());
  return 0;
}
#endif
