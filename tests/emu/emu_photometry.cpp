// CPU lane emulator for rpsf_core_stars_photometry.hpp (test infrastructure, never shipped in the product path).
// Runs S6 as csrc/stars.hip launches it (rpsf_stars_photometry): each() loops over the threads of a workgroup, workgroups run one after
// the other.  The LDS of every workgroup and the output start with garbage.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_stars_photometry.hpp"
#include "emu_ctx.hpp"

using namespace rpsfp;

namespace {
long launches = 0;
}  // namespace

// info[4] = WALK_WAVES, the workgroups the last emuph_photometry ran, S6's LDS bytes for info[3] radii (in: info[3])
extern "C" void emuph_info(long* info) { info[0] = WALK_WAVES, info[1] = launches, info[2] = (long)s6_lds_bytes((int)info[3]); }

// rpsf_stars_photometry after a rpsf_stars_background_host: `L` is the filtered mesh S1b left (not read when none != 0), `none` its flag.
// Returns -1 where the library returns RPSF_E_BADARG; out takes n x photometry_columns(m) doubles.
extern "C" int emuph_photometry(const float* img, const uint8_t* mask, int H, int W, int box, const double* L, int none, long n,
                                const double* positions, int m, const double* radii, int subpix, int use_mesh, double* out) {
  launches = 0;
  if (H <= 0 || W <= 0 || box < MIN_BOX || box > MAX_BOX || n < 0) return -1;
  if (apertures_problem(m, radii, subpix)) return -1;
  for (long i = 0; i < n; ++i)
    if (!position_ok(positions[2 * i], positions[2 * i + 1])) return -1;
  if (n == 0) return 0;
  const long npix = (long)H * W;
  std::vector<uint8_t> flags(npix, 0);
  if (mask)
    for (long i = 0; i < npix; ++i) flags[i] = mask[i] != 0;
  const Frame fr{img, flags.data(), H, W, box, (H + box - 1) / box, (W + box - 1) / box};
  const Apertures ap = make_apertures(m, radii, subpix);
  const int columns = photometry_columns(m);
  for (long i = 0; i < columns * n; ++i) out[i] = -777.0;
  std::vector<char> lds(s6_lds_bytes(m));
  CpuCtx walk{WALK_THREADS};
  for (long first = 0; first < n; first += WALK_WAVES) {
    std::memset(lds.data(), 0x5A, lds.size());
    s6_apertures(walk, fr, L, &none, use_mesh != 0, ap, positions, n, first, lds.data(), out);
    ++launches;
  }
  return 0;
}
