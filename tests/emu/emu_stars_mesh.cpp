// CPU lane emulator for rpsf_core_stars_mesh.hpp (test infrastructure, never shipped in the product path).
// Runs kernel S1b of the star finder - the fill and the 3 x 3 median filter of the background mesh - as csrc/stars.hip launches it: the
// one-workgroup driver with a context whose each() loops over the threads, or the many-workgroup route launch by launch, workgroups and
// grid threads one after the other.  `many`: 0 the one workgroup, 1 the many-workgroup route, -1 what the library picks for the size.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_stars_mesh.hpp"
#include "emu_ctx.hpp"

using namespace rpsfm;

namespace {

void select_many(const Source& src, Sel* state, Total* acc, std::vector<uint64_t>& lds) {
  const int nwg = many_workgroups(src.n);
  CpuCtx ctx{S1B_THREADS};
  many_step(state, acc, -1);
  for (int step = 0; step < STEPS; ++step) {
    for (int wg = 0; wg < nwg; ++wg) {
      for (uint64_t& x : lds) x = 0x5555555555555555ull;  // nothing may depend on what was left
      many_count(ctx, wg, nwg, src, state, step, acc, lds.data());
    }
    many_step(state, acc, step);
  }
}
}  // namespace

extern "C" void emusm_info(int* threads, long* many_nodes, long* lds_bytes) {
  *threads = S1B_THREADS, *many_nodes = MANY_NODES, *lds_bytes = (long)s1b_lds_bytes();
}

// level_out / rms_out: the filtered meshes; *none = 1: no valid node (then the outputs are not touched, *T = +inf)
extern "C" int emusm_filter_mesh(const double* level_in, const double* rms_in, int nby, int nbx, double threshold, int many, double* level_out,
                                 double* rms_out, double* global_rms, double* T, int* none) {
  if (nby <= 0 || nbx <= 0) return -1;
  const long n = (long)nby * nbx;
  std::vector<double> level(level_in, level_in + n), rms(rms_in, rms_in + n), level_f(n, -7.0), rms_f(n, -7.0);
  std::vector<uint64_t> lds(s1b_lds_bytes() / sizeof(uint64_t) + 1, 0x5555555555555555ull);
  double out[2] = {-7.0, -7.0};
  int flag = -1;
  const bool use_many = many < 0 ? n > MANY_NODES : many != 0;
  if (!use_many) {
    CpuCtx ctx{S1B_THREADS};
    s1b_mesh(ctx, nby, nbx, level.data(), rms.data(), level_f.data(), rms_f.data(), out, &flag, lds.data());
  } else {
    Sel state[2];
    Total acc;
    select_many(Source{level.data(), rms.data(), n, 1}, &state[0], &acc, lds);
    for (long i = 0; i < n + 3; ++i) many_fill(i, n, level.data(), rms.data(), &state[0]);  // (a grid is rounded up)
    for (long i = 0; i < n + 3; ++i) many_filter(i, nby, nbx, level.data(), rms.data(), level_f.data(), rms_f.data());
    select_many(Source{rms_f.data(), rms_f.data(), n, 0}, &state[1], &acc, lds);
    many_finish(&state[0], &state[1], out, &flag);
  }
  *none = flag;
  *T = threshold_of(threshold, out[OUT_GLOBAL_RMS], flag);
  if (flag) return 0;
  for (long i = 0; i < n; ++i) level_out[i] = level_f[i], rms_out[i] = rms_f[i];
  *global_rms = out[OUT_GLOBAL_RMS];
  return 0;
}
