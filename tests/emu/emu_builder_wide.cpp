// CPU lane emulator for rpsf_core_builder_wide.hpp (test infrastructure, never shipped in the product path).
// Runs the driver of kernel B1w as builder_patch_wide_kernel does: `slots` workgroups, workgroup b takes stars b, b + slots, ... in
// its own slot of the workspace; each() runs the threads of the workgroup one after the other where the kernel has them run side by
// side and then a barrier.  The workspace is filled with NaN once and not between the stars of a slot: nothing may depend on what
// the star before left there.  The phases take any N from 4 on, so the emulator also runs them at B1's sizes, where
// tests/test_builder_wide_host.py asks for B1's bits.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_builder_wide.hpp"

using namespace rpsfbw;

extern "C" int emubw_patches(int N, const float* img, int H, int W, int n_stars, const int32_t* corners, const double* frac,
                             double saturation, double star_minimum, double star_maximum, int slots, float* patches, uint8_t* flags) {
  if (N < EMU_MIN_N || N > MAX_N || H < 2 || W < 2 || slots < 1) return -1;
  std::vector<double> lds(lds_bytes(N) / sizeof(double) + 1);
  std::vector<double> workspace((size_t)slots * slot_doubles(N), std::nan(""));
  const auto each = [](auto&& f) {
    for (int tid = 0; tid < THREADS; ++tid) f(tid);
  };
  for (int block = 0; block < slots && block < n_stars; ++block) {
    for (double& x : lds) x = std::nan("");
    const Wide q = carve(lds.data(), workspace.data() + (size_t)block * slot_doubles(N), N);
    for (int star = block; star < n_stars; star += slots)
      flags[star] = b1w_star(each, N, img, H, W, corners[2 * star], corners[2 * star + 1], frac[2 * star], frac[2 * star + 1], saturation,
                             star_minimum, star_maximum, q, patches + (size_t)star * N * N);
  }
  return 0;
}

extern "C" size_t emubw_lds_bytes(int N) { return lds_bytes(N); }
extern "C" size_t emubw_slot_bytes(int N) { return slot_doubles(N) * sizeof(double); }
extern "C" int emubw_slots(int N) { return slots_for(N); }
