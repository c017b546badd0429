// CPU lane emulator for rpsf_core_cleanup_wide.hpp (test infrastructure, never shipped in the product path).
// Runs the driver of kernel B3w as builder_clean_wide_kernel does: `slots` workgroups, workgroup b takes cells b, b + slots, ... with
// its own LDS and its own slot of the workspace; each() runs the threads of the workgroup one after the other where the kernel has
// them run side by side and then a barrier.  LDS and workspace are filled with a pattern once per workgroup and not between its
// cells: nothing may depend on what the cell before left there.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_cleanup_wide.hpp"

namespace {
struct EmuCtx {
  template <class F>
  void each(F&& f) {
    for (int tid = 0; tid < rpsfcw::THREADS; ++tid) f(tid);
  }
};
}  // namespace

extern "C" int emucw_clean(int N, int n_cells, const double* in, double* out, uint8_t* flags, int slots) {
  if (N < rpsfcw::EMU_MIN_N || N > rpsfcw::MAX_N || n_cells < 0 || slots < 1) return -1;
  std::vector<double> lds(rpsfcw::lds_bytes(N) / sizeof(double) + 1), slot(rpsfcw::slot_bytes(N) / sizeof(double) + 1);
  EmuCtx ctx;
  for (int block = 0; block < slots && block < n_cells; ++block) {
    std::memset(lds.data(), 0xA5, lds.size() * sizeof(double));
    std::memset(slot.data(), 0xA5, slot.size() * sizeof(double));
    for (int cell = block; cell < n_cells; cell += slots) {
      const size_t at = (size_t)cell * N * N;
      rpsfcw::clean_cell_wide(ctx, N, in + at, out + at, flags + cell, lds.data(), slot.data());
    }
  }
  return 0;
}

extern "C" size_t emucw_lds_bytes(int N) { return rpsfcw::lds_bytes(N); }
extern "C" size_t emucw_slot_bytes(int N) { return rpsfcw::slot_bytes(N); }
