// CPU lane emulator for rpsf_core_cleanup.hpp (test infrastructure, never shipped in the product path).
// Runs the driver of kernel B3 once per cell; each() runs the threads of the workgroup one after the other where
// builder_clean_kernel has them run side by side and then a barrier, on the same LDS layout and with the same per-thread
// registers - so the masks, the fit, the labelling and the order of every sum are checked against builder.clean_cell without a GPU.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_cleanup.hpp"

namespace {
struct EmuCtx {
  int threads;
  std::vector<rpsfc::Regs> registers;
  template <class F>
  void each(F&& f) {
    for (int tid = 0; tid < threads; ++tid) f(tid);
  }
  rpsfc::Regs& regs(int tid) { return registers[(size_t)tid]; }
};
}  // namespace

extern "C" int emuc_clean(int N, int n_cells, const double* in, double* out, uint8_t* flags) {
  if (N < rpsfb::MIN_N || N > rpsfb::MAX_N || n_cells < 0) return -1;
  std::vector<double> lds(rpsfc::lds_bytes(N) / sizeof(double) + 1);
  EmuCtx ctx{rpsfb::threads_for(N), {}};
  for (int cell = 0; cell < n_cells; ++cell) {
    std::memset(lds.data(), 0xA5, lds.size() * sizeof(double));  // nothing may depend on what the previous cell left
    ctx.registers.assign((size_t)ctx.threads, rpsfc::Regs{});
    for (auto& g : ctx.registers) std::memset(&g, 0xA5, sizeof g);
    const size_t at = (size_t)cell * N * N;
    rpsfc::clean_cell(ctx, N, ctx.threads, in + at, out + at, flags + cell, lds.data());
  }
  return 0;
}

extern "C" size_t emuc_lds_bytes(int N) { return rpsfc::lds_bytes(N); }
