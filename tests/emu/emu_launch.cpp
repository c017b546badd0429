// C entry points over rpsf_launch.hpp for tests/test_launch_host.py (test infrastructure, never shipped in
// the product path): the form, the grid, the workgroups of each role and the queue draws the library decides for one apply, without a GPU.
#include "../../regularizepsf_amd/csrc/rpsf_launch.hpp"

using namespace rpsf;

// in (23): N, gen2, wg_threads, n_patches, tiles, frames, wgs_per_cu, cu_count, round_capacity, reserved_cus, sum_first override, head_patches,
//          persist, fused, hot_geometry, out_span_ok, planes_floats, k_cached, plane_nt_opt, frame_major_opt, stagger_us, prefetch, k_prefetch
// out (24): form, variant, grid, chunk, patch_blocks, stagger_ticks, stagger_blocks, sum_first, frame_major, plane_nt, rows, head_patches, prefetch,
//           k_prefetch, sum_queue_draws, xq_draws[8], too_large
extern "C" void emu_launch_decide(const int64_t* in, int64_t* out) {
  LaunchInput i;
  i.N = (int)in[0], i.gen2 = in[1] != 0, i.wg_threads = (int)in[2], i.n_patches = (int)in[3], i.tiles = (int)in[4], i.frames = (int)in[5];
  i.wgs_per_cu = (int)in[6], i.cu_count = (int)in[7], i.round_capacity = (int)in[8], i.reserved_cus = (int)in[9], i.sum_first = (int)in[10];
  i.head_patches = (int)in[11], i.persist = in[12] != 0, i.fused = in[13] != 0, i.hot_geometry = in[14] != 0, i.out_span_ok = in[15] != 0;
  i.planes_floats = (size_t)in[16], i.k_cached = in[17] != 0, i.plane_nt_opt = (int)in[18], i.frame_major_opt = (int)in[19];
  i.stagger_us = (int)in[20], i.prefetch = in[21] != 0, i.k_prefetch = (int)in[22];
  const LaunchDecision L = launch_decide(i);
  out[0] = L.form, out[1] = L.variant, out[2] = L.grid, out[3] = L.chunk, out[4] = L.patch_blocks, out[5] = L.stagger_ticks, out[6] = L.stagger_blocks;
  out[7] = L.sum_first, out[8] = L.frame_major, out[9] = L.plane_nt, out[10] = L.rows, out[11] = L.head_patches, out[12] = L.prefetch;
  out[13] = L.k_prefetch, out[14] = L.sum_queue_draws;
  for (int x = 0; x < 8; ++x) out[15 + x] = L.xq_draws[x];
  out[23] = patch_launch_too_large(i.N, i.n_patches, i.frames) ? 1 : 0;
}
extern "C" int emu_launch_chunk(int N, int n_patches) { return chunk_patches(n_patches, patch_teams(N)); }
extern "C" int emu_launch_teams(int N) { return patch_teams(N); }
