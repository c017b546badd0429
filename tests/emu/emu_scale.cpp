// CPU lane emulator for rpsf_core_scale.hpp (test infrastructure, never shipped in the product path).
// Runs the launches of rpsf_detail_scale_run (csrc/scale.hip) in their order - line kernel on the columns, transpose, line kernel on the
// rows, transpose - workgroup by workgroup and thread by thread, with a phase boundary where scale_transpose_kernel has its barrier, on
// buffers of exactly the sizes the library reserves; and kernel B4 pixel by pixel.  So the pivot table, the sweeps, the evaluation, the
// tile index algebra and the block mean are checked against SciPy and NumPy without a GPU.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_scale.hpp"

using namespace rpsfs;

namespace {
template <class Tout>
void transpose(long rows, long cols, const double* in, Tout* out) {
  std::vector<double> tile((size_t)TILE * TILE_LD);
  for (long tr = 0; tr < (rows + TILE - 1) / TILE; ++tr)
    for (long tc = 0; tc < (cols + TILE - 1) / TILE; ++tc) {
      for (double& x : tile) x = std::nan("");  // nothing may depend on what the previous tile left
      for (int tid = 0; tid < TILE * TILE_ROWS; ++tid) t_load(tid, tr, tc, rows, cols, in, tile.data());
      for (int tid = 0; tid < TILE * TILE_ROWS; ++tid) t_store(tid, tr, tc, rows, cols, tile.data(), out);
    }
}

template <class T>
void lines(long lanes, int m, int s, const T* y, const double* ip, double* work, double* out) {
  const long launched = (lanes + LINE_THREADS - 1) / LINE_THREADS * LINE_THREADS;  // the idle lanes of the last workgroup run too
  for (long lane = 0; lane < launched; ++lane) u_line(lane, lanes, m, s, y, ip, work, out);
}

template <class T, class Tout>
int upscale(const T* image, int H, int W, int s, Tout* out) {
  if (H < MIN_LINE || W < MIN_LINE || s < 2) return -1;
  const long hs = scaled(H, s), ws = scaled(W, s);
  const int longest = H > W ? H : W;
  std::vector<double> ip((size_t)longest - 4 + 1), rows((size_t)hs * W), turned((size_t)hs * W), cols((size_t)hs * ws),
      work((size_t)(H > hs ? H : hs) * W, std::nan(""));
  pivot_table(longest, ip.data());
  lines(W, H, s, image, ip.data(), work.data(), rows.data());
  transpose(hs, W, rows.data(), turned.data());
  for (double& x : work) x = std::nan("");
  lines(hs, W, s, turned.data(), ip.data(), work.data(), cols.data());
  transpose(ws, hs, cols.data(), out);
  return 0;
}
}  // namespace

extern "C" int emus_pivots(int m, double* ip) {
  if (m < MIN_LINE) return -1;
  pivot_table(m, ip);
  return 0;
}

extern "C" int emus_upscale(const void* image, int is_f64, int H, int W, int s, void* out, int out_is_f32) {
  if (is_f64)
    return out_is_f32 ? upscale(static_cast<const double*>(image), H, W, s, static_cast<float*>(out))
                      : upscale(static_cast<const double*>(image), H, W, s, static_cast<double*>(out));
  return out_is_f32 ? upscale(static_cast<const float*>(image), H, W, s, static_cast<float*>(out))
                    : upscale(static_cast<const float*>(image), H, W, s, static_cast<double*>(out));
}

extern "C" int emus_block_mean(const double* cells, int n_cells, int N, int s, double* out) {
  if (N < 1 || s < 1 || n_cells < 0) return -1;
  for (int cell = 0; cell < n_cells; ++cell)
    for (int pixel = 0; pixel < N * N; ++pixel)
      out[(size_t)cell * N * N + pixel] = b4_pixel(cells + (size_t)cell * (N * s) * (N * s), N, s, pixel);
  return 0;
}
