// CPU lane emulator for rpsf_core_stars_render.hpp (test infrastructure, never shipped in the product path).
// Runs S10 as csrc/stars.hip launches it (rpsf_stars_render): the host's tile lists, then each() loops over the threads of a workgroup
// and the workgroups run one after the other.  The LDS of every workgroup is exactly s10_lds_bytes() and starts with garbage; the
// per-thread register of the kernel is one double per thread of the workgroup, garbage as well.  The output is written only where the
// kernel writes it.
// With -DEMU_RENDER_MAIN the file is a stand-alone program (for a sanitizer build of the driver, the lists and the LDS carve): a small
// frame with partial tiles, stars on and off it, skipped ones, more than a chunk on one tile, every mode and both dtypes; it returns 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_stars_render.hpp"

using namespace rpsfn;

namespace {
struct CpuCtx {
  int threads;
  std::vector<double> regs;
  explicit CpuCtx(int n) : threads(n), regs((size_t)n, -777.0) {}
  double& reg(int t) { return regs[(size_t)t]; }
  template <class F>
  void each(F&& f) {
    for (int t = 0; t < threads; ++t) f(t);
  }
};
long launches = 0;

int check(int H, int W, long n_cells, int N, long n, const double* positions, double radius, int mode) {
  if (H <= 0 || W <= 0 || n < 0 || n_cells < 1 || !model_size_ok(N)) return -1;
  if (render_problem(radius, mode) || !(radius <= max_fit_radius(N))) return -1;
  for (long i = 0; i < n; ++i)
    if (!position_ok(positions[2 * i], positions[2 * i + 1])) return -1;
  return 0;
}
}  // namespace

// info[5] = the tile's rows, its columns, the chunk's records, the workgroups the last emurd_render ran, S10's LDS bytes
extern "C" void emurd_info(long* info) {
  info[0] = RENDER_TILE_R, info[1] = RENDER_TILE_C, info[2] = RENDER_CHUNK, info[3] = launches, info[4] = (long)s10_lds_bytes();
}

// The host's tile lists as rpsf_stars_render builds them.  offsets takes tiles + 1 entries; index takes up to `room` entries.  Returns
// the length of the index array (copy nothing into `index` when it is above `room`), -1 where the library returns RPSF_E_BADARG.
extern "C" long emurd_lists(int H, int W, long n_cells, int N, long n, const double* positions, const double* flux, const int* cells,
                            double radius, long long* offsets, int* index, long room, long* n_rendered) {
  if (check(H, W, n_cells, N, n, positions, radius, MODE_MODEL) != 0) return -1;
  std::vector<long long> off;
  std::vector<int> idx;
  const size_t drawn = tile_lists(H, W, (size_t)n, positions, flux, cells, (int)n_cells, radius, off, idx);
  if (n_rendered) *n_rendered = (long)drawn;
  std::memcpy(offsets, off.data(), off.size() * sizeof(long long));
  if ((long)idx.size() <= room && !idx.empty()) std::memcpy(index, idx.data(), idx.size() * sizeof(int));
  return (long)idx.size();
}

// rpsf_stars_render after a rpsf_stars_background_host: `L` is the filtered mesh S1b left (not read unless mode == 2), `none` its flag.
// Returns -1 where the library returns RPSF_E_BADARG and -6 where it returns RPSF_E_STATE (mode 2 on a frame without a usable pixel);
// out takes H x W float32 or float64.  The mask is not read: masks enter only through the mesh.
extern "C" int emurd_render(const float* img, int H, int W, int box, const double* L, int none, long n_cells, int N, const double* cube,
                            long n, const double* positions, const double* flux, const int* cells, double radius, int mode, int out_f64,
                            void* out, long* n_rendered) {
  launches = 0;
  if (box < MIN_BOX || box > MAX_BOX || check(H, W, n_cells, N, n, positions, radius, mode) != 0) return -1;
  if (mode == MODE_RESIDUAL_MESH && none) return -6;
  std::vector<long long> offsets;
  std::vector<int> index;
  const size_t drawn = tile_lists(H, W, (size_t)n, positions, flux, cells, (int)n_cells, radius, offsets, index);
  if (n_rendered) *n_rendered = (long)drawn;
  const Frame fr{img, nullptr, H, W, box, (H + box - 1) / box, (W + box - 1) / box};
  const Model model{cube, (int)n_cells, N};
  const Render rd = make_render(radius, mode, out_f64, N);
  const Stars st{positions, flux, cells, offsets.data(), index.data()};
  std::vector<char> lds(s10_lds_bytes());
  for (long t = 0; t < tiles_down(H); ++t)
    for (long u = 0; u < tiles_across(W); ++u) {
      std::memset(lds.data(), 0x5A, lds.size());
      CpuCtx ctx(WALK_THREADS);
      s10_render(ctx, fr, L, model, rd, st, (int)t, (int)u, lds.data(), out);
      ++launches;
    }
  return 0;
}

#if defined(EMU_RENDER_MAIN)
int main() {
  const int H = 21, W = 45, box = 16, nby = 2, nbx = 3, N = 9, n_cells = 2;
  std::vector<float> img((size_t)H * W);
  for (int r = 0; r < H; ++r)
    for (int c = 0; c < W; ++c) img[(size_t)r * W + c] = (float)(10.0 + 0.1 * r - 0.05 * c);
  const std::vector<double> L((size_t)nby * nbx, 10.0);
  std::vector<double> cube((size_t)n_cells * N * N, 0.25);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) cube[(size_t)i * N + j] = std::exp(-((i - 4.0) * (i - 4.0) + (j - 4.0) * (j - 4.0)) / 4.5);
  std::vector<double> pos = {10.0, 20.0, 7.5, 31.5, -100.0, -100.0, 0.0, 0.0, 20.0, 44.0, 23.9, 10.2, 5.0, 5.0, 8.0, 32.0};
  std::vector<double> flux = {100.0, 50.0, 10.0, 20.0, 30.0, 40.0, NAN, INFINITY};
  std::vector<int> cells = {0, 1, 0, 0, 1, 0, 0, 1};
  cells.push_back(2), pos.push_back(3.0), pos.push_back(3.0), flux.push_back(1.0);  // a cell outside the model
  for (int i = 0; i < 2 * RENDER_CHUNK + 1; ++i) {  // more than two chunks on one tile
    pos.push_back(12.0 + 0.01 * i), pos.push_back(40.0 - 0.01 * i), flux.push_back(1.0 + i), cells.push_back(i % 2);
  }
  const long n = (long)flux.size();
  for (double radius : {1.0, 2.5, 3.5})
    for (int mode : {MODE_MODEL, MODE_RESIDUAL, MODE_RESIDUAL_MESH})
      for (int f64 : {0, 1}) {
        std::vector<char> out((size_t)H * W * (f64 ? 8 : 4));
        long drawn = -1;
        if (emurd_render(img.data(), H, W, box, L.data(), 0, n_cells, N, cube.data(), n, pos.data(), flux.data(), cells.data(), radius, mode, f64,
                         out.data(), &drawn) != 0)
          return 1;
        if (drawn != n - 3) return 2;
      }
  std::vector<long long> offsets((size_t)(tiles_down(H) * tiles_across(W)) + 1);
  std::vector<int> index(1 << 16);
  long drawn = -1;
  const long entries = emurd_lists(H, W, n_cells, N, n, pos.data(), flux.data(), cells.data(), 3.5, offsets.data(), index.data(), (long)index.size(), &drawn);
  std::printf("emu_render: %ld stars, %ld drawn, %ld list entries, %ld LDS bytes\n", n, drawn, entries, (long)s10_lds_bytes());
  return entries > 0 && entries == offsets.back() ? 0 : 3;
}
#endif
