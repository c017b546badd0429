// rpsf_core_stars_render.hpp - model and residual frames from fitted stars (DESIGN.md 3.7 "Model and residual frames", S10), shared with the
// CPU lane emulator tests/emu/emu_render.cpp.  A driver over a context as in rpsf_core_stars.hpp, and the host's tile lists beside it.
//
//   S10 s10_render   one workgroup per tile of RENDER_TILE_R x RENDER_TILE_C output pixels, one pixel per thread: the stars on the tile's
//                    list are staged into LDS RENDER_CHUNK records (row, col, flux, cell) at a time, and every pixel adds flux x model_at
//                    of the stars whose disc holds it, in ascending star index, into one float64 register
//
// It GATHERS: a pixel is written by one thread, once, and the order of its sum is the order of the list, not of the hardware.  It reads
// the finder's frame and filtered mesh, the star records, the tile lists and the cube, and writes the output frame and nothing else.  No
// atomics at all, no workgroup waits for another.  Two runs on one input agree bit for bit.  This is NOT a PSF-photometry package's
// subtraction: the interpolation is bilinear and does not conserve flux below the pixel scale, the disc cuts the model at R, and a
// per-star fitted background is not subtracted.
#pragma once
#include <cstdint>
#include <vector>

#include "rpsf_core_stars_fit.hpp"

#pragma clang fp contract(off)

namespace rpsfn {
using namespace rpsff;

constexpr int RENDER_TILE_R = 8, RENDER_TILE_C = 32, RENDER_CHUNK = 64;
static_assert(RENDER_TILE_R * RENDER_TILE_C == WALK_THREADS, "one pixel per thread");
static_assert(RENDER_CHUNK <= WALK_THREADS, "a chunk is staged by one thread per record");
enum { MODE_MODEL = 0, MODE_RESIDUAL = 1, MODE_RESIDUAL_MESH = 2 };

struct Render {
  double R, R2, h;  // the radius of the disc, R R, and the star's centre in the cell: N / 2.0 - 0.5
  int mode, out_f64;
};
// the stars of a call as the host uploaded them, and the tile lists: offsets[t] .. offsets[t + 1] of `index` are tile t's stars, ascending
struct Stars {
  const double* pos;   // (row, col) per star
  const double* flux;
  const int* cell;
  const long long* offsets;
  const int* index;
};

// what is wrong with the radius or the mode, as far as it can be said without the model (null: nothing)
inline const char* render_problem(double radius, int mode) {
  if (!(radius > 0.0) || !(radius <= MAX_RADIUS)) return "radius must lie in 0 < R <= min(64, N / 2 - 1)";
  if (mode != MODE_MODEL && mode != MODE_RESIDUAL && mode != MODE_RESIDUAL_MESH) return "mode must be 0 (model), 1 (residual) or 2 (residual against the mesh)";
  return nullptr;
}
inline Render make_render(double radius, int mode, int out_f64, int N) { return Render{radius, radius * radius, N / 2.0 - 0.5, mode, out_f64 != 0}; }
// a star is drawn when its flux is finite and its cell is one of the model's
inline bool star_rendered(double flux, int cell, int n_cells) { return finite_d(flux) && cell >= 0 && cell < n_cells; }
RPSFS_HD long tiles_down(int H) { return ((long)H + RENDER_TILE_R - 1) / RENDER_TILE_R; }
RPSFS_HD long tiles_across(int W) { return ((long)W + RENDER_TILE_C - 1) / RENDER_TILE_C; }

// THE TILE LISTS, on the host.  Star i is on the list of every tile that S8's box floor(row - R) - 1 .. ceil(row + R) + 1 (likewise in
// columns), clipped to the frame, meets; a star that is not drawn (star_rendered) or whose box misses the frame is on no list.  Tiles in
// raster order, the stars of a tile in ascending index.  Returns the number of stars that are drawn, on the frame or off it.
inline size_t tile_lists(int H, int W, size_t n, const double* pos, const double* flux, const int* cell, int n_cells, double R,
                         std::vector<long long>& offsets, std::vector<int>& index) {
  const long ty = tiles_down(H), tx = tiles_across(W);
  offsets.assign((size_t)(ty * tx) + 1, 0);
  struct Span {
    int t0, t1, u0, u1;  // tile rows t0 .. t1 and tile columns u0 .. u1; t0 > t1: none
  };
  std::vector<Span> spans(n);
  size_t rendered = 0;
  for (size_t i = 0; i < n; ++i) {
    spans[i] = Span{1, 0, 1, 0};
    if (!star_rendered(flux[i], cell[i], n_cells)) continue;
    ++rendered;
    const double y = pos[2 * i], x = pos[2 * i + 1];
    const DiscBox box = disc_box(y, x, R);  // (the caller has checked position_ok: the box is far from an int's range)
    long r0 = box.r0, r1 = box.r1, c0 = box.c0, c1 = box.c1;
    if (r0 < 0) r0 = 0;
    if (c0 < 0) c0 = 0;
    if (r1 > H - 1) r1 = H - 1;
    if (c1 > W - 1) c1 = W - 1;
    if (r0 > r1 || c0 > c1) continue;
    spans[i] = Span{(int)(r0 / RENDER_TILE_R), (int)(r1 / RENDER_TILE_R), (int)(c0 / RENDER_TILE_C), (int)(c1 / RENDER_TILE_C)};
    for (long t = spans[i].t0; t <= spans[i].t1; ++t)
      for (long u = spans[i].u0; u <= spans[i].u1; ++u) ++offsets[(size_t)(t * tx + u) + 1];
  }
  for (size_t t = 0; t < (size_t)(ty * tx); ++t) offsets[t + 1] += offsets[t];
  index.assign((size_t)offsets.back(), 0);
  std::vector<long long> next(offsets.begin(), offsets.end() - 1);
  for (size_t i = 0; i < n; ++i)
    for (long t = spans[i].t0; t <= spans[i].t1; ++t)
      for (long u = spans[i].u0; u <= spans[i].u1; ++u) index[(size_t)next[(size_t)(t * tx + u)]++] = (int)i;
  return rendered;
}

// ------------------------------------------------------------------------------------------------ the chunk in LDS
// RENDER_CHUNK records, field-major: the rows, the columns, the fluxes (float64), then the cells (int32)
RPSFS_HD constexpr size_t s10_lds_bytes() { return (size_t)RENDER_CHUNK * (3 * 8 + 4); }
static_assert(s10_lds_bytes() % 16 == 0, "the chunk is a whole number of 16-byte words");

// One workgroup, the tile (tile_r, tile_c); thread t has pixel (tile_r RENDER_TILE_R + t / RENDER_TILE_C, tile_c RENDER_TILE_C + t %
// RENDER_TILE_C) and the register ctx.reg(t), s = 0.0 at first.  The tile's list is walked in chunks: the first threads stage one record
// each, then every thread whose pixel (r, c) lies on the frame takes the chunk's records in order: pr = r - row, pc = c - col, q = pr pr +
// pc pc, and when q <= R R: s += flux * model_at(cell).  Every thread takes part in every barrier, whether its pixel is on the frame or
// not: the trip count is the tile's, the same for all.  Then out[p] = s (MODEL), (double)img[p] - s (RESIDUAL) or ((double)img[p] -
// background_at) - s (RESIDUAL_MESH), rounded once to float32 unless out_f64.
template <class Ctx>
RPSFS_HD void s10_render(Ctx& ctx, const Frame& fr, const double* L, const Model& model, const Render& rd, const Stars& st, int tile_r,
                         int tile_c, void* lds, void* out) {
  double* s_row = static_cast<double*>(lds);
  double* s_col = s_row + RENDER_CHUNK;
  double* s_flux = s_col + RENDER_CHUNK;
  int* s_cell = reinterpret_cast<int*>(s_flux + RENDER_CHUNK);
  const long tile = (long)tile_r * tiles_across(fr.W) + tile_c;
  const long long begin = st.offsets[tile], end = st.offsets[tile + 1];
  const int N = model.N;
  const size_t cell_words = (size_t)N * N;
  ctx.each([&](int tid) { ctx.reg(tid) = 0.0; });
  for (long long k = begin; k < end; k += RENDER_CHUNK) {
    const int len = end - k < RENDER_CHUNK ? (int)(end - k) : RENDER_CHUNK;
    ctx.each([&](int tid) {
      if (tid >= len) return;
      const int i = st.index[k + tid];
      s_row[tid] = st.pos[2 * (size_t)i], s_col[tid] = st.pos[2 * (size_t)i + 1], s_flux[tid] = st.flux[i], s_cell[tid] = st.cell[i];
    });
    ctx.each([&](int tid) {
      const int r = tile_r * RENDER_TILE_R + tid / RENDER_TILE_C, c = tile_c * RENDER_TILE_C + tid % RENDER_TILE_C;
      if (r >= fr.H || c >= fr.W) return;
      double s = ctx.reg(tid);
      for (int j = 0; j < len; ++j) {
        const double pr = (double)r - s_row[j], pc = (double)c - s_col[j];
        const double q = pr * pr + pc * pc;
        if (!(q <= rd.R2)) continue;
        s += s_flux[j] * model_at(model.cube + (size_t)s_cell[j] * cell_words, N, rd.h, pr, pc);
      }
      ctx.reg(tid) = s;
    });
  }
  ctx.each([&](int tid) {
    const int r = tile_r * RENDER_TILE_R + tid / RENDER_TILE_C, c = tile_c * RENDER_TILE_C + tid % RENDER_TILE_C;
    if (r >= fr.H || c >= fr.W) return;
    const size_t p = (size_t)r * fr.W + c;
    const double s = ctx.reg(tid);
    double v = s;
    if (rd.mode == MODE_RESIDUAL) {
      v = (double)fr.img[p] - s;
    } else if (rd.mode == MODE_RESIDUAL_MESH) {
      const Mesh mesh{L, fr.nbx, 0, 0};
      v = ((double)fr.img[p] - background_at(fr, mesh, r, c)) - s;
    }
    if (rd.out_f64)
      static_cast<double*>(out)[p] = v;
    else
      static_cast<float*>(out)[p] = (float)v;
  });
}

}  // namespace rpsfn
