// CPU lane emulator for rpsf_core_builder_sub.hpp (test infrastructure, never shipped in the product path).
// Runs kernel B1n thread by thread with a phase boundary wherever builder_patch_sub_kernel has a barrier, on the same LDS layout: phase 1n
// (the chunked neighbour sums and the gather), then B1's own phases as tests/emu/emu_builder.cpp runs them.  The neighbour lists are the
// product's host code, called as the library calls it.
// With -DEMU_BUILDER_SUB_MAIN it is a program with a main of its own (for the host sanitizers): it reads a case file, writes the flags, the
// patches and the lists.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_builder_sub.hpp"

using namespace rpsfb;

// the lists alone: offsets[n_patches + 1]; at most `capacity` entries of `index` are written; returns the total, or -1
extern "C" long long emubn_lists(int H, int W, int N, int n_patches, const int32_t* corners, const int32_t* own, int n_all, const double* pos,
                                 const double* flux, const int32_t* cell, int n_cells, double R, long long* offsets, int32_t* index,
                                 long long capacity) {
  if (N < MIN_N || N > MAX_N || H < 2 || W < 2 || n_patches < 0 || n_all < 0) return -1;
  std::vector<long long> off;
  std::vector<int> idx;
  rpsfbn::neighbour_lists(H, W, N, (size_t)n_patches, corners, own, (size_t)n_all, pos, flux, cell, n_cells, R, off, idx);
  for (size_t k = 0; k < off.size(); ++k) offsets[k] = off[k];
  for (size_t k = 0; k < idx.size() && (long long)k < capacity; ++k) index[k] = idx[k];
  return (long long)idx.size();
}

// B1n on given lists (any superset in ascending order must do)
extern "C" int emubn_patches(int N, const float* img, int H, int W, const double* cube, int model_n, const double* pos, const double* flux,
                             const int32_t* cell, double R, int n_stars, const long long* offsets, const int32_t* index,
                             const int32_t* corners, const double* frac, double saturation, double star_minimum, double star_maximum,
                             float* patches, uint8_t* flags) {
  if (N < MIN_N || N > MAX_N || H < 2 || W < 2) return -1;
  const int T = threads_for(N);
  std::vector<double> lds(rpsfbn::lds_bytes(N) / sizeof(double) + 1);
  std::vector<double> regs((size_t)T * MAX_PPT);
  const rpsfbn::Sub sub{cube, model_n, R * R, model_n / 2.0 - 0.5, pos, flux, cell, offsets, index};
  for (int star = 0; star < n_stars; ++star) {
    for (double& x : lds) x = std::nan("");  // nothing may depend on what the previous star left
    const Lds s = carve(lds.data(), N);
    const rpsfbn::Chunk chunk = rpsfbn::carve_chunk(lds.data(), N);
    const int rr = corners[2 * star], rc = corners[2 * star + 1];
    float* out = patches + (size_t)star * N * N;
    const bool nobody = offsets[star] == offsets[star + 1];  // B1's own gather, as the kernel takes it
    for (int t = 0; t < T; ++t) {
      b1_tables(t, N, frac[2 * star], frac[2 * star + 1], s);
      if (nobody)
        b1_gather(t, T, N, img, H, W, rr, rc, s);
      else
        rpsfbn::b1n_begin(t, T, N, s);
    }
    for (long long at = offsets[star]; at < offsets[star + 1]; at += rpsfbn::CHUNK) {
      const int len = offsets[star + 1] - at < rpsfbn::CHUNK ? (int)(offsets[star + 1] - at) : rpsfbn::CHUNK;
      for (int t = 0; t < T; ++t) rpsfbn::b1n_stage(t, sub, at, len, chunk);
      for (int t = 0; t < T; ++t) rpsfbn::b1n_add(t, T, N, H, W, rr, rc, sub, len, chunk, s);
    }
    if (!nobody)
      for (int t = 0; t < T; ++t) rpsfbn::b1n_gather(t, T, N, img, H, W, rr, rc, s);
    for (int axis = 0; axis < 2; ++axis)
      for (int t = 0; t < T; ++t) b1_prefilter(t, N, axis, s);
    for (int axis = 0; axis < 2; ++axis) {
      for (int t = 0; t < T; ++t) b1_taps_read(t, T, N, axis, s, &regs[(size_t)t * MAX_PPT]);
      for (int t = 0; t < T; ++t) b1_taps_write(t, T, N, s, &regs[(size_t)t * MAX_PPT]);
    }
    for (int t = 0; t < T; ++t) b1_scan(t, T, N, s);
    for (int t = 0; t < T; ++t) b1_plane(t, N, s);
    for (int t = 0; t < T; ++t) b1_finish(t, T, N, saturation, s, out);
    flags[star] = b1_verdict(N, star_minimum, star_maximum, s);
  }
  return 0;
}

#if defined(EMU_BUILDER_SUB_MAIN)
// in:  int64 N, H, W, n_cells, model_n, n_all, n_stars; float64 R, saturation, star_minimum, star_maximum; float32 img[H W]; float64
//      cube[n_cells model_n^2], pos[2 n_all], flux[n_all]; int32 cell[n_all], own[n_stars], corners[2 n_stars]; float64 frac[2 n_stars]
// out: uint8 flags[n_stars]; float32 patches[n_stars N^2]; int64 offsets[n_stars + 1]; int32 index[offsets[n_stars]]
template <class T>
static bool take(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int64_t> head;
  std::vector<double> par, cube, pos, flux, frac;
  std::vector<float> img;
  std::vector<int32_t> cell, own, corners;
  bool ok = take(f, head, 7) && take(f, par, 4);
  if (!ok) return 3;
  const int N = (int)head[0], H = (int)head[1], W = (int)head[2], n_cells = (int)head[3], model_n = (int)head[4], n_all = (int)head[5],
            n_stars = (int)head[6];
  ok = take(f, img, (size_t)H * W) && take(f, cube, (size_t)n_cells * model_n * model_n) && take(f, pos, 2 * (size_t)n_all) &&
       take(f, flux, (size_t)n_all) && take(f, cell, (size_t)n_all) && take(f, own, (size_t)n_stars) && take(f, corners, 2 * (size_t)n_stars) &&
       take(f, frac, 2 * (size_t)n_stars);
  std::fclose(f);
  if (!ok) return 3;
  std::vector<long long> offsets((size_t)n_stars + 1);
  std::vector<int32_t> index((size_t)n_stars * (size_t)n_all + 1);
  const long long total = emubn_lists(H, W, N, n_stars, corners.data(), own.data(), n_all, pos.data(), flux.data(), cell.data(), n_cells, par[0],
                                      offsets.data(), index.data(), (long long)index.size());
  if (total < 0) return 4;
  std::vector<float> patches((size_t)n_stars * N * N, std::nanf(""));  // what phase 5 does not write stays NaN
  std::vector<uint8_t> flags((size_t)n_stars);
  if (emubn_patches(N, img.data(), H, W, cube.data(), model_n, pos.data(), flux.data(), cell.data(), par[0], n_stars, offsets.data(), index.data(),
                    corners.data(), frac.data(), par[1], par[2], par[3], patches.data(), flags.data()) != 0)
    return 4;
  std::FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 2;
  std::vector<int64_t> off64(offsets.begin(), offsets.end());
  std::fwrite(flags.data(), 1, flags.size(), g);
  std::fwrite(patches.data(), sizeof(float), patches.size(), g);
  std::fwrite(off64.data(), sizeof(int64_t), off64.size(), g);
  std::fwrite(index.data(), sizeof(int32_t), (size_t)total, g);
  std::fclose(g);
  std::printf("%d patches, %lld list entries\n", n_stars, total);
  return 0;
}
#endif
