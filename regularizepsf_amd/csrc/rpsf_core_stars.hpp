// rpsf_core_stars.hpp - the star finder (csrc/stars.hip), shared with the CPU lane emulator tests/emu/emu_stars.cpp.
//
// Workgroup kernels are written as DRIVERS over a context: `ctx.each(f)` runs f(tid) for every thread of the workgroup and then
// a barrier.  On the GPU every thread runs the driver, each() is `f(threadIdx.x); __syncthreads();`; the emulator runs the driver
// once and each() loops over the threads.  Everything a driver keeps between two each() calls is computed from LDS words that
// all threads read alike, so the one copy of the emulator and the per-thread copies of the GPU hold the same values.
// Grid kernels without barriers are plain per-thread functions of the global thread index.
//
//   S1  s1_box       one workgroup per background box: sigma-clipped median / mean / sd (exact median by bisection on float32 keys in LDS)
//   S2  s2_tile      one workgroup per TILE_R x TILE_C tile: residual d = pixel - bilinear background, 3 x 3 filter, test against T
//   S3  s3_tile, s3_seam, s3_flatten     labels = smallest linear index of the 8-connected component
//   S4  s4_count, s4_scan, s4_roots, s4_init, s4_accumulate, s4_walk     roots in index order, area / bounding box, moments
//
// All arithmetic on values is float64; sums run in a fixed order (per thread in index order, then 16 x 16 resp. 8 x 8 trees),
// the only atomics are integer min / max / add.  Two runs on one input agree bit for bit.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RPSFS_HD __host__ __device__ __forceinline__
#else
#define RPSFS_HD inline
#endif

// the sums below are compared with NumPy's at 1e-12: no fused multiply-adds the source does not spell out
#pragma clang fp contract(off)

namespace rpsfs {

constexpr int MIN_BOX = 8, MAX_BOX = 128;
constexpr int S1_THREADS = 256;
constexpr int MAX_ROUNDS = 16;
constexpr int TILE_R = 32, TILE_C = 32, TILE_THREADS = 256;  // S2 and S3 work on the same tiles
constexpr int HALO_C = TILE_C + 2, HALO_N = (TILE_R + 2) * (TILE_C + 2);
constexpr int MESH_W = 8;  // a tile with its halo spans at most 34 / 8 + 3 mesh nodes per axis
constexpr int SEAM_SLOTS = TILE_C + 2 * TILE_R;  // first row, first column and last column of a tile
constexpr int SEG = 64;  // S4: pixels per row segment
constexpr int SCAN_THREADS = 1024;
constexpr int WALK_THREADS = 256, WALK_LANES = 64, WALK_WAVES = WALK_THREADS / WALK_LANES;

// ------------------------------------------------------------------------------------------------ integer atomics
#if defined(__HIP_DEVICE_COMPILE__)
RPSFS_HD int load_relaxed(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
RPSFS_HD int fetch_min(int* p, int v) { return atomicMin(p, v); }
RPSFS_HD int fetch_max(int* p, int v) { return atomicMax(p, v); }
RPSFS_HD int fetch_add(int* p, int v) { return atomicAdd(p, v); }
#else
RPSFS_HD int load_relaxed(const int* p) { return *p; }
RPSFS_HD int fetch_min(int* p, int v) { const int o = *p; if (v < o) *p = v; return o; }
RPSFS_HD int fetch_max(int* p, int v) { const int o = *p; if (v > o) *p = v; return o; }
RPSFS_HD int fetch_add(int* p, int v) { const int o = *p; *p = o + v; return o; }
#endif

// ------------------------------------------------------------------------------------------------ shared pieces
// order-preserving map of the finite floats onto unsigned integers; NO_KEY marks a pixel that is not usable
constexpr unsigned NO_KEY = 0xFFFFFFFFu, MAX_KEY = 0xFF7FFFFFu;
RPSFS_HD unsigned key_of(float x) {
  unsigned u;
  std::memcpy(&u, &x, 4);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
RPSFS_HD double value_of(unsigned k) {
  const unsigned u = (k >> 31) ? (k & 0x7FFFFFFFu) : ~k;
  float x;
  std::memcpy(&x, &u, 4);
  return (double)x;
}
RPSFS_HD bool finite_f(float x) { return std::fabs(x) <= 3.40282346638528859812e38f; }
RPSFS_HD bool usable(const float* img, const uint8_t* mask, size_t p) { return finite_f(img[p]) && !mask[p]; }

// the bilinear background surface along one axis: nodes i0, i1 and the weight t of i1 for pixel index r
RPSFS_HD void axis_coord(int r, int box, int nb, int& i0, int& i1, double& t) {
  double u = ((double)r + 0.5) / (double)box - 0.5;
  if (u < 0.0) u = 0.0;
  if (u > (double)(nb - 1)) u = (double)(nb - 1);
  const int lim = nb - 2 > 0 ? nb - 2 : 0;
  const int f = (int)std::floor(u);
  i0 = f < lim ? f : lim;
  t = nb == 1 ? 0.0 : u - (double)i0;
  i1 = i0 + 1 < nb - 1 ? i0 + 1 : nb - 1;
}

struct Frame {
  const float* img;
  const uint8_t* mask;  // 1: ignore
  int H, W, box, nby, nbx;
};

// mesh[(i - oi) * ld + (j - oj)] is node (i, j): the whole mesh in global memory (oi = oj = 0, ld = nbx) or a tile's window of it in LDS
struct Mesh {
  const double* L;
  int ld, oi, oj;
  RPSFS_HD double at(int i, int j) const { return L[(i - oi) * ld + (j - oj)]; }
};

RPSFS_HD double background_at(const Frame& fr, const Mesh& m, int r, int c) {
  int i0, i1, j0, j1;
  double t, s;
  axis_coord(r, fr.box, fr.nby, i0, i1, t);
  axis_coord(c, fr.box, fr.nbx, j0, j1, s);
  return (1.0 - t) * ((1.0 - s) * m.at(i0, j0) + s * m.at(i0, j1)) + t * ((1.0 - s) * m.at(i1, j0) + s * m.at(i1, j1));
}
// the residual: pixel - background on usable pixels, 0 elsewhere
RPSFS_HD double residual_at(const Frame& fr, const Mesh& m, int r, int c) {
  const size_t p = (size_t)r * fr.W + c;
  return usable(fr.img, fr.mask, p) ? (double)fr.img[p] - background_at(fr, m, r, c) : 0.0;
}

// ------------------------------------------------------------------------------------------------ S1
struct Part {  // what one thread, or one group of 16, contributes to a pass over the box
  double d;
  unsigned c, lo, hi, pad;
};
RPSFS_HD Part fold16(const Part* p) {  // in index order
  Part r{0.0, 0u, NO_KEY, 0u, 0u};
  for (int j = 0; j < 16; ++j) {
    r.d += p[j].d;
    r.c += p[j].c;
    if (p[j].lo < r.lo) r.lo = p[j].lo;
    if (p[j].hi > r.hi) r.hi = p[j].hi;
  }
  return r;
}
// S1's LDS: box * box keys, then the Part records.  A Part holds a double, and box * box keys of an odd box end 4 bytes off an 8-byte
// boundary: the records start at the next multiple of 16 bytes.
constexpr size_t S1_RECORDS = S1_THREADS + 16;
RPSFS_HD size_t s1_part_offset(int box) { return ((size_t)box * box * sizeof(unsigned) + 15) & ~(size_t)15; }
RPSFS_HD size_t s1_lds_bytes(int box) { return s1_part_offset(box) + S1_RECORDS * sizeof(Part); }

enum { PASS_SUM, PASS_SSD, PASS_BELOW, PASS_NEXT, PASS_CLIP };
struct Kept {  // the kept set is the keys in [lo, hi]
  unsigned lo, hi;
  double mean, med, sd;
};
// one thread's share of a pass: samples tid, tid + 256, ... of the box
RPSFS_HD Part s1_partial(int tid, int cnt, const unsigned* keys, int pass, const Kept& k, unsigned arg) {
  Part r{0.0, 0u, NO_KEY, 0u, 0u};
  for (int p = tid; p < cnt; p += S1_THREADS) {
    const unsigned key = keys[p];
    if (key < k.lo || key > k.hi) continue;
    const double v = value_of(key);
    switch (pass) {
      case PASS_SUM:
        r.d += v, r.c += 1;
        if (key < r.lo) r.lo = key;
        if (key > r.hi) r.hi = key;
        break;
      case PASS_SSD: r.d += (v - k.mean) * (v - k.mean); break;
      case PASS_BELOW: r.c += key < arg; break;
      case PASS_NEXT:
        if (key <= arg) r.c += 1;
        else if (key < r.lo) r.lo = key;
        break;
      default:
        if (std::fabs(v - k.med) <= 3.0 * k.sd) {
          r.c += 1;
          if (key < r.lo) r.lo = key;
          if (key > r.hi) r.hi = key;
        }
    }
  }
  return r;
}

// Box (bi, bj) of the lattice.  `lds` holds s1_lds_bytes(box).
template <class Ctx>
RPSFS_HD void s1_box(Ctx& ctx, const Frame& fr, int bi, int bj, void* lds, double* level, double* rms) {
  unsigned* keys = static_cast<unsigned*>(lds);
  Part* part = reinterpret_cast<Part*>(static_cast<char*>(lds) + s1_part_offset(fr.box));
  Part* part2 = part + S1_THREADS;
  const int r0 = bi * fr.box, c0 = bj * fr.box;
  const int bh = (fr.H - r0 < fr.box ? fr.H - r0 : fr.box), bw = (fr.W - c0 < fr.box ? fr.W - c0 : fr.box);
  const int cnt = bh * bw;
  ctx.each([&](int tid) {
    for (int p = tid; p < cnt; p += S1_THREADS) {
      const size_t g = (size_t)(r0 + p / bw) * fr.W + c0 + p % bw;
      keys[p] = usable(fr.img, fr.mask, g) ? key_of(fr.img[g]) : NO_KEY;
    }
  });
  Kept k{0u, MAX_KEY, 0.0, 0.0, 0.0};
  auto reduce = [&](int pass, unsigned arg) -> Part {
    ctx.each([&](int tid) { part[tid] = s1_partial(tid, cnt, keys, pass, k, arg); });
    ctx.each([&](int tid) {
      if (tid < 16) part2[tid] = fold16(part + 16 * tid);
    });
    return fold16(part2);  // read by everybody before the next pass's second barrier lets part2 change
  };
  const double nan = std::nan("");
  double out_level = nan, out_rms = nan;
  for (int round = 0;; ++round) {
    Part s = reduce(PASS_SUM, 0u);
    const unsigned n = s.c;
    if (n == 0) break;
    k.mean = s.d / (double)n;
    k.lo = s.lo, k.hi = s.hi;  // the same set, bounded by its own extremes
    s = reduce(PASS_SSD, 0u);
    k.sd = std::sqrt(s.d / (double)n);
    // the (n - 1) / 2-th smallest key is the largest T with |{key < T}| <= (n - 1) / 2, built bit by bit below the bits all kept keys share
    const unsigned kth = (n - 1) / 2;
    int top = 31;
    while (top >= 0 && !(((k.lo ^ k.hi) >> top) & 1u)) --top;
    unsigned ans = top == 31 ? 0u : (k.lo >> (top + 1)) << (top + 1);
    for (int bit = top; bit >= 0; --bit) {
      const unsigned trial = ans | (1u << bit);
      if (reduce(PASS_BELOW, trial).c <= kth) ans = trial;
    }
    const double a = value_of(ans);
    k.med = a;
    if (n % 2 == 0) {
      s = reduce(PASS_NEXT, ans);
      const double b = s.c >= kth + 2 ? a : value_of(s.lo);
      k.med = (a + b) / 2.0;
    }
    out_level = (k.sd == 0.0 || std::fabs(k.mean - k.med) >= 0.3 * k.sd) ? k.med : 2.5 * k.med - 1.5 * k.mean;
    out_rms = k.sd;
    if (round == MAX_ROUNDS || k.sd == 0.0) break;
    s = reduce(PASS_CLIP, 0u);
    if (s.c == n) break;
    k.lo = s.lo, k.hi = s.hi;  // v -> fl(v - med) is monotone: what is kept is again an interval of values
  }
  ctx.each([&](int tid) {
    if (tid == 0) level[bi * fr.nbx + bj] = out_level, rms[bi * fr.nbx + bj] = out_rms;
  });
}

// ------------------------------------------------------------------------------------------------ S2
RPSFS_HD size_t s2_lds_bytes() { return (size_t)(HALO_N + MESH_W * MESH_W) * sizeof(double); }

// The filter [[1,2,1],[2,4,2],[1,2,1]] / 16 at halo position (hr, hc).  The order of the additions: per row
// h = (left + 2 centre) + right, then f = ((h(above) + 2 h(centre)) + h(below)) / 16; the products by 2 and the division are exact.
RPSFS_HD double s2_filter(const double* dl, int hr, int hc) {
  double h[3];
  for (int k = 0; k < 3; ++k) {
    const double* row = dl + (hr - 1 + k) * HALO_C + hc;
    h[k] = (row[-1] + 2.0 * row[0]) + row[1];
  }
  return ((h[0] + 2.0 * h[1]) + h[2]) / 16.0;
}

// Tile (ty, tx): det[p] = 1 where the filtered residual exceeds T on a usable pixel.  `L` is the whole filtered mesh.  `fout`, when given,
// takes the filtered residual of every pixel: the bits the threshold saw, for the deblend option (rpsf_core_stars_deblend.hpp).
template <class Ctx>
RPSFS_HD void s2_tile(Ctx& ctx, const Frame& fr, const double* L, double T, int ty, int tx, void* lds, uint8_t* det, double* fout = nullptr) {
  double* dl = static_cast<double*>(lds);
  double* mw = dl + HALO_N;
  const int r0 = ty * TILE_R, c0 = tx * TILE_C;
  const int ra = r0 > 0 ? r0 - 1 : 0, rb = r0 + TILE_R < fr.H - 1 ? r0 + TILE_R : fr.H - 1;
  const int ca = c0 > 0 ? c0 - 1 : 0, cb = c0 + TILE_C < fr.W - 1 ? c0 + TILE_C : fr.W - 1;
  int wi0, wi1, wj0, wj1, unused;
  double tt;
  axis_coord(ra, fr.box, fr.nby, wi0, unused, tt);
  axis_coord(rb, fr.box, fr.nby, unused, wi1, tt);
  axis_coord(ca, fr.box, fr.nbx, wj0, unused, tt);
  axis_coord(cb, fr.box, fr.nbx, unused, wj1, tt);
  ctx.each([&](int tid) {
    const int i = wi0 + tid / MESH_W, j = wj0 + tid % MESH_W;
    if (tid < MESH_W * MESH_W && i <= wi1 && j <= wj1) mw[tid] = L[(size_t)i * fr.nbx + j];
  });
  const Mesh window{mw, MESH_W, wi0, wj0};
  ctx.each([&](int tid) {
    for (int p = tid; p < HALO_N; p += TILE_THREADS) {
      const int r = r0 - 1 + p / HALO_C, c = c0 - 1 + p % HALO_C;
      dl[p] = (r >= 0 && r < fr.H && c >= 0 && c < fr.W) ? residual_at(fr, window, r, c) : 0.0;  // zeros outside the frame
    }
  });
  ctx.each([&](int tid) {
    for (int p = tid; p < TILE_R * TILE_C; p += TILE_THREADS) {
      const int lr = p / TILE_C, lc = p % TILE_C, r = r0 + lr, c = c0 + lc;
      if (r >= fr.H || c >= fr.W) continue;
      const size_t g = (size_t)r * fr.W + c;
      const double f = s2_filter(dl, lr + 1, lc + 1);
      det[g] = (f > T && usable(fr.img, fr.mask, g)) ? 1 : 0;
      if (fout) fout[g] = f;
    }
  });
}

// ------------------------------------------------------------------------------------------------ S3
// Union-find on an array of parents, parent <= child always: every walk towards a root strictly descends and every failed link
// continues from a strictly smaller node, so each loop ends whatever the other threads do; nobody waits for anybody.
RPSFS_HD int uf_find(const int* parent, int x) {
  for (;;) {
    const int p = load_relaxed(parent + x);
    if (p == x) return x;
    x = p;
  }
}
RPSFS_HD void uf_unite(int* parent, int a, int b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b, b = t;
    }
    const int old = fetch_min(parent + a, b);  // a > b
    if (old == a) return;                      // a was still a root: linked
    a = old;                                   // somebody linked a first (old < a): its former parent and b remain to be united
  }
}

// Tile (ty, tx): labels[p] = smallest linear index of p's component WITHIN the tile, -1 off the mask.  `ll`: TILE_R * TILE_C ints of LDS.
template <class Ctx>
RPSFS_HD void s3_tile(Ctx& ctx, const uint8_t* det, int H, int W, int ty, int tx, int* ll, int32_t* labels) {
  const int r0 = ty * TILE_R, c0 = tx * TILE_C;
  ctx.each([&](int tid) {
    for (int p = tid; p < TILE_R * TILE_C; p += TILE_THREADS) {
      const int r = r0 + p / TILE_C, c = c0 + p % TILE_C;
      ll[p] = (r < H && c < W && det[(size_t)r * W + c]) ? p : -1;
    }
  });
  ctx.each([&](int tid) {
    for (int p = tid; p < TILE_R * TILE_C; p += TILE_THREADS) {
      if (ll[p] < 0) continue;
      const int lr = p / TILE_C, lc = p % TILE_C;
      if (lc > 0 && ll[p - 1] >= 0) uf_unite(ll, p, p - 1);
      if (lr > 0) {
        if (lc > 0 && ll[p - TILE_C - 1] >= 0) uf_unite(ll, p, p - TILE_C - 1);
        if (ll[p - TILE_C] >= 0) uf_unite(ll, p, p - TILE_C);
        if (lc < TILE_C - 1 && ll[p - TILE_C + 1] >= 0) uf_unite(ll, p, p - TILE_C + 1);
      }
    }
  });
  ctx.each([&](int tid) {
    for (int p = tid; p < TILE_R * TILE_C; p += TILE_THREADS) {
      const int r = r0 + p / TILE_C, c = c0 + p % TILE_C;
      if (r >= H || c >= W) continue;
      int label = -1;
      if (ll[p] >= 0) {
        const int root = uf_find(ll, p);  // raster order inside the tile is raster order in the frame
        label = (r0 + root / TILE_C) * W + c0 + root % TILE_C;
      }
      labels[(size_t)r * W + c] = label;
    }
  });
}

// Thread gid of the seam pass: pixel `slot` of tile gid / SEAM_SLOTS, united with its left, upper-left, upper and upper-right
// neighbours that lie in another tile.  (Inside a tile every such pair was united by s3_tile.)
RPSFS_HD void s3_seam(long gid, int H, int W, int32_t* labels) {
  const int tiles_x = (W + TILE_C - 1) / TILE_C, tiles_y = (H + TILE_R - 1) / TILE_R;
  const long tile = gid / SEAM_SLOTS;
  const int slot = (int)(gid % SEAM_SLOTS);
  if (tile >= (long)tiles_x * tiles_y) return;
  const int ty = (int)(tile / tiles_x), tx = (int)(tile % tiles_x);
  int lr, lc;
  if (slot < TILE_C) lr = 0, lc = slot;
  else if (slot < TILE_C + TILE_R) lr = slot - TILE_C, lc = 0;
  else lr = slot - TILE_C - TILE_R, lc = TILE_C - 1;
  const int r = ty * TILE_R + lr, c = tx * TILE_C + lc;
  if (r >= H || c >= W) return;
  const int p = r * W + c;
  if (labels[p] < 0) return;
  const int dr[4] = {0, -1, -1, -1}, dc[4] = {-1, -1, 0, 1};
  for (int k = 0; k < 4; ++k) {
    const int qr = r + dr[k], qc = c + dc[k];
    if (qr < 0 || qc < 0 || qc >= W) continue;
    if (qr / TILE_R == ty && qc / TILE_C == tx) continue;
    const int q = qr * W + qc;
    if (labels[q] >= 0) uf_unite(labels, p, q);
  }
}

RPSFS_HD void s3_flatten(long gid, long npix, int32_t* labels) {
  if (gid >= npix) return;
  const int l = labels[gid];
  if (l >= 0) labels[gid] = uf_find(labels, l);
}

// ------------------------------------------------------------------------------------------------ S4
RPSFS_HD int segs_per_row(int W) { return (W + SEG - 1) / SEG; }

// roots (labels[p] == p) of row segment `seg`: counted, then written in index order from segoff[seg] on
RPSFS_HD void s4_count(long seg, int H, int W, const int32_t* labels, int* segcnt) {
  const int spr = segs_per_row(W);
  if (seg >= (long)H * spr) return;
  const int r = (int)(seg / spr), c0 = (int)(seg % spr) * SEG, c1 = c0 + SEG < W ? c0 + SEG : W;
  int n = 0;
  for (int c = c0; c < c1; ++c) n += labels[(size_t)r * W + c] == r * W + c;
  segcnt[seg] = n;
}
RPSFS_HD void s4_roots(long seg, int H, int W, const int32_t* labels, const int* segoff, int* roots) {
  const int spr = segs_per_row(W);
  if (seg >= (long)H * spr) return;
  const int r = (int)(seg / spr), c0 = (int)(seg % spr) * SEG, c1 = c0 + SEG < W ? c0 + SEG : W;
  int at = segoff[seg];
  for (int c = c0; c < c1; ++c)
    if (labels[(size_t)r * W + c] == r * W + c) roots[at++] = r * W + c;
}
// one workgroup of SCAN_THREADS: exclusive prefix sums of segcnt into segoff, the total into *total.  `lds`: SCAN_THREADS + 32 ints.
template <class Ctx>
RPSFS_HD void s4_scan(Ctx& ctx, long nseg, const int* segcnt, int* segoff, int* total, int* lds) {
  int* part = lds;
  int* part2 = lds + SCAN_THREADS;
  const long chunk = (nseg + SCAN_THREADS - 1) / SCAN_THREADS;
  ctx.each([&](int tid) {
    int n = 0;
    for (long i = tid * chunk; i < (tid + 1) * chunk && i < nseg; ++i) n += segcnt[i];
    part[tid] = n;
  });
  ctx.each([&](int tid) {
    if (tid >= 32) return;
    int n = 0;
    for (int j = 0; j < 32; ++j) n += part[32 * tid + j];
    part2[tid] = n;
  });
  ctx.each([&](int tid) {
    int run = 0;
    for (int g = 0; g < tid / 32; ++g) run += part2[g];
    for (int j = 32 * (tid / 32); j < tid; ++j) run += part[j];
    if (tid == SCAN_THREADS - 1) *total = run + part[tid];
    for (long i = tid * chunk; i < (tid + 1) * chunk && i < nseg; ++i) {
      segoff[i] = run;
      run += segcnt[i];
    }
  });
}

// per component k (root roots[k]): stats[4k ..] = area, last row, first column, last column; the first row is the root's
RPSFS_HD void s4_init(long k, long count, int W, const int* roots, int* stats) {
  if (k >= count) return;
  const int root = roots[k];
  stats[4 * k] = 0, stats[4 * k + 1] = root / W, stats[4 * k + 2] = stats[4 * k + 3] = root % W;
}
RPSFS_HD long s4_slot(const int* roots, long count, int root) {  // roots ascend
  long lo = 0, hi = count - 1;
  while (lo < hi) {
    const long mid = (lo + hi) / 2;
    if (roots[mid] < root) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
RPSFS_HD void s4_accumulate(long gid, long npix, int W, const int32_t* labels, const int* roots, long count, int* stats) {
  if (gid >= npix) return;
  const int l = labels[gid];
  if (l < 0) return;
  const long k = s4_slot(roots, count, l);
  fetch_add(stats + 4 * k, 1);
  fetch_max(stats + 4 * k + 1, (int)(gid / W));
  fetch_min(stats + 4 * k + 2, (int)(gid % W));
  fetch_max(stats + 4 * k + 3, (int)(gid % W));
}

RPSFS_HD size_t s4_walk_lds_bytes() { return (size_t)(WALK_THREADS + WALK_WAVES * 8) * 3 * sizeof(double); }

// One workgroup, WALK_WAVES components from `first` on, one wave each: lane j takes pixels j, j + 64, ... of the bounding box in raster
// order and sums d, d * row, d * col over those of the component; the 64 partial sums fold as 8 groups of 8, each in lane order.
// moments[4k ..] = sum d, sum d * row, sum d * col, area; a component outside [min_area, max_area] is not walked and gets zeros.
template <class Ctx>
RPSFS_HD void s4_walk(Ctx& ctx, const Frame& fr, const double* L, const int32_t* labels, const int* roots, const int* stats, long count,
                      long min_area, long max_area, long first, double* lds, double* moments) {
  double* acc = lds;
  double* acc2 = lds + WALK_THREADS * 3;
  const Mesh mesh{L, fr.nbx, 0, 0};
  auto wanted = [&](long k) { return k < count && stats[4 * k] >= min_area && (max_area < 0 || stats[4 * k] <= max_area); };
  ctx.each([&](int tid) {
    const long k = first + tid / WALK_LANES;
    const int lane = tid % WALK_LANES;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (wanted(k)) {
      const int root = roots[k], r0 = root / fr.W, c0 = stats[4 * k + 2];
      const long bw = stats[4 * k + 3] - c0 + 1, npx = (long)(stats[4 * k + 1] - r0 + 1) * bw;
      for (long j = lane; j < npx; j += WALK_LANES) {
        const int r = r0 + (int)(j / bw), c = c0 + (int)(j % bw);
        if (labels[(size_t)r * fr.W + c] != root) continue;
        const double d = residual_at(fr, mesh, r, c);
        s0 += d, s1 += d * (double)r, s2 += d * (double)c;
      }
    }
    acc[3 * tid] = s0, acc[3 * tid + 1] = s1, acc[3 * tid + 2] = s2;
  });
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES, lane = tid % WALK_LANES;
    if (lane >= 8) return;
    for (int m = 0; m < 3; ++m) {
      double s = 0.0;
      for (int j = 0; j < 8; ++j) s += acc[3 * (wave * WALK_LANES + 8 * lane + j) + m];
      acc2[3 * (wave * 8 + lane) + m] = s;
    }
  });
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES;
    const long k = first + wave;
    if (tid % WALK_LANES != 0 || k >= count) return;
    for (int m = 0; m < 3; ++m) {
      double s = 0.0;
      for (int j = 0; j < 8; ++j) s += acc2[3 * (wave * 8 + j) + m];
      moments[4 * k + m] = s;
    }
    moments[4 * k + 3] = (double)stats[4 * k];
  });
}

}  // namespace rpsfs
