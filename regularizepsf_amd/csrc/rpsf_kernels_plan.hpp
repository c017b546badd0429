// rpsf_kernels_plan.hpp - the plain (non-template) kernels that a plan's launch path needs beside the patch kernels: the tile sum alone,
// K5, K5' and the three kernels of the hipFFT fallback.  Defined in exactly one unit, the one that launches them: csrc/rpsf.hip, which
// includes this after rpsf_device.hpp (TileSum, sum_tiles_worker, sum_planes_at, ImageView / OutView: rpsf_kernels.hpp).
#pragma once

__global__ __launch_bounds__(256) void sum_tiles_kernel(TileSum p) { sum_tiles_worker(p, blockIdx.x, gridDim.x); }

// ------------------------------------------------------------------------------------------------
// K5: out = sum of the colour planes that have a patch over the pixel (fixed order: deterministic)
// ------------------------------------------------------------------------------------------------
struct SumParams {
  const float* planes;
  size_t plane_stride;
  float* out;
  int rows, W, ld_planes, ld_out;
  int row_begin;       // first window row this launch sums
  int row0;            // full-image row of window row 0
  int lat_r0, lat_c0;  // full-image coordinates of lattice tile (0, 0)
  int half_shift;      // log2(N/2)
  int nti, ntj;
  const uint8_t* cover;  // nti x ntj, 4-bit class masks
  size_t planes_frame_floats, out_frame_floats;  // batch: frame f (= blockIdx.y) at planes + f*..., out + f*...
};

__device__ __forceinline__ int cover_at(const SumParams& p, int y, int x) {
  int ty = (y - p.lat_r0) >> p.half_shift, tx = (x - p.lat_c0) >> p.half_shift;
  if (y < p.lat_r0 || x < p.lat_c0 || ty >= p.nti || tx >= p.ntj) return 0;
  return p.cover[ty * p.ntj + tx];
}

__device__ __forceinline__ bool sum_vector_ok(const SumParams& p) {
  return ((p.ld_planes | p.ld_out) & 3) == 0 &&
         ((reinterpret_cast<uintptr_t>(p.planes) | reinterpret_cast<uintptr_t>(p.out) | (p.plane_stride * 4)) & 15) == 0;
}
// Branch-free 16-byte read of plane k: a plane without a patch over the tile is never read (its content is
// stale) - the load is redirected to one always-valid line and its result discarded.  Keeping the loads
// unconditional matters: a load under a branch is waited for at the join, which serialises the four planes.
__device__ __forceinline__ float4 load_plane4(const SumParams& p, int k, size_t off, int cov) {
  const bool on = (cov >> k) & 1;
  const float* src = on ? p.planes + k * p.plane_stride + off : p.planes;
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 a = __builtin_nontemporal_load(reinterpret_cast<const f4*>(src));
  return make_float4(on ? a.x : 0.f, on ? a.y : 0.f, on ? a.z : 0.f, on ? a.w : 0.f);
}
__device__ __forceinline__ void store_out4(float* o, float4 v) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, reinterpret_cast<f4*>(o));
}

// four consecutive pixels (x .. x+3) of window row yl
__device__ __forceinline__ void sum_planes_group(const SumParams& p, int yl, int x, bool vector_ok) {
  int y = yl + p.row0;
  size_t off = (size_t)yl * p.ld_planes + x;
  float* o = p.out + (size_t)yl * p.ld_out + x;
  int c0 = cover_at(p, y, x), c3 = cover_at(p, y, x + 3);
  if (vector_ok && x + 3 < p.W && c0 == c3) {  // one tile, aligned: four 16-byte loads, one 16-byte store
    float4 a0 = load_plane4(p, 0, off, c0), a1 = load_plane4(p, 1, off, c0), a2 = load_plane4(p, 2, off, c0),
           a3 = load_plane4(p, 3, off, c0);
    store_out4(o, make_float4(((a0.x + a1.x) + a2.x) + a3.x, ((a0.y + a1.y) + a2.y) + a3.y,
                              ((a0.z + a1.z) + a2.z) + a3.z, ((a0.w + a1.w) + a2.w) + a3.w));
  } else {
    for (int i = 0; i < 4 && x + i < p.W; ++i) o[i] = sum_planes_at(p.planes, p.plane_stride, off + i, cover_at(p, y, x + i));
  }
}

__global__ void sum_planes_kernel(SumParams p) {
  p.planes += (size_t)blockIdx.y * p.planes_frame_floats;
  p.out += (size_t)blockIdx.y * p.out_frame_floats;
  const unsigned groups = (unsigned)(p.W + 3) >> 2;
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)groups * p.rows) return;
  const bool small = (size_t)groups * p.rows < ((size_t)1 << 32);
  const int yl = small ? (int)((unsigned)idx / groups) : (int)(idx / groups);
  const int xg = small ? (int)((unsigned)idx % groups) : (int)(idx % groups);
  sum_planes_group(p, yl + p.row_begin, xg * 4, sum_vector_ok(p));
}

// ------------------------------------------------------------------------------------------------
// K5': fix-up after a direct overlap-add launch.  FIX_SUB workgroups per lattice tile; most exit at once.
//   out_tile = (tile initialised by its direct contributors ? out_tile : 0) + sum of the colour planes that hold a
//   side contribution (static: contributors of another chunk; dynamic: demoted at run time), in colour order.
// Tiles without any contributor are zeroed (the reference leaves uncovered output at 0, transform.py:167-169).
// ------------------------------------------------------------------------------------------------
struct FixParams {
  const float* planes;
  size_t plane_stride, planes_frame_floats;
  int ld_planes;
  float* out;
  int ld_out;
  size_t out_frame_floats;
  int rows, W, row0;           // resident output window: rows [row0, row0 + rows) of the image, W columns
  int lat_r0, lat_c0, half;    // full-image coordinates of lattice tile (0, 0); tile edge
  int ntj;
  const uint8_t* tile_info;    // bits 0-3 static side mask, bit 4 tile has contributors
  const uint32_t* flags;
  const uint32_t* dyn_side;
  uint32_t epoch, n_tiles;
};
constexpr int FIX_SUB = 8;

__global__ __launch_bounds__(256) void fixup_kernel(FixParams p) {
  const uint32_t tile = blockIdx.x / FIX_SUB, sub = blockIdx.x % FIX_SUB, frame = blockIdx.y;
  const uint32_t d = p.dyn_side[(size_t)frame * p.n_tiles + tile], f = p.flags[(size_t)frame * p.n_tiles + tile];
  const uint32_t side = (p.tile_info[tile] & 15u) | ((d >> 8) == p.epoch ? (d & 15u) : 0u);
  const bool init = (f >> 8) == p.epoch && (f & 8u);
  if (side == 0 && init) return;
  const int ti = tile / p.ntj, tj = tile % p.ntj;
  const int span = (p.half + FIX_SUB - 1) / FIX_SUB;
  const int ty0 = p.lat_r0 + ti * p.half + (int)sub * span;
  const int y0 = max(ty0, p.row0), y1 = min(min(ty0 + span, p.lat_r0 + (ti + 1) * p.half), p.row0 + p.rows);
  const int x0 = max(p.lat_c0 + tj * p.half, 0), x1 = min(p.lat_c0 + (tj + 1) * p.half, p.W);
  if (y0 >= y1 || x0 >= x1) return;
  const float* planes = p.planes + (size_t)frame * p.planes_frame_floats;
  float* out = p.out + (size_t)frame * p.out_frame_floats;
  const bool vec = ((x0 | x1 | p.ld_planes | p.ld_out) & 3) == 0 && (p.plane_stride & 3) == 0 &&
                   ((reinterpret_cast<uintptr_t>(planes) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  typedef float f4 __attribute__((ext_vector_type(4)));
  if (vec) {
    const int gw = (x1 - x0) >> 2, total = gw * (y1 - y0);
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
      const int yl = y0 + i / gw - p.row0, x = x0 + ((i % gw) << 2);
      f4* o = reinterpret_cast<f4*>(out + (size_t)yl * p.ld_out + x);
      const f4* pl = reinterpret_cast<const f4*>(planes + (size_t)yl * p.ld_planes + x);
      f4 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)  // unconditional loads (redirected to plane 0's line when unused) so they overlap
        v[k] = __builtin_nontemporal_load(((side >> k) & 1) ? pl + k * (p.plane_stride >> 2) : pl);
      f4 acc = init ? *o : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((side >> k) & 1) acc += v[k];
      *o = acc;
    }
  } else {
    const int w = x1 - x0, total = w * (y1 - y0);
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
      const int yl = y0 + i / w - p.row0, x = x0 + i % w;
      float* o = out + (size_t)yl * p.ld_out + x;
      const float* pl = planes + (size_t)yl * p.ld_planes + x;
      float acc = init ? *o : 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((side >> k) & 1) acc += pl[k * p.plane_stride];
      *o = acc;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// hipFFT fallback (any patch size without a plan): gather, multiply, scatter
// ------------------------------------------------------------------------------------------------
struct GenericGeom {
  int N, first, count;         // patches [first, first + count) of the plan
  int origin_row, origin_col;
  ImageView im;
  OutView ov;
};
// one thread per (patch, r, c) of the chunk
__global__ void generic_gather_kernel(GenericGeom gg, const int32_t* __restrict__ coords, const float* __restrict__ win,
                                      cf* __restrict__ buf) {
  const size_t per = (size_t)gg.N * gg.N;
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= per * gg.count) return;
  const int k = (int)(idx / per), rem = (int)(idx % per), r = rem / gg.N, c = rem % gg.N;
  const int y = pad_index(coords[2 * (gg.first + k)] + gg.origin_row + r, gg.im.H, gg.im.pad_mode);
  const int x = pad_index(coords[2 * (gg.first + k) + 1] + gg.origin_col + c, gg.im.W, gg.im.pad_mode);
  const float px = (y < 0 || x < 0) ? gg.im.pad_value : gg.im.img[(size_t)(y - gg.im.row0) * gg.im.ld + x];
  buf[idx] = cf{px * (win[r] * win[c]), 0.0f};
}
__global__ void generic_multiply_kernel(cf* __restrict__ buf, const cf* __restrict__ k, size_t count, float scale) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) buf[i] = cmul(buf[i], k[i]) * scale;
}
// `colour` < 0: every patch of the chunk, atomic adds (any corner list).  `colour` 0 .. 3: only the patches of that colour class, which do not
// overlap one another (rpsf.hip generic_colours), with plain read-add-write: the four passes of a chunk run one after the other on the
// stream, so every pixel receives its contributions in a fixed order and the fallback is bit-reproducible like the compiled sizes.
__global__ void generic_scatter_kernel(GenericGeom gg, const int32_t* __restrict__ coords, const float* __restrict__ win,
                                       const cf* __restrict__ buf, const uint8_t* __restrict__ colours, int colour) {
  const size_t per = (size_t)gg.N * gg.N;
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= per * gg.count) return;
  const int k = (int)(idx / per), rem = (int)(idx % per), r = rem / gg.N, c = rem % gg.N;
  if (colour >= 0 && colours[gg.first + k] != colour) return;
  const int y = coords[2 * (gg.first + k)] + gg.origin_row + r, x = coords[2 * (gg.first + k) + 1] + gg.origin_col + c;
  if (y < 0 || y >= gg.ov.H || x < 0 || x >= gg.ov.W) return;  // the crop of transform.py:174-177
  float* dst = gg.ov.out + (size_t)(y - gg.ov.row0) * gg.ov.ld + x;
  const float v = buf[idx].x * (win[r] * win[c]);
  if (colour >= 0) *dst += v;
  else unsafeAtomicAdd(dst, v);
}
