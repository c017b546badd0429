// rpsf_core_convert.hpp - device-array views (rpsf_view, include/rpsf.h): the zero-copy predicate, the argument checks and the per-thread
// bodies of the two conversion kernels, in plain C++ so that tests/emu/emu_convert.cpp runs on the CPU what csrc/convert.hip runs on the GPU.
//
//   C1 (gather and convert): any supported dtype at any positive byte strides -> a dense float32 frame.
//   C2 (convert and scatter): a dense float32 frame -> float32 / float64 / float16 at any positive byte strides; rows x cols elements are
//       written and nothing between them.
//
// WORK: the dense side is cut, as one flat array of rows x cols floats, into chunks of E elements, E = max(4, 16 / item size) - 4 for the
// 4- and 8-byte types, 8 for the 2-byte ones, 16 for uint8 - so that a whole chunk is 16 bytes (or a multiple) on either side.  A thread takes
// chunks tid, tid + threads, ... (grid-stride); every address is 64-bit.  A whole chunk moves by 16-byte accesses on the dense side when the
// dense base is 16-byte aligned (the plan's staging always is), and on the strided side when strided_vec() holds: col_stride == item size,
// base, row_stride (and the frame stride of a stack) multiples of 16 bytes, cols a multiple of E (a chunk then lies in one row and starts on
// a 16-byte boundary).  Everything else - the last, short chunk included - goes element by element (byte by byte where the strided side's
// pointer or strides are no multiples of the item size).
// CONVERSIONS: float32 moves as its 32 bits (denormals and NaN payloads survive); integers as (float)(double)v; float64 by the C cast in
// both directions; float16 in integer arithmetic, round to nearest even, on the CPU and the GPU alike.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/rpsf.h"

#if defined(__HIPCC__)
#define RPSFV_HD __host__ __device__ __forceinline__
#else
#define RPSFV_HD inline
#endif

namespace rpsfconv {

constexpr int MAX_WORKGROUPS = 2048, WG = 256;  // the grid-stride launch: at most this many workgroups of WG threads per frame

RPSFV_HD int item_size(int dtype) {
  switch (dtype) {
    case RPSF_DTYPE_FLOAT32: case RPSF_DTYPE_INT32: return 4;
    case RPSF_DTYPE_FLOAT64: return 8;
    case RPSF_DTYPE_FLOAT16: case RPSF_DTYPE_INT16: case RPSF_DTYPE_UINT16: return 2;
    case RPSF_DTYPE_UINT8: return 1;
    default: return 0;
  }
}
RPSFV_HD int chunk_elems(int dtype) { return item_size(dtype) >= 4 ? 4 : 16 / item_size(dtype); }

// ---------------------------------------------------------------------------------------------------------------- predicates (host)
// null: fine; else what is wrong with the view.  *empty: nothing to do.  An output is float32, float64 or float16.
inline const char* view_problem(const rpsf_view* v, bool output, bool* empty) {
  *empty = false;
  if (!v) return "null view";
  const int item = item_size(v->dtype);
  if (item == 0) return "unknown dtype";
  if (output && v->dtype != RPSF_DTYPE_FLOAT32 && v->dtype != RPSF_DTYPE_FLOAT64 && v->dtype != RPSF_DTYPE_FLOAT16)
    return "an output view is float32, float64 or float16";
  if (v->rows < 0 || v->cols < 0) return "negative shape";
  if (v->row_stride <= 0 || v->col_stride <= 0) return "strides must be positive";
  *empty = v->rows == 0 || v->cols == 0;
  if (*empty) return nullptr;
  if (!v->data) return "null data";
  return nullptr;
}

// THE ZERO-COPY PREDICATE: the view is what rpsf_geometry's ld_image / ld_out describe - float32, unit column step, a row stride that is
// a multiple of 4 bytes, at least a row long and an int's worth of floats, a pointer aligned as a float
inline bool zero_copy(const rpsf_view& v) {
  return v.dtype == RPSF_DTYPE_FLOAT32 && v.col_stride == 4 && v.row_stride % 4 == 0 && v.row_stride >= 4 * (int64_t)v.cols &&
         v.row_stride / 4 <= (int64_t)0x7FFFFFFF && reinterpret_cast<uintptr_t>(v.data) % 4 == 0;
}
inline bool dense_f32(const rpsf_view& v) { return zero_copy(v) && v.row_stride == 4 * (int64_t)v.cols; }  // what the saturation entry points take

// ---------------------------------------------------------------------------------------------------------------- kernel arguments
struct Args {
  char* strided;           // element (f, r, c) at strided + f * frame_stride + r * row_stride + c * col_stride (bytes)
  float* dense;            // element (f, r, c) at dense[f * dense_frame_stride + r * cols + c]
  int64_t frame_stride, row_stride, col_stride, dense_frame_stride;
  int rows, cols;
  int strided_vec, dense_vec;  // whole chunks by 16-byte accesses on that side
  int elem_aligned;            // the strided side's base and strides are multiples of the item size (else its elements move byte by byte)
};

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
inline Args make_args(const rpsf_view& v, int frames, int64_t frame_stride, float* dense, int64_t dense_frame_stride) {
  const int E = chunk_elems(v.dtype);
  Args a{static_cast<char*>(v.data), dense, frame_stride, v.row_stride, v.col_stride, dense_frame_stride, v.rows, v.cols, 0, 0, 0};
  const int item = item_size(v.dtype);
  a.elem_aligned = reinterpret_cast<uintptr_t>(v.data) % (uintptr_t)item == 0 && v.row_stride % item == 0 && v.col_stride % item == 0 &&
                   (frames == 1 || frame_stride % item == 0);
  a.strided_vec = v.col_stride == item_size(v.dtype) && aligned16(v.data) && v.row_stride % 16 == 0 && v.cols % E == 0 && (frames == 1 || frame_stride % 16 == 0);
  a.dense_vec = aligned16(dense) && (frames == 1 || dense_frame_stride % 4 == 0);
  return a;
}
inline int64_t chunks_of(const Args& a, int E) { return ((int64_t)a.rows * a.cols + E - 1) / E; }
inline unsigned workgroups_for(int64_t chunks) {
  const int64_t wgs = (chunks + WG - 1) / WG;
  return (unsigned)(wgs < 1 ? 1 : wgs > MAX_WORKGROUPS ? MAX_WORKGROUPS : wgs);
}

// ---------------------------------------------------------------------------------------------------------------- element conversions
RPSFV_HD uint32_t float_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
RPSFV_HD float bits_float(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// IEEE binary16 -> binary32, exact
RPSFV_HD uint32_t half_to_float_bits(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 31u;
  uint32_t sig = h & 0x3FFu;
  if (exp == 31u) return sign | 0x7F800000u | (sig << 13);  // inf, NaN (payload kept)
  if (exp != 0u) return sign | ((exp + 112u) << 23) | (sig << 13);
  if (sig == 0u) return sign;
  int e = 113;  // denormal: normalise
  while (!(sig & 0x400u)) sig <<= 1, --e;
  return sign | ((uint32_t)e << 23) | ((sig & 0x3FFu) << 13);
}

// IEEE binary32 -> binary16, round to nearest even; overflow to inf, underflow through the denormals to zero; NaN stays NaN (quiet)
RPSFV_HD uint16_t float_bits_to_half(uint32_t f) {
  const uint16_t sign = (uint16_t)((f >> 16) & 0x8000u);
  const uint32_t mag = f & 0x7FFFFFFFu;
  if (mag >= 0x7F800000u) return (uint16_t)(sign | (mag > 0x7F800000u ? 0x7E00u | ((mag >> 13) & 0x3FFu) : 0x7C00u));
  if (mag >= 0x47800000u) return (uint16_t)(sign | 0x7C00u);  // 2^16 and above; what rounds up to 2^16 carries into it below
  if (mag < 0x33000000u) return sign;                          // below 2^-25: zero (2^-25 itself is the halfway case to the even 0)
  if (mag < 0x38800000u) {  // below 2^-14: a half denormal, last place 2^-24 = the 24-bit significand shifted right by 126 - exponent
    const uint32_t sig = 0x00800000u | (mag & 0x007FFFFFu);
    const uint32_t shift = 126u - (mag >> 23);  // 14 ... 24
    const uint32_t kept = sig >> shift, rest = sig & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    return (uint16_t)(sign | (kept + (rest > half || (rest == half && (kept & 1u)) ? 1u : 0u)));
  }
  const uint32_t kept = (mag - 0x38000000u) >> 13, rest = mag & 0x1FFFu;  // exponent and significand in place: a carry runs into the exponent
  return (uint16_t)(sign | (kept + (rest > 0x1000u || (rest == 0x1000u && (kept & 1u)) ? 1u : 0u)));
}

template <class T> struct Elem;  // to_bits: the element as the bits of its float32; from_bits: the other way (outputs only)
template <> struct Elem<float> {
  using Raw = uint32_t;
  static RPSFV_HD uint32_t to_bits(Raw v) { return v; }
  static RPSFV_HD Raw from_bits(uint32_t b) { return b; }
};
template <> struct Elem<double> {
  using Raw = double;
  static RPSFV_HD uint32_t to_bits(Raw v) { return float_bits((float)v); }
  static RPSFV_HD Raw from_bits(uint32_t b) { return (double)bits_float(b); }
};
struct Half {};
template <> struct Elem<Half> {
  using Raw = uint16_t;
  static RPSFV_HD uint32_t to_bits(Raw v) { return half_to_float_bits(v); }
  static RPSFV_HD Raw from_bits(uint32_t b) { return float_bits_to_half(b); }
};
template <class I> struct IntElem {
  using Raw = I;
  static RPSFV_HD uint32_t to_bits(Raw v) { return float_bits((float)(double)v); }
};
template <> struct Elem<uint8_t> : IntElem<uint8_t> {};
template <> struct Elem<int16_t> : IntElem<int16_t> {};
template <> struct Elem<uint16_t> : IntElem<uint16_t> {};
template <> struct Elem<int32_t> : IntElem<int32_t> {};

struct alignas(16) V16 {
  uint32_t w[4];
};

// one element of the strided side: a plain access where it is aligned to its size, byte by byte elsewhere
template <class Raw>
RPSFV_HD Raw load_elem(const char* p, int aligned) {
  if (aligned) return *reinterpret_cast<const Raw*>(p);
  Raw v;
  unsigned char b[sizeof(Raw)];
  for (int i = 0; i < (int)sizeof(Raw); ++i) b[i] = static_cast<unsigned char>(p[i]);
  __builtin_memcpy(&v, b, sizeof(Raw));
  return v;
}
template <class Raw>
RPSFV_HD void store_elem(char* p, Raw v, int aligned) {
  if (aligned) {
    *reinterpret_cast<Raw*>(p) = v;
    return;
  }
  unsigned char b[sizeof(Raw)];
  __builtin_memcpy(b, &v, sizeof(Raw));
  for (int i = 0; i < (int)sizeof(Raw); ++i) p[i] = static_cast<char>(b[i]);
}

// ---------------------------------------------------------------------------------------------------------------- the thread bodies
// C1: thread `tid` of `threads` on frame `frame`
template <class T>
RPSFV_HD void c1_thread(const Args& a, int64_t tid, int64_t threads, int frame) {
  using Raw = typename Elem<T>::Raw;
  constexpr int E = sizeof(Raw) >= 4 ? 4 : 16 / (int)sizeof(Raw);
  const int64_t total = (int64_t)a.rows * a.cols, chunks = (total + E - 1) / E;
  const char* src = a.strided + (int64_t)frame * a.frame_stride;
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.dense + (int64_t)frame * a.dense_frame_stride);
  for (int64_t k = tid; k < chunks; k += threads) {
    const int64_t i0 = k * E;
    const int n = total - i0 < E ? (int)(total - i0) : E;
    int64_t r = i0 / a.cols;
    int c = (int)(i0 - r * a.cols);
    uint32_t v[E];
    if (a.strided_vec && n == E) {
      constexpr int Q = E * (int)sizeof(Raw) / 16;
      V16 raw[Q];
      const V16* p = reinterpret_cast<const V16*>(src + r * a.row_stride + (int64_t)c * (int64_t)sizeof(Raw));
      for (int q = 0; q < Q; ++q) raw[q] = p[q];
      Raw e[E];
      __builtin_memcpy(e, raw, sizeof e);
      for (int j = 0; j < E; ++j) v[j] = Elem<T>::to_bits(e[j]);
    } else {
      for (int j = 0; j < n; ++j) {
        v[j] = Elem<T>::to_bits(load_elem<Raw>(src + r * a.row_stride + (int64_t)c * a.col_stride, a.elem_aligned));
        if (++c == a.cols) c = 0, ++r;
      }
    }
    if (a.dense_vec && n == E) {
      V16* q = reinterpret_cast<V16*>(dst + i0);
      for (int j = 0; j < E / 4; ++j) q[j] = V16{{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]}};
    } else {
      for (int j = 0; j < n; ++j) dst[i0 + j] = v[j];
    }
  }
}

// C2: the mirror image; T is float, double or Half
template <class T>
RPSFV_HD void c2_thread(const Args& a, int64_t tid, int64_t threads, int frame) {
  using Raw = typename Elem<T>::Raw;
  constexpr int E = sizeof(Raw) >= 4 ? 4 : 16 / (int)sizeof(Raw);
  const int64_t total = (int64_t)a.rows * a.cols, chunks = (total + E - 1) / E;
  char* dst = a.strided + (int64_t)frame * a.frame_stride;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.dense + (int64_t)frame * a.dense_frame_stride);
  for (int64_t k = tid; k < chunks; k += threads) {
    const int64_t i0 = k * E;
    const int n = total - i0 < E ? (int)(total - i0) : E;
    int64_t r = i0 / a.cols;
    int c = (int)(i0 - r * a.cols);
    uint32_t v[E];
    if (a.dense_vec && n == E) {
      const V16* q = reinterpret_cast<const V16*>(src + i0);
      for (int j = 0; j < E / 4; ++j) {
        const V16 x = q[j];
        v[4 * j] = x.w[0], v[4 * j + 1] = x.w[1], v[4 * j + 2] = x.w[2], v[4 * j + 3] = x.w[3];
      }
    } else {
      for (int j = 0; j < n; ++j) v[j] = src[i0 + j];
    }
    if (a.strided_vec && n == E) {
      constexpr int Q = E * (int)sizeof(Raw) / 16;
      Raw e[E];
      for (int j = 0; j < E; ++j) e[j] = Elem<T>::from_bits(v[j]);
      V16 raw[Q];
      __builtin_memcpy(raw, e, sizeof e);
      V16* p = reinterpret_cast<V16*>(dst + r * a.row_stride + (int64_t)c * (int64_t)sizeof(Raw));
      for (int q = 0; q < Q; ++q) p[q] = raw[q];
    } else {
      for (int j = 0; j < n; ++j) {
        store_elem<Raw>(dst + r * a.row_stride + (int64_t)c * a.col_stride, Elem<T>::from_bits(v[j]), a.elem_aligned);
        if (++c == a.cols) c = 0, ++r;
      }
    }
  }
}

// the body for a dtype code: f.template operator()<T>()
template <class F>
RPSFV_HD bool dispatch_dtype(int dtype, F&& f) {
  switch (dtype) {
    case RPSF_DTYPE_FLOAT32: f.template operator()<float>(); return true;
    case RPSF_DTYPE_FLOAT64: f.template operator()<double>(); return true;
    case RPSF_DTYPE_FLOAT16: f.template operator()<Half>(); return true;
    case RPSF_DTYPE_UINT8: f.template operator()<uint8_t>(); return true;
    case RPSF_DTYPE_INT16: f.template operator()<int16_t>(); return true;
    case RPSF_DTYPE_UINT16: f.template operator()<uint16_t>(); return true;
    case RPSF_DTYPE_INT32: f.template operator()<int32_t>(); return true;
    default: return false;
  }
}
}  // namespace rpsfconv
