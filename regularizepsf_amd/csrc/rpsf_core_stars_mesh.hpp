// rpsf_core_stars_mesh.hpp - kernel S1b of the star finder (csrc/stars.hip): the fill and the 3 x 3 median filter of the background mesh
// on the device, shared with the CPU lane emulator tests/emu/emu_stars_mesh.cpp.  What it computes is regularizepsf_amd.stars.filter_mesh,
// bit for bit:
//
//   valid = isfinite(level) & isfinite(rms); no valid node: the flag "no usable box".  The invalid nodes of level take the median of
//   level[valid], those of rms the median of rms[valid] (NumPy's rule: the middle element, or (a + b) / 2.0 of the two middle ones);
//   a 3 x 3 median (rank 4 of 9) with the indices clamped at the edges runs over both filled meshes into a second pair of arrays;
//   global_rms is the median of the filtered rms; T = threshold * global_rms.
//
// All of it is selection on the value bits - the only arithmetic is (a + b) / 2.0 and the one multiply.  A whole-mesh median is the exact
// k-th element by a search on the order-preserving 64-bit keys of the doubles (B2's idea, rpsf_core_builder.hpp, four bits at a time): a MIN
// and a MAX pass bound the keys; then, nibble by nibble below the nibbles all keys share, a counting pass builds the 16-bin histogram of the
// next nibble over the keys that carry the prefix found so far, and the bin that holds the k-th key extends the prefix; one NEXT pass finds
// the upper middle element of an even count.  Two medians run side by side (level and rms share the valid nodes), so a pass counts for two
// channels.  No storage grows with the mesh and nothing depends on how the nodes are dealt to threads: counts are integers, minima and
// maxima are order-free.
//
//   one workgroup (s1b_mesh): the S1B_THREADS threads stride over the mesh (the drivers of rpsf_core_stars.hpp: ctx.each(f) is f(tid) for
//       every thread, then a barrier); the keys of MIN, MAX and NEXT fold through LDS as 16 x 16, the histograms are LDS counters that the
//       threads add to with integer atomics; every thread keeps the same selection state.
//   many workgroups (many_*): above MANY_NODES nodes.  The selection state lives in device memory; per pass one launch of many_count
//       (workgroups fold or count in LDS, then integer atomic add / min / max into one accumulator) and a one-thread launch of many_step,
//       which moves the state on and resets the accumulator; fill and filter are grid kernels, one thread per node.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RPSFM_HD __host__ __device__ __forceinline__
#else
#define RPSFM_HD inline
#endif

// T = threshold * global_rms and (a + b) / 2.0 are compared with NumPy's bit for bit: nothing may be contracted
#pragma clang fp contract(off)

namespace rpsfm {

constexpr int S1B_THREADS = 256;
// The switch between the two routes.  One workgroup reads nodes / 256 values per thread and pass from L2; at 16 384 nodes that is 64
// dependent-free loads, a few microseconds - what the two launches of a many-workgroup pass cost before they count anything.  Below, the
// launches would dominate; above, the one compute unit would.
constexpr long MANY_NODES = 16384;
constexpr int MANY_WORKGROUPS = 256;  // at most, of S1B_THREADS threads, per counting launch

// the passes of one selection, in order: step 0 MIN, 1 MAX, 2 .. 17 DIGIT for nibble 15 .. 0 of the key, 18 NEXT
constexpr int RADIX_BITS = 4, DIGITS = 1 << RADIX_BITS, NIBBLES = 64 / RADIX_BITS;
constexpr int STEP_MIN = 0, STEP_MAX = 1, STEP_DIGIT0 = 2, STEP_NEXT = STEP_DIGIT0 + NIBBLES, STEPS = STEP_NEXT + 1;

// ------------------------------------------------------------------------------------------------ integer atomics
#if defined(__HIP_DEVICE_COMPILE__)
RPSFM_HD void add_u32(unsigned* p, unsigned v) { atomicAdd(p, v); }
RPSFM_HD void min_u64(uint64_t* p, uint64_t v) { atomicMin(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
RPSFM_HD void max_u64(uint64_t* p, uint64_t v) { atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
#else
RPSFM_HD void add_u32(unsigned* p, unsigned v) { *p += v; }
RPSFM_HD void min_u64(uint64_t* p, uint64_t v) { if (v < *p) *p = v; }
RPSFM_HD void max_u64(uint64_t* p, uint64_t v) { if (v > *p) *p = v; }
#endif

// ------------------------------------------------------------------------------------------------ keys
// order-preserving map of the doubles (infinities included, NaN excluded) onto unsigned integers
RPSFM_HD uint64_t key_of(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
RPSFM_HD double value_of(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x;
  std::memcpy(&x, &u, 8);
  return x;
}
RPSFM_HD bool finite_d(double x) { return std::fabs(x) <= 1.79769313486231570815e308; }

// ------------------------------------------------------------------------------------------------ selection
// What two medians run over: channel 0 reads a[i], channel 1 reads b[i]; with `valid_only` only the nodes where both are finite count.
struct Source {
  const double* a;
  const double* b;
  long n;
  int valid_only;
  RPSFM_HD bool use(long i) const { return !valid_only || (finite_d(a[i]) && finite_d(b[i])); }
};

struct Fold {  // what a thread or a group of 16 contributes to a MIN, MAX or NEXT pass
  uint64_t k[2];
  unsigned c[2];
};
struct Total {  // what the whole mesh contributes to a pass: keys and c[ch][0] of MIN / MAX / NEXT, the histograms of a DIGIT pass
  uint64_t k[2];
  unsigned c[2][DIGITS];
};
struct Sel {  // the state of two selections; n: the nodes that count
  uint64_t lo[2], hi[2], ans[2], next[2];  // ans: the nibbles of the k-th key found so far, zeros below
  unsigned n, below[2], le[2];             // below: the keys smaller than every key that carries the prefix ans
  int top[2];                              // the highest bit in which two keys of the channel differ, -1: all keys are one
};

RPSFM_HD bool digit_step(int step) { return step >= STEP_DIGIT0 && step < STEP_NEXT; }
RPSFM_HD int step_nibble(int step) { return NIBBLES - 1 - (step - STEP_DIGIT0); }
RPSFM_HD uint64_t above(uint64_t key, int nibble) { return nibble == NIBBLES - 1 ? 0ull : key >> (RADIX_BITS * (nibble + 1)); }
RPSFM_HD int digit_of(uint64_t key, int nibble) { return (int)((key >> (RADIX_BITS * nibble)) & (uint64_t)(DIGITS - 1)); }
RPSFM_HD bool channel_counts(const Sel& s, int ch, int nibble) { return RADIX_BITS * nibble <= s.top[ch]; }  // the nibble is not shared by all keys

RPSFM_HD Fold identity(int step) {
  const uint64_t k = (step == STEP_MIN || step == STEP_NEXT) ? ~0ull : 0ull;
  return Fold{{k, k}, {0u, 0u}};
}
RPSFM_HD void merge(int step, Fold& into, const Fold& x) {
  for (int ch = 0; ch < 2; ++ch) {
    into.c[ch] += x.c[ch];
    if (step == STEP_MAX) {
      if (x.k[ch] > into.k[ch]) into.k[ch] = x.k[ch];
    } else if (x.k[ch] < into.k[ch]) {
      into.k[ch] = x.k[ch];
    }
  }
}
RPSFM_HD Fold fold16(int step, const Fold* p) {
  Fold r = identity(step);
  for (int j = 0; j < 16; ++j) merge(step, r, p[j]);
  return r;
}
RPSFM_HD Total total_of(const Fold& f) {
  Total t{};
  for (int ch = 0; ch < 2; ++ch) t.k[ch] = f.k[ch], t.c[ch][0] = f.c[ch];
  return t;
}

// has the step anything to decide?  (thread-uniform: a function of the state alone)
RPSFM_HD bool step_active(const Sel& s, int step) {
  if (step == STEP_MIN) return true;
  if (s.n == 0) return false;
  if (step == STEP_MAX) return true;
  if (step == STEP_NEXT) return s.n % 2 == 0;
  return channel_counts(s, 0, step_nibble(step)) || channel_counts(s, 1, step_nibble(step));
}

// MIN, MAX, NEXT: nodes first, first + stride, ... of the source
RPSFM_HD Fold partial(long first, long stride, const Source& src, const Sel& s, int step) {
  Fold r = identity(step);
  for (long i = first; i < src.n; i += stride) {
    if (!src.use(i)) continue;
    const uint64_t key[2] = {key_of(src.a[i]), key_of(src.b[i])};
    for (int ch = 0; ch < 2; ++ch) {
      if (step == STEP_MIN) {
        r.c[ch] += 1;
        if (key[ch] < r.k[ch]) r.k[ch] = key[ch];
      } else if (step == STEP_MAX) {
        if (key[ch] > r.k[ch]) r.k[ch] = key[ch];
      } else if (key[ch] <= s.ans[ch]) {
        r.c[ch] += 1;
      } else if (key[ch] < r.k[ch]) {
        r.k[ch] = key[ch];
      }
    }
  }
  return r;
}

// DIGIT: nodes first, first + stride, ... into hist[ch * DIGITS + digit] (counters many threads add to): per channel the keys that carry the
// prefix found so far, by their next nibble
RPSFM_HD void count(long first, long stride, const Source& src, const Sel& s, int nibble, unsigned* hist) {
  for (long i = first; i < src.n; i += stride) {
    if (!src.use(i)) continue;
    const uint64_t key[2] = {key_of(src.a[i]), key_of(src.b[i])};
    for (int ch = 0; ch < 2; ++ch)
      if (channel_counts(s, ch, nibble) && above(key[ch], nibble) == above(s.ans[ch], nibble)) add_u32(hist + ch * DIGITS + digit_of(key[ch], nibble), 1u);
  }
}

// the state after `step`, from what the whole mesh contributed to it
RPSFM_HD void advance(Sel& s, int step, const Total& total) {
  const unsigned kth = s.n ? (s.n - 1) / 2 : 0;
  for (int ch = 0; ch < 2; ++ch) {
    if (step == STEP_MIN) {
      s.lo[ch] = total.k[ch], s.n = total.c[0][0];
      s.hi[ch] = s.ans[ch] = s.next[ch] = 0, s.below[ch] = s.le[ch] = 0, s.top[ch] = -1;
    } else if (step == STEP_MAX) {
      s.hi[ch] = total.k[ch];
      int top = 63;
      while (top >= 0 && !(((s.lo[ch] ^ s.hi[ch]) >> top) & 1ull)) --top;
      s.top[ch] = top;
      const int shared = top < 0 ? 0 : RADIX_BITS * (top / RADIX_BITS + 1);  // the bits of the nibbles all keys share lie above
      s.ans[ch] = shared >= 64 ? 0ull : (s.lo[ch] >> shared) << shared;
      s.below[ch] = 0;  // every key carries that prefix
    } else if (step == STEP_NEXT) {
      s.le[ch] = total.c[ch][0], s.next[ch] = total.k[ch];
    } else if (channel_counts(s, ch, step_nibble(step))) {
      // below <= kth < below + (keys with the prefix): the k-th key is in the first bin the running count passes kth in
      unsigned run = s.below[ch];
      int d = 0;
      bool before = true;  // (a fixed trip count: the bins stay in registers)
      for (int e = 0; e < DIGITS - 1; ++e) {
        before = before && run + total.c[ch][e] <= kth;
        if (before) run += total.c[ch][e], ++d;
      }
      s.ans[ch] |= (uint64_t)d << (RADIX_BITS * step_nibble(step));
      s.below[ch] = run;
    }
  }
}

// NumPy's median of the channel, once every step has run
RPSFM_HD double median_of(const Sel& s, int ch) {
  const double a = value_of(s.ans[ch]);
  if (s.n % 2 == 1) return a;
  const double b = s.le[ch] >= (s.n - 1) / 2 + 2 ? a : value_of(s.next[ch]);
  return (a + b) / 2.0;
}

// ------------------------------------------------------------------------------------------------ per node
// node i of both meshes, in place: an invalid node takes the medians of the valid ones
RPSFM_HD void fill_node(long i, double* level, double* rms, double median_level, double median_rms) {
  if (finite_d(level[i]) && finite_d(rms[i])) return;
  level[i] = median_level, rms[i] = median_rms;
}

// rank 4 of the 3 x 3 neighbourhood of node (r, c), indices clamped (scipy.ndimage.median_filter(mesh, 3, mode="nearest"))
RPSFM_HD double median9(const double* mesh, int nby, int nbx, int r, int c) {
  double v[9];
  uint64_t k[9];
  for (int dr = -1; dr <= 1; ++dr)
    for (int dc = -1; dc <= 1; ++dc) {
      const int rr = r + dr < 0 ? 0 : (r + dr > nby - 1 ? nby - 1 : r + dr), cc = c + dc < 0 ? 0 : (c + dc > nbx - 1 ? nbx - 1 : c + dc);
      const int j = 3 * (dr + 1) + dc + 1;
      v[j] = mesh[(long)rr * nbx + cc], k[j] = key_of(v[j]);
    }
  double out = v[4];
  for (int j = 0; j < 9; ++j) {
    int below = 0, not_above = 0;
    for (int m = 0; m < 9; ++m) below += k[m] < k[j], not_above += k[m] <= k[j];
    if (below <= 4 && 4 < not_above) out = v[j];  // every j that passes holds the same key
  }
  return out;
}
RPSFM_HD void filter_node(long i, int nby, int nbx, const double* level, const double* rms, double* level_f, double* rms_f) {
  const int r = (int)(i / nbx), c = (int)(i % nbx);
  level_f[i] = median9(level, nby, nbx, r, c), rms_f[i] = median9(rms, nby, nbx, r, c);
}

// out[0] = global_rms, out[1] = T.  No usable box: T = +inf, under which S2 detects nothing whatever the meshes hold.
constexpr int OUT_GLOBAL_RMS = 0, OUT_T = 1;
RPSFM_HD double threshold_of(double threshold, double global_rms, int none) { return none ? HUGE_VAL : threshold * global_rms; }

// ------------------------------------------------------------------------------------------------ one workgroup
constexpr int HIST = 2 * DIGITS;  // counters of a DIGIT pass
RPSFM_HD size_t s1b_lds_bytes() { return (size_t)(S1B_THREADS + 16) * sizeof(Fold) + 3 * HIST * sizeof(unsigned); }  // 6.8 KiB

// MIN, MAX and NEXT fold through LDS as 16 x 16.  A DIGIT pass adds to a histogram in LDS and ends with one barrier.  Three histograms
// rotate: pass q adds to histogram q % 3 while the first threads clear histogram (q + 1) % 3, which was last read before the barrier of
// pass q - 1.
template <class Ctx>
RPSFM_HD Sel select(Ctx& ctx, const Source& src, Fold* part) {
  Fold* part2 = part + S1B_THREADS;
  unsigned* hists = reinterpret_cast<unsigned*>(part2 + 16);
  Sel s{};
  ctx.each([&](int tid) {
    if (tid < HIST) hists[tid] = 0u;
  });
  int q = 0;
  for (int step = 0; step < STEPS; ++step) {
    if (!step_active(s, step)) continue;
    if (digit_step(step)) {
      unsigned* mine = hists + HIST * (q % 3);
      unsigned* next = hists + HIST * ((q + 1) % 3);
      ctx.each([&](int tid) {
        if (tid < HIST) next[tid] = 0u;
        count(tid, S1B_THREADS, src, s, step_nibble(step), mine);
      });
      Total t{};
      for (int j = 0; j < HIST; ++j) t.c[j / DIGITS][j % DIGITS] = mine[j];
      advance(s, step, t);
      ++q;
      continue;
    }
    ctx.each([&](int tid) { part[tid] = partial(tid, S1B_THREADS, src, s, step); });
    ctx.each([&](int tid) {
      if (tid < 16) part2[tid] = fold16(step, part + 16 * tid);
    });
    advance(s, step, total_of(fold16(step, part2)));  // read by everybody before the next fold's second barrier lets part2 change
  }
  return s;
}

// The whole of S1b on an nby x nbx mesh.  level / rms: S1's raw meshes, filled in place; level_f / rms_f: the filtered ones;
// out[OUT_GLOBAL_RMS]; *none = 1 when no node is valid (then nothing else is written).  `lds` holds s1b_lds_bytes().
template <class Ctx>
RPSFM_HD void s1b_mesh(Ctx& ctx, int nby, int nbx, double* level, double* rms, double* level_f, double* rms_f, double* out, int* none,
                       void* lds) {
  Fold* part = static_cast<Fold*>(lds);
  const long n = (long)nby * nbx;
  const Sel valid = select(ctx, Source{level, rms, n, 1}, part);
  if (valid.n == 0) {
    ctx.each([&](int tid) {
      if (tid == 0) *none = 1;
    });
    return;
  }
  const double median_level = median_of(valid, 0), median_rms = median_of(valid, 1);
  ctx.each([&](int tid) {
    for (long i = tid; i < n; i += S1B_THREADS) fill_node(i, level, rms, median_level, median_rms);
  });
  ctx.each([&](int tid) {
    for (long i = tid; i < n; i += S1B_THREADS) filter_node(i, nby, nbx, level, rms, level_f, rms_f);
  });
  const Sel all = select(ctx, Source{rms_f, rms_f, n, 0}, part);
  const double global_rms = median_of(all, 0);
  ctx.each([&](int tid) {
    if (tid == 0) *none = 0, out[OUT_GLOBAL_RMS] = global_rms;
  });
}

// ------------------------------------------------------------------------------------------------ many workgroups
RPSFM_HD int many_workgroups(long n) {
  const long w = (n + S1B_THREADS - 1) / S1B_THREADS;
  return (int)(w < 1 ? 1 : w > MANY_WORKGROUPS ? MANY_WORKGROUPS : w);
}

// workgroup `wg` of `nwg`: its share of the step into *acc.  `lds` holds s1b_lds_bytes().
template <class Ctx>
RPSFM_HD void many_count(Ctx& ctx, int wg, int nwg, const Source& src, const Sel* state, int step, Total* acc, void* lds) {
  const Sel s = *state;
  if (!step_active(s, step)) return;
  const long first = (long)wg * S1B_THREADS, stride = (long)nwg * S1B_THREADS;
  if (digit_step(step)) {
    unsigned* hist = static_cast<unsigned*>(lds);
    ctx.each([&](int tid) {
      if (tid < HIST) hist[tid] = 0u;
    });
    ctx.each([&](int tid) { count(first + tid, stride, src, s, step_nibble(step), hist); });
    ctx.each([&](int tid) {
      if (tid < HIST && hist[tid]) add_u32(&acc->c[tid / DIGITS][tid % DIGITS], hist[tid]);
    });
    return;
  }
  Fold* part = static_cast<Fold*>(lds);
  Fold* part2 = part + S1B_THREADS;
  ctx.each([&](int tid) { part[tid] = partial(first + tid, stride, src, s, step); });
  ctx.each([&](int tid) {
    if (tid < 16) part2[tid] = fold16(step, part + 16 * tid);
  });
  ctx.each([&](int tid) {
    if (tid != 0) return;
    const Fold mine = fold16(step, part2);
    for (int ch = 0; ch < 2; ++ch) {
      if (mine.c[ch]) add_u32(&acc->c[ch][0], mine.c[ch]);
      if (step == STEP_MAX) max_u64(&acc->k[ch], mine.k[ch]);
      else min_u64(&acc->k[ch], mine.k[ch]);
    }
  });
}
// one thread, after the counting launch of `step` (step -1: before the first): the state moves on, the accumulator is made ready for the
// next step
RPSFM_HD void many_step(Sel* state, Total* acc, int step) {
  if (step >= 0) {
    Sel s = *state;
    if (step_active(s, step)) advance(s, step, *acc);
    *state = s;
  }
  *acc = total_of(identity(step + 1));
}
RPSFM_HD void many_fill(long i, long n, double* level, double* rms, const Sel* valid) {
  if (i >= n || valid->n == 0) return;
  fill_node(i, level, rms, median_of(*valid, 0), median_of(*valid, 1));
}
RPSFM_HD void many_filter(long i, int nby, int nbx, const double* level, const double* rms, double* level_f, double* rms_f) {
  if (i >= (long)nby * nbx) return;
  filter_node(i, nby, nbx, level, rms, level_f, rms_f);
}
RPSFM_HD void many_finish(const Sel* valid, const Sel* all, double* out, int* none) {
  if (valid->n == 0) {
    *none = 1;
    return;
  }
  *none = 0, out[OUT_GLOBAL_RMS] = median_of(*all, 0);
}

}  // namespace rpsfm
