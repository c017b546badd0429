// CPU lane emulator for rpsf_core_stars_disc.hpp alone (test infrastructure, never shipped in the product path): the box and the walk of
// a disc, the record template and the fold steps, without any of the drivers that use them (tests/test_disc_host.py).
// With -DEMU_DISC_MAIN the file is a stand-alone program (for a sanitizer build of the walk and of the records' carve): walks on, off and
// across the rim of a small frame, a fold of every kind; it prints what it counted and returns 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../regularizepsf_amd/csrc/rpsf_core_stars_disc.hpp"
#include "emu_ctx.hpp"

using namespace rpsfk;

// info[2] = WALK_LANES, WALK_WAVES
extern "C" void emudk_info(long* info) { info[0] = WALK_LANES, info[1] = WALK_WAVES; }

// box[6] = r0, r1, c0, c1, bw, npx of disc_box(y, x, R)
extern "C" void emudk_box(double y, double x, double R, long* box) {
  const DiscBox b = disc_box(y, x, R);
  box[0] = b.r0, box[1] = b.r1, box[2] = b.c0, box[3] = b.c1, box[4] = b.bw, box[5] = b.npx;
}

// walk_disc of every lane in turn over the disc q <= R2 around (y, x) of an H x W frame (mask: 1 = ignore).  One record per call of a
// visitor, in the order of the calls: ints[4 k ..] = lane, kind (0: in the disc, 1: a usable pixel of the frame), r, c - r = c = 0 for
// kind 0, which is not told them -, doubles[4 k ..] = pr, pc, q, p.  Returns the number of records, -1 when more than `cap`.
extern "C" long emudk_walk(const float* img, const uint8_t* mask, int H, int W, double y, double x, double R, double R2, long cap, int* ints,
                           double* doubles) {
  const Frame fr{img, mask, H, W, 0, 0, 0};
  long k = 0;
  auto put = [&](int lane, int kind, int r, int c, double pr, double pc, double q, double p) {
    if (k < cap) ints[4 * k] = lane, ints[4 * k + 1] = kind, ints[4 * k + 2] = r, ints[4 * k + 3] = c;
    if (k < cap) doubles[4 * k] = pr, doubles[4 * k + 1] = pc, doubles[4 * k + 2] = q, doubles[4 * k + 3] = p;
    ++k;
  };
  for (int lane = 0; lane < WALK_LANES; ++lane)
    walk_disc(
        fr, disc_box(y, x, R), y, x, R2, lane, [&](double pr, double pc) { put(lane, 0, 0, 0, pr, pc, 0.0, -1.0); },
        [&](int r, int c, size_t p, double pr, double pc, double q) { put(lane, 1, r, c, pr, pc, q, (double)p); });
  return k <= cap ? k : -1;
}

// bytes() of the five records the drivers use: -1 for any other
extern "C" long emudk_record_bytes(int doubles, int has_at, int counts) {
  if (doubles == 6 && has_at && counts == 2) return (long)LaneRecords<6, true, 2>::bytes();     // S8
  if (doubles == 8 && has_at && counts == 2) return (long)LaneRecords<8, true, 2>::bytes();     // S12
  if (doubles == 7 && !has_at && counts == 2) return (long)LaneRecords<7, false, 2>::bytes();   // S7
  if (doubles == 13 && !has_at && counts == 1) return (long)LaneRecords<13, false, 1>::bytes(); // S9
  if (doubles == 18 && has_at && counts == 2) return (long)LaneRecords<18, true, 2>::bytes();   // S11
  return -1;
}

// The fold of a workgroup's WALK_THREADS lane records of FOLD_DOUBLES doubles (the last of them the signed e of a peak), the peak's
// index and two counts, as the drivers call it: 64 -> 8 by the first 8 lanes of every wave, 8 -> 1 by its first lane.  The inputs are
// field-major (d[f WALK_THREADS + i]); sums[wave FOLD_SUMS + f], counts[wave 2 + f], peak_e[wave], peak_at[wave].  The records lie in
// a buffer of exactly walk_records_bytes() that starts with garbage.  offsets[4]: where, in bytes from the buffer's start, the lane
// records' `at` and `cnt` and the group records' `d` and `cnt` lie.
constexpr int FOLD_SUMS = 2, FOLD_DOUBLES = FOLD_SUMS + 1;
using FoldRecords = LaneRecords<FOLD_DOUBLES, true, 2>;
extern "C" void emudk_fold(const double* d, const long long* at, const int* cnt, double* sums, int* counts, double* peak_e, long long* peak_at,
                           long* offsets) {
  std::vector<char> lds(walk_records_bytes<FoldRecords>());
  std::memset(lds.data(), 0x5A, lds.size());
  const FoldRecords acc(lds.data(), WALK_THREADS);
  const FoldRecords acc2(lds.data() + WALK_THREADS * FoldRecords::bytes(), WALK_GROUPS);
  offsets[0] = (char*)acc.at - lds.data(), offsets[1] = (char*)acc.cnt - lds.data();
  offsets[2] = (char*)acc2.d - lds.data(), offsets[3] = (char*)acc2.cnt - lds.data();
  CpuCtx ctx{WALK_THREADS};
  ctx.each([&](int tid) {
    for (int f = 0; f < FOLD_DOUBLES; ++f) acc.d[f * WALK_THREADS + tid] = d[f * WALK_THREADS + tid];
    acc.at[tid] = at[tid];
    for (int f = 0; f < 2; ++f) acc.cnt[f * WALK_THREADS + tid] = cnt[f * WALK_THREADS + tid];
  });
  ctx.each([&](int tid) {
    if (tid % WALK_LANES >= 8) return;
    fold_sums_64to8(acc, acc2, tid, FOLD_SUMS), fold_counts_64to8(acc, acc2, tid, 2), fold_peak_64to8(acc, acc2, tid, FOLD_SUMS);
  });
  ctx.each([&](int tid) {
    const int wave = tid / WALK_LANES;
    if (tid % WALK_LANES != 0) return;
    fold_sums_8to1(acc2, wave, FOLD_SUMS, sums + wave * FOLD_SUMS), fold_counts_8to1(acc2, wave, 2, counts + wave * 2);
    const Peak seen = fold_peak_8to1(acc2, wave, FOLD_SUMS);
    peak_e[wave] = seen.e, peak_at[wave] = seen.at;
  });
}

#if defined(EMU_DISC_MAIN)
int main() {
  const int H = 12, W = 10;
  std::vector<float> img((size_t)H * W, 1.0f);
  std::vector<uint8_t> mask((size_t)H * W, 0);
  img[4 * W + 4] = NAN, mask[5 * W + 5] = 1;
  const long cap = 4096;
  std::vector<int> ints(4 * cap);
  std::vector<double> doubles(4 * cap);
  long calls = 0;
  const double pos[] = {5.0, 4.0, 5.5, 4.5, -0.25, 0.0, 11.0, 9.0, -100.0, -100.0};
  for (int i = 0; i < 5; ++i)
    for (double R : {1.0, 2.0, 6.0}) {
      const long k = emudk_walk(img.data(), mask.data(), H, W, pos[2 * i], pos[2 * i + 1], R, R * R, cap, ints.data(), doubles.data());
      if (k < 0) return 1;
      calls += k;
    }
  std::vector<double> d((size_t)FOLD_DOUBLES * WALK_THREADS);
  std::vector<long long> at(WALK_THREADS);
  std::vector<int> cnt(2 * WALK_THREADS);
  for (int i = 0; i < WALK_THREADS; ++i) {
    d[i] = i % 3 == 0 ? 1e16 : i % 3 == 1 ? 1.0 : -1e16, d[WALK_THREADS + i] = 0.1 * i, d[2 * WALK_THREADS + i] = i % 7 == 0 ? NAN : (double)(i % 5) - 2.0;
    at[i] = i % 11 == 0 ? -1 : 1000 - i, cnt[i] = i, cnt[WALK_THREADS + i] = 1;
  }
  double sums[WALK_WAVES * FOLD_SUMS], peak_e[WALK_WAVES];
  int counts[WALK_WAVES * 2];
  long long peak_at[WALK_WAVES];
  long offsets[4];
  emudk_fold(d.data(), at.data(), cnt.data(), sums, counts, peak_e, peak_at, offsets);
  std::printf("emu_disc: %ld visitor calls, %d + %d pixels counted by the fold, %ld bytes of records\n", calls, counts[1], counts[3],
              (long)walk_records_bytes<FoldRecords>());
  return counts[1] == WALK_LANES && emudk_record_bytes(6, 1, 2) == 64 ? 0 : 2;
}
#endif
