// rpsf_lattice.hpp - what the host decides from a corner list alone: whether the corners form a regular half-overlap lattice, the
// colour classes, the processing order, the tile tables the fused and persistent launches of the patch kernels wait on, the quadrant
// words of the direct mode, the row bands of a large host frame, and the geometry predicates that choose between launch forms.
// Plain C++: rpsf.hip uploads what lattice_build() returns, tests/emu/*.cpp and tests/test_lattice_host.py call the same functions.
//
// Lattice (h = N / 2): patch corners at (r0 + li h, c0 + lj h), nli x nlj cells, at most one patch per cell.  The output is cut into
// nti x ntj = (nli + 1) x (nlj + 1) TILES of h x h pixels; the patch of cell (li, lj) writes the tiles (li + (q >> 1), lj + (q & 1)),
// q = 0 .. 3, and its COLOUR is 2 (li & 1) + (lj & 1): patches of one colour do not overlap, so each colour has a plane of its own.
// A summing workgroup waits until a tile's counter reaches epoch x popcount(cover[tile]) - a wrong table is a wait that never ends.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/rpsf.h"
#include "rpsf_core.hpp"
#include "rpsf_launch.hpp"  // patch_teams(), chunk_patches(): the processing order and the tile order are cut by the chunk the launches index by

namespace rpsf {

// Patch sizes the sweep kernel (third generation) is compiled for
constexpr bool sweep_patch_size(int N) { return N == 64 || N == 32 || N == 16; }

inline uint64_t morton2(uint32_t a, uint32_t b) {
  auto spread = [](uint64_t x) {
    x &= 0xffffffffull;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
  };
  return (spread(a) << 1) | spread(b);
}

// Development knobs of the processing order (rpsf.hip fills them from the environment in development builds only)
struct LatticeKnobs {
  int strips = 0;         // column strips; 0: about 8 patches wide (4096^2: 4 as before; 8192^2: 8, -1.2 % against 4)
  bool meet = true;       // (4096^2 / 256: 0.1877 vs 0.1900 ms with alternating strip directions; false selects those)
  bool rim_first = true;  // false: the rim patches stay where the walk put them
  int rim_last = -1;      // rim patches at the end (1) or at the start (0) of their chunk; -1: the end for N = 256
};
// A view's parent: its lattice origin and whether it has a lattice
struct LatticeParent {
  int r0, c0;
  bool lattice;
};
struct PatchDesc {  // per processing-order slot (the kernels read it as int4)
  int32_t row, col, k_index, colour;
};
static_assert(sizeof(PatchDesc) == 16, "PatchDesc layout");
struct QuadWords {  // per processing-order slot: quadrant words (rpsf_core.hpp, store_patch_direct; the kernels read them as uint4)
  uint32_t q[4];
};
static_assert(sizeof(QuadWords) == 16, "QuadWords layout");

struct LatticeTables {
  bool lattice = false;    // regular half-overlap lattice, at most one patch per cell
  bool direct_ok = false;  // lattice and one patch per workgroup
  int r0 = 0, c0 = 0, nti = 0, ntj = 0;  // origin and tiles (lattice only)
  int par_j = 0;                         // parity of a view's first patch column in its parent's lattice
  std::vector<int32_t> order;            // processing order: slot -> patch
  std::vector<PatchDesc> desc;
  // ---- lattice only ----
  std::vector<int32_t> cell;             // lattice cell -> patch (or -1)
  std::vector<uint8_t> cover;            // per tile: colours of its contributors
  std::vector<int32_t> sweep_slot;       // complete lattice of at least 2 x 2 patches of a sweep_patch_size(): cell -> transfer-kernel slot
  // ---- second generation (fused plane sum) ----
  std::vector<uint32_t> sum_order;       // all tiles, the ones whose contributors run first first
  std::vector<uint32_t> prefetch_tiles;  // per chunk: lattice tiles in the order the chunk's patches first need them
  uint32_t prefetch_first[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  // ---- direct_ok ----
  std::vector<QuadWords> quads;
  std::vector<uint8_t> tile_info;        // per tile: static side mask | 16 if any patch covers it
};

// Regular lattice test + colour classes + tile tables + processing order.  k_index: null for a plan of its own, else patch i of a view is
// patch k_index[i] of its parent; v2: the tables of the second-generation kernels are wanted; parent: null unless a view.
inline LatticeTables lattice_build(int N, int n, const int32_t* coords, const int32_t* k_index, bool v2, const LatticeParent* parent,
                                   const LatticeKnobs& knobs = LatticeKnobs()) {
  LatticeTables t;
  const int half = N / 2;
  int r0 = coords[0], c0 = coords[1], r1 = r0, c1 = c0;
  for (int i = 0; i < n; ++i) {
    r0 = std::min(r0, coords[2 * i]), r1 = std::max(r1, coords[2 * i]);
    c0 = std::min(c0, coords[2 * i + 1]), c1 = std::max(c1, coords[2 * i + 1]);
  }
  bool ok = true;
  for (int i = 0; i < n && ok; ++i) ok = (coords[2 * i] - r0) % half == 0 && (coords[2 * i + 1] - c0) % half == 0;
  int nti = 0, ntj = 0;
  if (ok) {
    nti = (r1 - r0) / half + 2, ntj = (c1 - c0) / half + 2;
    if ((size_t)nti * ntj >= ((size_t)1 << 24)) ok = false;
  }
  std::vector<uint8_t> cls(n, 0);
  std::vector<int32_t>& cell = t.cell;
  const int nli = nti - 1, nlj = ntj - 1;
  const int par_i = ok && parent && parent->lattice ? ((r0 - parent->r0) / half) & 1 : 0;
  const int par_j = ok && parent && parent->lattice ? ((c0 - parent->c0) / half) & 1 : 0;
  if (ok) {
    cell.assign((size_t)nli * nlj, -1);
    for (int i = 0; i < n && ok; ++i) {
      const int li = (coords[2 * i] - r0) / half, lj = (coords[2 * i + 1] - c0) / half;
      if (cell[(size_t)li * nlj + lj] >= 0) ok = false;  // duplicate corner: two patches in one plane cell
      cell[(size_t)li * nlj + lj] = i;
      // (a view takes its colours from the parent's lattice: the planes are summed in colour order, so a band's pixels then come out
      // bit-identical to the whole-frame apply's)
      cls[i] = (uint8_t)((((li + par_i) & 1) << 1) | ((lj + par_j) & 1));
    }
  }
  t.lattice = ok;
  const int chunk = chunk_patches(n, patch_teams(N));
  t.direct_ok = ok && patch_teams(N) == 1;
  // ---- processing order: 8 chunks, one per XCD (workgroups b and b + 8 share one) ----
  t.order.resize(n);
  if (ok) {
    // Column strips walked boustrophedon, cut into 8 equal runs: compact regions, so that the four patches over a
    // tile mostly run on one XCD (they read the same pixels through one L2, and the tile can be accumulated there).
    const int strips = knobs.strips > 0 ? std::min(nlj, knobs.strips) : nlj >= 8 ? std::max(4, nlj / 8) : 1;
    int k = 0;
    for (int s2 = 0; s2 < strips; ++s2) {
      const int ja = (int)((long)nlj * s2 / strips), jb = (int)((long)nlj * (s2 + 1) / strips);
      auto row = [&](int li) {
        for (int lj = ja; lj < jb; ++lj)
          if (cell[(size_t)li * nlj + lj] >= 0) t.order[k++] = cell[(size_t)li * nlj + lj];
      };
      if (knobs.meet) {
        // the upper half of every strip top-down, the lower half bottom-up: the two XCDs of a strip meet in the middle at the end, and
        // neighbouring strips walk the same rows at the same time, so the tiles on region borders do not wait a whole launch for
        // their last contributor (their planes would long have left the Infinity Cache)
        const int mid = (nli + 1) / 2;
        for (int li = 0; li < mid; ++li) row(li);
        for (int li = nli - 1; li >= mid; --li) row(li);
        continue;
      }
      for (int step = 0; step < nli; ++step) row((s2 & 1) ? nli - 1 - step : step);
    }
    // Inside a chunk the patches on the rim of the lattice go first.  They hang over the image edge and take the slower
    // padded gather / cropped store path (+50 % per patch at N = 256); dispatched first, they are the long jobs of a
    // longest-job-first list schedule: a CU that drew one simply takes one patch fewer later on, instead of a late rim
    // patch stretching the last round.  (Round 1: N = 256 215 -> 207 us, 2048^2 / N = 128 67 -> 58 us.)
    if (knobs.rim_first) {
      auto rim = [&](int32_t i) {
        const int r = coords[2 * i], c = coords[2 * i + 1];
        return r == r0 || r == r1 || c == c0 || c == c1;
      };
      // ... until the rim patches got their 16-byte paths: they are now the cheaper ones (half or a quarter of the stores).  With one
      // patch per CU (N = 256) they go LAST, so that the patches of the partial last round are the short ones (4096^2: -1 %,
      // profiles/r02av); with four workgroups per CU (N = 128) first is still the better order (2048^2: 0.0685 vs 0.0705 ms).
      const bool rim_last = knobs.rim_last >= 0 ? knobs.rim_last != 0 : N == 256;
      for (int x = 0; x < 8; ++x) {
        const int lo = std::min(n, x * chunk), hi = std::min(n, lo + chunk);
        if (rim_last)
          std::stable_partition(t.order.begin() + lo, t.order.begin() + hi, [&](int32_t i) { return !rim(i); });
        else
          std::stable_partition(t.order.begin() + lo, t.order.begin() + hi, rim);
      }
    }
  } else {
    std::vector<std::pair<uint64_t, int32_t>> keyed(n);
    for (int i = 0; i < n; ++i)
      keyed[i] = {morton2((uint32_t)((coords[2 * i] - r0) / half), (uint32_t)((coords[2 * i + 1] - c0) / half)), i};
    std::sort(keyed.begin(), keyed.end());
    for (int i = 0; i < n; ++i) t.order[i] = keyed[i].second;
  }
  t.desc.resize(n);
  for (int s2 = 0; s2 < n; ++s2) {
    const int i = t.order[s2];
    t.desc[s2] = PatchDesc{coords[2 * i], coords[2 * i + 1], k_index ? k_index[i] : i, ok ? cls[i] : 0};
  }
  if (!ok) {
    cell.clear();
    return t;
  }
  t.r0 = r0, t.c0 = c0, t.nti = nti, t.ntj = ntj, t.par_j = par_j;
  // ---- third generation: the sweep kernel runs when every lattice cell has its patch ----
  if (sweep_patch_size(N) && nli >= 2 && nlj >= 2 && (size_t)nli * nlj == (size_t)n) {
    t.sweep_slot.resize((size_t)nli * nlj);
    for (size_t c = 0; c < t.sweep_slot.size(); ++c) t.sweep_slot[c] = k_index ? k_index[cell[c]] : cell[c];
  }
  // the patches over tile (ti, tj), up to four
  auto contributors = [&](int ti, int tj, int* who) {
    int nwho = 0;
    for (int a2 = 0; a2 < 2; ++a2)
      for (int b2 = 0; b2 < 2; ++b2) {
        const int li = ti - a2, lj = tj - b2;
        if (li < 0 || lj < 0 || li >= nli || lj >= nlj) continue;
        const int i = cell[(size_t)li * nlj + lj];
        if (i >= 0) who[nwho++] = i;
      }
    return nwho;
  };
  // ---- tiles: coverage, owner chunk, ranks ----
  std::vector<int> chunk_of(n), seq_of(n);
  for (int s2 = 0; s2 < n; ++s2) chunk_of[t.order[s2]] = s2 / chunk, seq_of[t.order[s2]] = s2;
  t.cover.assign((size_t)nti * ntj, 0);
  std::vector<uint8_t> tile_info((size_t)nti * ntj, 0);
  std::vector<uint32_t> quad_of((size_t)n * 4, quad_word(QUAD_NONE, 0, 0));
  for (int ti = 0; ti < nti; ++ti)
    for (int tj = 0; tj < ntj; ++tj) {
      int who[4];
      const int nwho = contributors(ti, tj, who);
      std::sort(who, who + nwho, [&](int a2, int b2) { return seq_of[a2] < seq_of[b2]; });  // accumulation order = processing order
      const size_t tile = (size_t)ti * ntj + tj;
      int owner = -1, best = 0;
      for (int k = 0; k < nwho; ++k) {
        t.cover[tile] |= (uint8_t)(1u << cls[who[k]]);
        int cnt = 0;
        for (int m = 0; m < nwho; ++m) cnt += chunk_of[who[m]] == chunk_of[who[k]];
        if (cnt > best) best = cnt, owner = chunk_of[who[k]];  // ties: the chunk of the earliest contributor
      }
      int rank = 0;
      uint8_t side = 0;
      for (int k = 0; k < nwho; ++k) {
        const int i = who[k];
        const int li = (coords[2 * i] - r0) / half, lj = (coords[2 * i + 1] - c0) / half;
        const int q = 2 * (ti - li) + (tj - lj);
        if (t.direct_ok && chunk_of[i] == owner) {
          quad_of[(size_t)i * 4 + q] = quad_word(QUAD_DIRECT, (uint32_t)rank++, (uint32_t)tile);
        } else {
          quad_of[(size_t)i * 4 + q] = quad_word(QUAD_SIDE, 0, (uint32_t)tile);
          side |= (uint8_t)(1u << cls[i]);
        }
      }
      tile_info[tile] = (uint8_t)(side | (nwho ? 16 : 0));
    }
  if (v2) {  // fused plane sum: tile order (by the slot of the last contributor: the dispatch order inside a chunk)
    std::vector<std::pair<int, uint32_t>> keyed;
    for (int ti = 0; ti < nti; ++ti)
      for (int tj = 0; tj < ntj; ++tj) {
        int who[4], last = -1;
        const int nwho = contributors(ti, tj, who);
        for (int k = 0; k < nwho; ++k) last = std::max(last, seq_of[who[k]] % chunk);
        keyed.push_back({last, (uint32_t)(ti * ntj + tj)});
      }
    std::stable_sort(keyed.begin(), keyed.end(), [](const auto& a2, const auto& b2) { return a2.first < b2.first; });
    t.sum_order.resize(keyed.size());
    for (size_t i = 0; i < keyed.size(); ++i) t.sum_order[i] = keyed[i].second;
    // image prefetch lists: for every chunk, each lattice tile once, in the order the chunk's slots first touch it
    for (int x = 0; x < 8; ++x) {
      t.prefetch_first[x] = (uint32_t)t.prefetch_tiles.size();
      std::vector<char> seen((size_t)nti * ntj, 0);
      for (int s2 = std::min(n, x * chunk); s2 < std::min(n, (x + 1) * chunk); ++s2) {
        const int i = t.order[s2];
        const int li = (coords[2 * i] - r0) / half, lj = (coords[2 * i + 1] - c0) / half;
        for (int q = 0; q < 4; ++q) {
          const size_t tile = (size_t)(li + (q >> 1)) * ntj + (lj + (q & 1));
          if (!seen[tile]) seen[tile] = 1, t.prefetch_tiles.push_back((uint32_t)tile);
        }
      }
    }
    t.prefetch_first[8] = (uint32_t)t.prefetch_tiles.size();
  }
  if (t.direct_ok) {
    t.quads.resize(n);
    for (int s2 = 0; s2 < n; ++s2) std::copy_n(&quad_of[(size_t)t.order[s2] * 4], 4, t.quads[s2].q);
    t.tile_info = std::move(tile_info);
  }
  return t;
}

// Row bands of one large host frame of H rows: the lattice rows are cut into B = min(want, max_bands, lattice rows / 2) equal groups (at
// least two lattice rows per band: it runs a third, the one above); band b owns the output rows [cut[b], cut[b + 1]) and runs every patch
// that reaches into them.  in_rows[b]: image rows [0, in_rows[b]) must be resident before it runs (every np.pad mode but 'wrap' maps a
// row beyond the image edge to a row within the patch's own reach).  Returns B, or 0 where the frame is not cut.
struct RowBands {
  std::vector<int> cut, in_rows;
  std::vector<std::vector<int32_t>> patches;
};
inline int row_bands(int N, int n, const int32_t* coords, int H, int want, int max_bands, RowBands& out) {
  std::vector<int> rows;
  for (int i = 0; i < n; ++i) rows.push_back(coords[2 * i]);
  std::sort(rows.begin(), rows.end());
  rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
  const int L = (int)rows.size();
  const int B = std::min({want, max_bands, L / 2});
  if (B < 2) return 0;
  std::vector<int> cut(B + 1);
  // (equal bands: a first band of two lattice rows - an earlier first download - bought nothing, profiles/r06y_host_frame_knobs.log)
  for (int b = 0; b < B; ++b) cut[b] = b == 0 ? 0 : std::min(H, std::max(0, rows[(size_t)L * b / B]));
  cut[B] = H;
  for (int b = 0; b < B; ++b)
    if (cut[b + 1] <= cut[b]) return 0;
  out.cut = cut, out.in_rows.clear(), out.patches.assign(B, {});
  for (int b = 0; b < B; ++b) {
    int in_hi = 0;
    for (int i = 0; i < n; ++i) {
      const int r = coords[2 * i];
      if (r < cut[b + 1] && r + N > cut[b]) out.patches[b].push_back(i), in_hi = std::max(in_hi, std::min(H, r + N));
    }
    if (out.patches[b].empty()) return 0;
    out.in_rows.push_back(std::max(in_hi, cut[b + 1]));
  }
  return B;
}

// Floats of one colour plane of the resident output window
inline size_t plane_floats_needed(const rpsf_geometry& g) { return ((size_t)g.out_rows * g.width + 3) & ~(size_t)3; }

// Whether the lattice tiles cover the resident output window.  The plane sums, the direct mode's fix-up and the sweep kernel write lattice tiles
// only: pixels of the window that no tile covers are written by nobody (the reference leaves them zero), so the window is cleared first.
inline bool lattice_covers_window(int N, int lat_r0, int lat_c0, int nti, int ntj, const rpsf_geometry& g) {
  const int half = N / 2;
  const long r0 = (long)lat_r0 + g.origin_row, c0 = (long)lat_c0 + g.origin_col;
  return r0 <= g.out_row0 && r0 + (long)nti * half >= (long)g.out_row0 + g.out_rows && c0 <= 0 && c0 + (long)ntj * half >= g.width;
}

// What the persistent kernels are compiled for (patch_body2's HOT instantiation has no pixel-by-pixel rim paths): every 16-byte unit
// of a patch - four pixels of one row starting at a column that is a multiple of 4 - maps under np.pad's index map to four consecutive
// image columns (ascending or descending) or to the fill.  True for 'constant', 'symmetric' and 'wrap' when the width is a multiple of
// 4 (no unit straddles an image edge or a reflection); 'reflect' and 'edge' tear units apart.  Other launches take patch_kernel2.
// (self-contained: the patch columns themselves - lattice origin + origin_col - and the plane stride are checked here too, not left to
// fused_geometry, so that relaxing that one can never hand the HOT kernels a unit they have no path for)
// aligned16: the image pointer, the frame stride and the plane stride are multiples of 16 bytes.
inline bool hot_geometry(const rpsf_geometry& g, bool lattice, int lat_c0, bool aligned16) {
  return (g.pad_mode == RPSF_PAD_CONSTANT || g.pad_mode == RPSF_PAD_SYMMETRIC || g.pad_mode == RPSF_PAD_WRAP) && g.width % 4 == 0 &&
         g.ld_image % 4 == 0 && g.origin_col % 4 == 0 && aligned16 && lattice && ((long)lat_c0 + g.origin_col) % 4 == 0;
}

// The geometry a fused plane sum needs: every plane line written whole by one store instruction (see sum_tile), and the planes
// addressed through one 32-bit buffer offset.  out_aligned16: the output pointer is a multiple of 16 bytes.
inline bool fused_geometry(const rpsf_geometry& g, int lat_c0, bool out_aligned16) {
  return g.width % 32 == 0 && g.ld_out % 4 == 0 && ((long)lat_c0 + g.origin_col) % 32 == 0 && out_aligned16 &&
         16 * plane_floats_needed(g) < ((size_t)1 << 32);
}

}  // namespace rpsf
