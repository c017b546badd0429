// C entry points over rpsf_lattice.hpp for tests/test_lattice_host.py (test infrastructure, never shipped in the product path): the
// tables the library uploads at plan creation, the row bands of a host frame and the launch form a frame geometry selects, without a GPU.
#include <cstring>

#include "../../regularizepsf_amd/csrc/rpsf_lattice.hpp"

using namespace rpsf;

static LatticeTables g_t;
static RowBands g_b;

template <class T>
static int64_t put(const std::vector<T>& v, void* dst) {
  if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(T));
  return (int64_t)(v.size() * sizeof(T));
}

// parent: null, or {r0, c0, lattice} of a view's parent.  scalars (16): lattice, direct_ok, r0, c0, nti, ntj, par_j, prefetch_first[9]
extern "C" void emu_lattice_build(int N, int n, const int32_t* coords, const int32_t* k_index, int v2, const int32_t* parent, int64_t* scalars) {
  const LatticeParent par = parent ? LatticeParent{parent[0], parent[1], parent[2] != 0} : LatticeParent{};
  g_t = lattice_build(N, n, coords, k_index, v2 != 0, parent ? &par : nullptr);
  const int64_t s[7] = {g_t.lattice, g_t.direct_ok, g_t.r0, g_t.c0, g_t.nti, g_t.ntj, g_t.par_j};
  std::copy_n(s, 7, scalars);
  std::copy_n(g_t.prefetch_first, 9, scalars + 7);
}

// Table `which` of the last build (dst null: the size alone); returns its bytes
extern "C" int64_t emu_lattice_fetch(int which, void* dst) {
  switch (which) {
    case 0: return put(g_t.order, dst);
    case 1: return put(g_t.desc, dst);
    case 2: return put(g_t.cover, dst);
    case 3: return put(g_t.tile_info, dst);
    case 4: return put(g_t.quads, dst);
    case 5: return put(g_t.sum_order, dst);
    case 6: return put(g_t.prefetch_tiles, dst);
    case 7: return put(g_t.sweep_slot, dst);
    case 8: return put(g_t.cell, dst);
    default: return -1;
  }
}

extern "C" int emu_lattice_bands(int N, int n, const int32_t* coords, int H, int want, int max_bands) {
  g_b = RowBands();
  return row_bands(N, n, coords, H, want, max_bands, g_b);
}
// 0: cut, 1: in_rows, 2 + b: the patches of band b
extern "C" int64_t emu_lattice_bands_fetch(int which, void* dst) {
  if (which == 0) return put(g_b.cut, dst);
  if (which == 1) return put(g_b.in_rows, dst);
  return which - 2 < (int)g_b.patches.size() ? put(g_b.patches[which - 2], dst) : -1;
}

// The launch form of a whole H x W frame (ld = W, origin 0, aligned buffers, one frame) on a default second-generation plan over these
// corners: 0 separate plane sum, 1 fused with one patch per workgroup, 2 persistent + fused; bit 2: the lattice covers the frame
extern "C" int emu_lattice_launch(int N, int n, const int32_t* coords, int H, int W, int pad_mode) {
  const LatticeTables t = lattice_build(N, n, coords, nullptr, true, nullptr);
  rpsf_geometry g{};
  g.height = H, g.width = W, g.ld_image = W, g.ld_out = W, g.pad_mode = pad_mode, g.image_rows = H, g.out_rows = H;
  const bool fused = t.lattice && fused_geometry(g, t.c0, true);
  const bool hot = hot_geometry(g, t.lattice, t.c0, true);
  return (fused ? (hot ? 2 : 1) : 0) | (t.lattice && lattice_covers_window(N, t.r0, t.c0, t.nti, t.ntj, g) ? 4 : 0);
}
