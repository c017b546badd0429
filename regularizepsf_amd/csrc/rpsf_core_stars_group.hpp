// rpsf_core_stars_group.hpp - which stars are fitted together (DESIGN.md 3.7 "Group fits"): the connected components of the graph that
// links two stars no further apart than a link distance.  Plain C++ for the host, no GPU, as rpsf_lattice.hpp; csrc/stars.hip
// (rpsf_stars_link_groups, rpsf_stars_fit_groups) and the CPU emulator tests/emu/emu_group.cpp share it.
//
// LINKING.  Two eligible stars i < j are linked when dy dy + dx dx <= L L, with dy = y_i - y_j, dx = x_i - x_j, in float64 and nothing
// fused.  An ineligible star links to nobody.  LABELS.  label[i] is the smallest index of i's component, size[i] the component's size as
// found.  A component of more than max_group members is broken up: every member is fitted alone, is `crowded`, and keeps the size.  The
// components of 2 .. max_group members come out as a CSR list, groups in ascending label and members in ascending index.
//
// COST.  Expected linear time: the stars are binned into a hashed grid of cells of side s >= L (a dense grid will not do: |y|, |x| reach
// 2^20 and L may be small), each star is compared with the later stars of its own and the eight neighbouring cells, and a union-find whose
// roots are always the smallest index of their tree joins them.  The result is a property of the graph: it does not depend on the order
// in which cells or pairs are visited.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <unordered_map>
#include <vector>

#pragma clang fp contract(off)

namespace rpsfq {

constexpr int MAX_GROUP = 8;
constexpr int FLAG_CROWDED = 16;  // beside S8's flags 1, 2, 4, 8 (RPSF_STARS_FIT_CROWDED of include/rpsf.h)

struct Groups {
  std::vector<int32_t> label, size;
  std::vector<uint8_t> crowded;
  std::vector<long long> starts;  // group k has members[starts[k] .. starts[k + 1])
  std::vector<int32_t> members;
  size_t count() const { return starts.empty() ? 0 : starts.size() - 1; }
};

// what is wrong with the link distance or max_group for fit discs of radius R (null: nothing); beyond 2 R two discs share no pixel
inline const char* group_problem(double link, int max_group, double radius) {
  if (!(link > 0.0) || !(link <= 2.0 * radius)) return "link must lie in 0 < link <= 2 R";
  if (max_group < 1 || max_group > MAX_GROUP) return "max_group must lie in 1 ... 8";
  return nullptr;
}
// the same without a radius (rpsf_stars_link_groups): any finite positive distance
inline const char* link_problem(double link, int max_group) {
  if (!(link > 0.0) || !(std::fabs(link) <= 1.7976931348623157e308)) return "link must be positive and finite";
  if (max_group < 1 || max_group > MAX_GROUP) return "max_group must lie in 1 ... 8";
  return nullptr;
}

inline bool linked(double y0, double x0, double y1, double x1, double L2) {
  const double dy = y0 - y1, dx = x0 - x1;
  return dy * dy + dx * dx <= L2;
}

// pos[2 i ..] = (y, x), finite with |y|, |x| < 2^20; eligible may be null (every star is eligible)
inline void link_groups(size_t n, const double* pos, const uint8_t* eligible, double L, int max_group, Groups& out) {
  out.label.assign(n, 0), out.size.assign(n, 1), out.crowded.assign(n, 0);
  out.starts.assign(1, 0), out.members.clear();
  if (n == 0) return;
  const double L2 = L * L;
  // the side of a grid cell: L, but not so small that a cell coordinate leaves 32 bits (|y| / s < 2^30); s >= L is all the search needs
  const double side = L < 0x1p-10 ? 0x1p-10 : L;
  auto key_of = [](long long cy, long long cx) { return ((uint64_t)(cy + (1LL << 31)) << 32) | (uint64_t)(cx + (1LL << 31)); };
  std::vector<long long> cy(n), cx(n);
  std::unordered_map<uint64_t, int32_t> cell_of;  // grid cell -> its number, in the order of first appearance
  cell_of.reserve(2 * n);
  std::vector<int32_t> star_cell(n, -1);
  std::vector<long long> cell_start(1, 0);
  for (size_t i = 0; i < n; ++i) {
    if (eligible && !eligible[i]) continue;
    cy[i] = (long long)std::floor(pos[2 * i] / side), cx[i] = (long long)std::floor(pos[2 * i + 1] / side);
    const auto found = cell_of.emplace(key_of(cy[i], cx[i]), (int32_t)cell_of.size());
    star_cell[i] = found.first->second;
    if (found.second) cell_start.push_back(0);
    ++cell_start[(size_t)star_cell[i] + 1];
  }
  const size_t n_cells = cell_of.size();
  for (size_t k = 0; k < n_cells; ++k) cell_start[k + 1] += cell_start[k];
  std::vector<int32_t> cell_stars((size_t)cell_start[n_cells]);  // per cell its stars, ascending
  {
    std::vector<long long> next(cell_start.begin(), cell_start.end() - 1);
    for (size_t i = 0; i < n; ++i)
      if (star_cell[i] >= 0) cell_stars[(size_t)next[(size_t)star_cell[i]]++] = (int32_t)i;
  }
  std::vector<int32_t> parent(n);
  for (size_t i = 0; i < n; ++i) parent[i] = (int32_t)i;
  auto find = [&](int32_t i) {
    while (parent[(size_t)i] != i) i = parent[(size_t)i] = parent[(size_t)parent[(size_t)i]];
    return i;
  };
  for (size_t i = 0; i < n; ++i) {
    if (star_cell[i] < 0) continue;
    for (long long dy = -1; dy <= 1; ++dy)
      for (long long dx = -1; dx <= 1; ++dx) {
        const auto at = cell_of.find(key_of(cy[i] + dy, cx[i] + dx));
        if (at == cell_of.end()) continue;
        for (long long k = cell_start[(size_t)at->second]; k < cell_start[(size_t)at->second + 1]; ++k) {
          const size_t j = (size_t)cell_stars[(size_t)k];
          if (j <= i || !linked(pos[2 * i], pos[2 * i + 1], pos[2 * j], pos[2 * j + 1], L2)) continue;
          const int32_t a = find((int32_t)i), b = find((int32_t)j);
          if (a < b)
            parent[(size_t)b] = a;  // the root of a tree is its smallest index
          else if (b < a)
            parent[(size_t)a] = b;
        }
      }
  }
  std::vector<int32_t> members_of(n, 0);
  for (size_t i = 0; i < n; ++i) out.label[i] = find((int32_t)i), ++members_of[(size_t)out.label[i]];
  std::vector<long long> slot(n, -1);  // per root of a group: where its next member goes
  for (size_t i = 0; i < n; ++i) {
    const int32_t size = members_of[(size_t)out.label[i]];
    out.size[i] = size, out.crowded[i] = size > max_group;
    if ((size_t)out.label[i] == i && size >= 2 && size <= max_group) slot[i] = out.starts.back(), out.starts.push_back(out.starts.back() + size);
  }
  out.members.assign((size_t)out.starts.back(), 0);
  for (size_t i = 0; i < n; ++i) {
    long long& at = slot[(size_t)out.label[i]];
    if (at >= 0) out.members[(size_t)at++] = (int32_t)i;
  }
}

}  // namespace rpsfq
