// C entry points over rpsf_lanes.hpp for tests/test_lanes_host.py (test infrastructure, never shipped in the product path): the lane, join,
// queue-base, epoch and sequence-number decisions the library makes for every operation on a plan, without a GPU.
#include "../../regularizepsf_amd/csrc/rpsf_lanes.hpp"

using namespace rpsf;

static LaneBook g_book;

extern "C" void emu_lanes_reset(int enabled, uint32_t seq, uint32_t done_epoch) {
  g_book = LaneBook();
  g_book.enabled = enabled != 0, g_book.seq = seq, g_book.done_epoch = done_epoch;
}
extern "C" void emu_lanes_enable(int enabled) { g_book.enabled = enabled != 0; }
extern "C" void emu_lanes_expose() { g_book.exposed = true; }
extern "C" void emu_lanes_set_exposed(int exposed) { g_book.exposed = exposed != 0; }  // (RPSF_OPT_PIPELINE set to 1 again arms the lanes)
extern "C" int emu_lanes_join() { return g_book.join() ? 1 : 0; }
extern "C" int emu_lanes_epoch_restarts(int frames) { return g_book.epoch_restarts(frames) ? 1 : 0; }
// out (2): epoch, restart
extern "C" void emu_lanes_next_epoch(int frames, int64_t* out) {
  const LaneEpoch e = g_book.next_epoch(frames);
  out[0] = e.epoch, out[1] = e.restart;
}
// out (16): lane, join, fork, wait_fork, gate, seq, gate_want (= seq - 1 as the kernel gets it), sum_queue_base, xq_base[8]
// layout (6): width, out_row0, out_rows, origin_row, origin_col, plane stride of the apply's geometry
extern "C" void emu_lanes_begin(int hot, int gated_kernel, uint64_t img_lo, uint64_t img_hi, uint64_t out_lo, uint64_t out_hi, const int64_t* layout,
                                int64_t* out) {
  LaneLayout lay;
  for (int i = 0; i < 6; ++i) lay.v[i] = layout[i];
  const LanePick k = g_book.begin(hot != 0, gated_kernel != 0, LaneRange{(uintptr_t)img_lo, (uintptr_t)img_hi}, LaneRange{(uintptr_t)out_lo, (uintptr_t)out_hi}, lay);
  out[0] = k.lane, out[1] = k.join, out[2] = k.fork, out[3] = k.wait_fork, out[4] = k.gate, out[5] = k.seq, out[6] = (uint32_t)(k.seq - 1);
  out[7] = k.sum_queue_base;
  for (int x = 0; x < 8; ++x) out[8 + x] = k.xq_base[x];
}
extern "C" void emu_lanes_commit(int lane, const uint32_t* xq_draws, uint32_t sum_draws) {
  LanePick k;
  k.lane = lane;
  LaneDraws d;
  for (int x = 0; x < 8; ++x) d.xq[x] = xq_draws[x];
  d.sum = sum_draws;
  g_book.commit(k, d);
}
// out (6): as rpsf_plan_lane_info - applies begun on lane 0, on lane 1, begun with the gate set, joins that were due, enabled, exposed
extern "C" void emu_lanes_info(int64_t* out) {
  long v[6];
  g_book.info(v);
  for (int i = 0; i < 6; ++i) out[i] = v[i];
}
extern "C" int emu_lanes_seq_reached(uint32_t have, uint32_t want) { return lane_seq_reached(have, want) ? 1 : 0; }
