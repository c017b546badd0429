// rpsf_lanes.hpp - the launch lanes of a plan, as plain C++ (no HIP: tests/emu/emu_lanes.cpp compiles it for the CPU tests).
//
// Back-to-back fused persistent applies of a 256-pixel plan alternate between two streams ("lanes"): lane 0 is the plan's public stream, lane 1 a
// second stream the plan owns.  Apply n + 1 then starts on the CUs apply n leaves idle in its last round and its tile-sum tail; apply n + 2 follows
// apply n on the same lane, so at most two applies are in flight.  What two applies in flight share is ordered per tile inside the kernels
// (DESIGN.md 3.3): the sums of an apply publish a sequence number per tile (tile_summed) and the patches of the next apply wait for it in front of
// their plane stores.  Everything that is not such an apply first JOINS the lanes - the public stream waits for lane 1 - and then runs as it always
// did.  This header decides, for every operation on a plan, which lane it takes, whether a join or a fork event is due, which queue positions the
// launch owns and which epoch and sequence number it carries; rpsf.hip turns the decisions into stream operations.
//
// A wrong base or epoch is a wait that never ends on the device, so none of this is decided anywhere else.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rpsf {

// Has the sequence number a tile carries reached `want`?  Signed difference: right across the wrap of the 32-bit counter as long as the two are less
// than 2^31 applies apart (they are at most one apart: every gated apply sums every tile).
constexpr bool lane_seq_reached(uint32_t have, uint32_t want) { return (int32_t)(have - want) >= 0; }

// The counters of the fused tile sums hold epoch x contributors (at most 4) in 32 bits
constexpr uint32_t LANE_EPOCH_LIMIT = 1u << 29;

struct LaneRange {  // bytes [lo, hi) of a caller's buffer
  uintptr_t lo = 0, hi = 0;
  bool overlaps(const LaneRange& o) const { return lo < o.hi && o.lo < hi; }
};

// Where a tile's colour planes lie depends on the geometry of the apply, not on the tile alone: the plane line length is the frame width, the
// first plane row the first output row, the lattice origin moves with the geometry's origin and the planes are a stride apart.  The gate orders
// tile t of one apply against tile t of the next, which is the same memory only while these agree.
struct LaneLayout {
  int64_t v[6] = {-1, -1, -1, -1, -1, -1};  // width, out_row0, out_rows, origin_row, origin_col, plane stride (floats)
  bool operator==(const LaneLayout& o) const {
    for (int i = 0; i < 6; ++i)
      if (v[i] != o.v[i]) return false;
    return true;
  }
};

struct LaneDraws {  // queue positions one launch takes (PatchLaunch, rpsf.hip)
  uint32_t xq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t sum = 0;
};

// What rpsf.hip does for one apply, in this order: join, fork, wait_fork, launch on `lane`
struct LanePick {
  int lane = 0;            // 0: the public stream, 1: the plan's second stream
  bool join = false;       // first: record the end of lane 1, let the public stream wait for it
  bool fork = false;       // record the fork event on the public stream in front of this launch (lane 0) ...
  bool wait_fork = false;  // ... and lane 1 waits for it before its first launch behind a join
  bool gate = false;       // the previous apply may still be in flight: the patches wait for its tile sums (sequence number seq - 1)
  uint32_t seq = 0;        // what the tile sums of this launch publish (gated kernel only)
  uint32_t xq_base[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t sum_queue_base = 0;
};

struct LaneEpoch {
  uint32_t epoch = 0;
  bool restart = false;  // the tile counters are cleared in front of this launch
};

struct LaneBook {
  bool enabled = false;  // RPSF_OPT_PIPELINE on a plan that has the gated kernel
  bool exposed = false;  // the caller has taken the public stream's handle: what it enqueues there is unknown to the plan - one lane from then on
  uint32_t xq_base[2][8] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
  uint32_t sum_queue_base[2] = {0, 0};
  uint32_t seq = 0;             // sequence number of the last launch of the gated kernel
  uint32_t done_epoch = 0;      // epoch of the last fused launch (tile_done holds epoch x contributors)
  int done_last_frames = 1;     // frames of the last fused launch
  int last_lane = -1;           // lane of the last pipelined apply since the last join; -1: the lanes are joined
  bool lane1_busy = false;      // lane 1 holds work the public stream does not wait for yet
  bool public_dirty = true;     // the public stream may hold work lane 1 is not ordered behind
  bool lane1_forked = false;    // lane 1 has waited for the fork event recorded since the last join
  LaneRange last_img, last_out;  // the caller's buffers of the last pipelined apply
  LaneLayout last_layout;        // ... and where its planes lie
  // The lane report (rpsf_plan_lane_info): host-side counts that nothing reads but a caller who asks - pipelined applies begun on either lane,
  // those of them that wait at the gate, and the joins that found lane 1 busy.  No decision depends on them.
  long begun[2] = {0, 0};
  long begun_gated = 0;
  long joins_due = 0;

  // Everything that is not a pipelined apply calls this first.  True: lane 1 has work in flight - record its end and let the public stream wait.
  // Whatever the caller enqueues next goes to the public stream, so lane 1 has to be forked from it again before its next launch.
  bool join() {
    const bool due = lane1_busy;
    lane1_busy = false, last_lane = -1, public_dirty = true;
    if (due) ++joins_due;
    return due;
  }

  // The epoch of a fused launch of `frames` frames (fused launches only).  A launch advances the counters of its own frames alone and a tile is
  // complete at epoch x contributors, so a new count starts whenever the frame count changes, and before the counters would overflow.
  bool epoch_restarts(int frames) const { return frames != done_last_frames || done_epoch + 1 >= LANE_EPOCH_LIMIT; }
  LaneEpoch next_epoch(int frames) {
    LaneEpoch e;
    e.restart = epoch_restarts(frames);
    done_last_frames = frames;
    e.epoch = done_epoch = e.restart ? 1 : done_epoch + 1;
    return e;
  }

  // One apply.  `hot`: a fused, persistent, single-frame launch of the gated kernel on the public stream that neither clears the output first nor
  // restarts the tile counters, from an entry point that lets the plan choose the stream.  `gated_kernel`: the launch runs the kernel whose tile
  // sums publish sequence numbers (hot implies it).  Queue positions are taken by commit().
  LanePick begin(bool hot, bool gated_kernel, LaneRange img, LaneRange out, const LaneLayout& layout = LaneLayout()) {
    LanePick k;
    const bool pipelined = hot && gated_kernel && enabled && !exposed;
    if (!pipelined) {
      k.join = join();
    } else {
      // the caller's own buffers: apply n + 1 must not read what apply n still writes, nor write what it still reads
      // ... and the planes: another geometry puts tile t's planes where the last apply has another tile's, which no gate guards
      if (last_lane >= 0 && (img.overlaps(last_out) || out.overlaps(last_img) || !(layout == last_layout))) k.join = join();
      k.lane = last_lane < 0 ? 0 : 1 - last_lane;
      k.gate = last_lane >= 0;
      if (k.lane == 0 && public_dirty) k.fork = true, public_dirty = false, lane1_forked = false;
      if (k.lane == 1) {
        k.wait_fork = !lane1_forked;
        lane1_forked = true, lane1_busy = true;
      }
      last_lane = k.lane, last_img = img, last_out = out, last_layout = layout;
      ++begun[k.lane];
      if (k.gate) ++begun_gated;
    }
    if (gated_kernel) k.seq = ++seq;
    for (int x = 0; x < 8; ++x) k.xq_base[x] = xq_base[k.lane][x];
    k.sum_queue_base = sum_queue_base[k.lane];
    return k;
  }

  // out (6): pipelined applies begun on lane 0, on lane 1, those begun with `gate` set, joins that were due, enabled, exposed
  void info(long out[6]) const {
    out[0] = begun[0], out[1] = begun[1], out[2] = begun_gated, out[3] = joins_due, out[4] = enabled ? 1 : 0, out[5] = exposed ? 1 : 0;
  }

  // The launch is on its way: its lane's queue counters will end `draws` further on
  void commit(const LanePick& k, const LaneDraws& draws) {
    for (int x = 0; x < 8; ++x) xq_base[k.lane][x] += draws.xq[x];
    sum_queue_base[k.lane] += draws.sum;
  }
};

}  // namespace rpsf
