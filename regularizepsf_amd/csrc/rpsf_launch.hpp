// rpsf_launch.hpp - what the patch launch of one apply is, as plain C++ (no HIP, no plan: tests/emu/emu_launch.cpp compiles it for the CPU tests).
//
// A fused apply of a 128- or 256-pixel plan is one grid whose workgroups take their role from their block index (patch_body2, rpsf_kernels2.hpp):
// head summing workgroups, patch workgroups - persistent ones that draw their slots from the eight chunk queues, or one per slot and frame -
// and, in the form that is not persistent, tail summing workgroups.  This header decides how many of each there are, the grid, and how many
// positions the launch draws from every never-reset queue word; LaneBook::commit (rpsf_lanes.hpp) adds those counts to the bases of the next
// launch.  A count that is not what the kernels draw, or a grid whose first resident workgroups all wait, is a wait that never ends on the
// device, so none of this is decided anywhere else; tests/test_launch_host.py replays every decision on a model of the device side.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace rpsf {

// Patches one workgroup of the patch kernels processes (first generation: 64-thread workgroups shared by several small patches), and
// the patches per XCD chunk that follow from it: an eighth of the plan's, in whole workgroups.  The processing order, the prefetch
// lists and the fused tile order are cut by it (lattice_build) and the kernels index by it (PatchParams::chunk).
constexpr int patch_teams(int N) { return N * N / 2 / 64 >= 64 ? 1 : 64 / (N * N / 2 / 64); }
inline int chunk_patches(int n_patches, int teams) { return ((n_patches + 7) / 8 + teams - 1) / teams * teams; }

// A patch launch is one grid of at most 2^31 - 1 workgroups: one per frame and patch_teams() patches of each chunk
inline bool patch_launch_too_large(int N, int n_patches, int frames) {
  const int teams = patch_teams(N);
  return (size_t)8 * (chunk_patches(n_patches, teams) / teams) * frames > 0x7fffffffu;
}

// The plan, the chip and the apply as the decision sees them
struct LaunchInput {
  int N = 256;
  bool gen2 = true;        // a second-generation kernel (the only ones with a fused form)
  int wg_threads = 512;    // first generation: stagger_blocks counts 512-thread shares of a CU
  int n_patches = 0;
  int tiles = 0;           // lattice tiles (nti x ntj): positions of the tile list per frame
  int frames = 1;
  int wgs_per_cu = 1;      // resident workgroups of the patch kernel per CU
  int cu_count = 256;      // the plan's CUs (rpsf_plan_set_cu_mask)
  int round_capacity = 0;  // patches the plan's CUs hold at once: cu_count x wgs_per_cu x patch_teams
  int reserved_cus = 0;
  int sum_first = -1;      // RPSF_SUM_FIRST override (a multiple of 8), -1 = none
  int head_patches = 0;
  bool persist = false, fused = false;
  bool hot_geometry = false;  // the geometry the persistent kernels are compiled for (hot_geometry, rpsf_lattice.hpp)
  bool out_span_ok = true;    // the output window lies within one 32-bit buffer offset (asked of the 256-pixel plan alone)
  size_t planes_floats = 0;
  bool k_cached = false;
  int plane_nt_opt = -1;      // RPSF_OPT_PLANE_NT, -1 = none
  int frame_major_opt = -1;   // RPSF_FRAME_MAJOR (development sweeps: 0 = never, 2 = any persistent batch), -1 = none
  int stagger_us = -1;        // < 0: by the amount of work
  bool prefetch = false;      // the image prefetch is on and the plan has its tile lists
  int k_prefetch = 0;
};

// What the patch launch of one apply is, but for the lane it takes (PatchLaunch, rpsf.hip)
struct LaunchDecision {
  // first generation / second generation, patches only / fused: summing workgroups behind (and sum_first beside) the patches / persistent: patch
  // workgroups that draw their slots from per-XCD queues and end as summing ones
  enum Form { GEN1, GEN2, FUSED, PERSISTENT } form;
  enum Variant { PLAIN, K_CACHED, K_CACHED_PLANES_NT } variant;  // persistent: PersistentKernel2's fn / fn_k_cached / fn_k_cached_planes_nt
  unsigned grid;      // workgroups
  int chunk;          // patches per XCD chunk
  int patch_blocks;   // second generation: workgroups [sum_first, sum_first + patch_blocks) of a launch that is not persistent process patches
  int stagger_ticks, stagger_blocks;
  int sum_first, frame_major, plane_nt;  // fused and persistent
  int rows, head_patches, prefetch;      // persistent: patch workgroups per XCD, ...
  int k_prefetch;                        // persistent, 256-pixel plan: first-round K prefetch by the head summing workgroups (0 / 1)
  uint32_t xq_draws[8];                  // persistent: how many draws this launch makes from the slot queue of each XCD
  uint32_t sum_queue_draws;              // fused and persistent: the same for the tile queue
};

// Summing workgroups that run beside the patches from the start of a fused launch (multiple of 8: one per XCD), by the
// amount of work in the launch.  256-pixel plan (512-thread workgroups, one per CU): r02y, a band of 520 patches 130-138 us
// with 8, 131-146 with 32; r02av, plane stores kept in the Infinity Cache: 4096^2 0.193 / 0.190 / 0.196 ms with 8 / 16 / 24,
// 8192^2 0.78 / 0.77 / 0.74 / 0.765 ms with 8 / 16 / 32 / 48 - the sooner a tile is summed, the likelier its planes are still
// cached.  128-pixel plan (128-thread workgroups, four per CU): 4096^2 0.217 / 0.214 / 0.212 / 0.206 ms with 16 / 64 / 96 / 128
// against 0.218 ms with the separate sum kernel; 2048^2 0.067 ms with 0 ... 24 against 0.069; 8 x 2048^2 0.372 / 0.360 / 0.352 /
// 0.343 / 0.340 ms with 8 / 32 / 64 / 128 / 192 against 0.362.
inline int sum_first_for(const LaunchInput& in) {
  if (in.sum_first >= 0) return in.sum_first;
  const long work = (long)in.n_patches * in.frames;
  if (in.N == 128) return work >= 4096 ? 160 : work >= 2048 ? 128 : work >= 512 ? 8 : 0;  // (160 from 4096 patch-frames on: -2 ... -4 %, profiles/r04bf)
  return work >= 2048 ? 32 : work >= 1024 ? 16 : work >= 512 ? 8 : 0;
}

inline LaunchDecision launch_decide(const LaunchInput& in) {
  const bool N256 = in.gen2 && in.N == 256, N128 = in.gen2 && in.N == 128;
  const int teams = patch_teams(in.N);
  LaunchDecision L{};
  L.chunk = chunk_patches(in.n_patches, teams);
  L.stagger_ticks = std::max(0, in.stagger_us) * 100;
  L.grid = (unsigned)((size_t)8 * (L.chunk / teams) * in.frames);  // (patch_launch_too_large: it fits)
  L.form = in.gen2 ? LaunchDecision::GEN2 : LaunchDecision::GEN1;
  L.stagger_blocks = in.gen2 ? in.round_capacity : in.cu_count * std::max(1, 512 / in.wg_threads);
  L.patch_blocks = in.gen2 ? (int)L.grid : 0;  // (the first-generation kernel does not read it)
  if (!in.fused) return L;                     // (fused: second-generation plans only, launch_apply)
  const int count = in.tiles * in.frames;      // positions of the tile list
  // Persistent batches whose planes would not fit the Infinity Cache side by side run frame after frame in one launch: every
  // frame keeps the cache behaviour of a single apply, and the next frame's patches take the CUs the previous one's last
  // patches leave idle (RPSF_FRAME_MAJOR=0/1 overrides).
  bool frame_major = N256 && in.persist && in.frames > 1 && in.n_patches >= 1024 &&
                     16.0 * (double)in.planes_floats * in.frames > 256.0 * 1048576.0;  // (8 x 2048^2: 0.056 ms per frame side by side, 0.061 in turn)
  if (in.frame_major_opt >= 0)  // development sweeps: 0 = never, 2 = any persistent batch
    frame_major = in.frame_major_opt == 2 ? (in.persist && in.frames > 1) : (frame_major && in.frame_major_opt != 0);
  L.frame_major = frame_major ? 1 : 0;
  // Frames of a batch side by side keep the planes of ALL of them live at once (8 x 2048^2: 537 MB against a 256 MiB Infinity Cache): the 128-pixel
  // kernels then store them with the streaming hint - 0.3156 -> 0.3009 ms (-4.7 %); a single frame loses 8 % that way, and so does the 256-pixel
  // plan at either size (profiles/r04bd).  RPSF_PLANE_NT=0/1 overrides (development sweeps).
  // (needs the plain-load form of K - a batch shares it - and planes well beyond the Infinity Cache: 4 x 2048^2, 268 MB, still loses 3 %; 6 x, 403 MB, gains 5 %)
  L.plane_nt = N128 && in.k_cached && in.frames > 1 && !frame_major && 16.0 * (double)in.planes_floats * in.frames > 300.0 * 1048576.0;
  if (in.plane_nt_opt >= 0) L.plane_nt = in.plane_nt_opt != 0 && N128 && in.k_cached;  // (RPSF_OPT_PLANE_NT)
  const int tune_frames = in.frames;  // (the settings of a single apply measured worse here: 0.203 vs 0.186 ms per frame at 8 x 4096^2)
  // (where the launch's draws start - sum_queue_base, xq_base - depends on the lane it takes: launch_apply fills them in, rpsf_lanes.hpp)
  // persistent form: as many patch workgroups as the chip holds beside the summing ones; each works through the slots
  // of its XCD's chunk and ends as a summing workgroup itself (no workgroups behind the patches).
  // FORWARD PROGRESS.  HIP promises neither that a grid is resident as a whole nor an order of dispatch, and other launches
  // (a second plan on another stream, RCCL's kernels) may hold CUs.  What this launch needs: (1) every patch slot is drawn
  // from its chunk's queue - none is tied to a particular workgroup - so the slots of chunk x are worked off by whichever
  // workgroups with blockIdx % 8 == x are resident, and a workgroup turns to summing only when its chunk's queue is empty,
  // i.e. when every remaining patch of the chunk is in the hands of a resident workgroup that does not wait for anything;
  // (2) summing workgroups wait (poll + s_sleep) only for tiles whose patches are drawn or will be drawn by (1).  So the
  // launch completes as soon as, for every chunk that holds a patch, ONE patch workgroup gets a CU: in dispatch order the first
  // sum_first + (chunks that hold a patch) workgroups.  The only workgroups that hold a CU without progress of their own are the sum_first
  // head summing ones (<= 32 of 512 threads for the 256-pixel plan; up to 160 of 128 threads - four to a CU, 40 CUs' worth - for the
  // 128-pixel plan from 4096 patch-frames on, sum_first_for); concurrent persistent launches therefore cannot starve one another unless their
  // head summing workgroups alone fill the chip (tests: test_two_persistent_plans_on_two_streams, 256- and 128-pixel plans).
  // WHAT THIS DOES NOT COVER: a plan masked to a few CUs (rpsf_plan_set_cu_mask admits 8).  sum_first follows the amount of work, not the
  // budget, and max(1, ...) below hides the deficit: where the plan's CUs hold fewer workgroups than sum_first + the chunks that hold a patch
  // (the form that is not persistent: sum_first + 1), the first resident workgroups all wait for patches that are never dispatched.  The
  // model of tests/test_launch_host.py shows the stall exactly there (a 256-pixel plan on 8 ... 15 CUs from 512 patch-frames on, 8 ... 39 from
  // 2048 on; a 128-pixel plan on 8 ... 41 CUs from 4096 on).  Capping sum_first by that count is NOT enough on the device: workgroups are
  // dealt round-robin over the XCDs, a workgroup can only take a place on its own XCD, and a mask need not leave the XCDs the same number of
  // CUs - 32 head summing workgroups and 8 patch workgroups on 40 masked CUs did not finish on an MI355X (profiles/launch_budget_gpu.log).
  // What holds for any mask is per XCD: sum_first / 8 + 1 places on the XCD the mask leaves the fewest.  Until the decision knows the
  // device's CU count and is modelled per XCD, masks are for budgets close to the whole chip (include/rpsf.h).
  // (queue positions of an XCD: chunk slots x frames, the frames of a slot side by side)
  L.sum_first = sum_first_for(in);
  const int rows = std::min(L.chunk * in.frames, std::max(1, (in.round_capacity - L.sum_first - in.reserved_cus) / 8));
  // (the gated kernel - the persistent 256-pixel one - stores the output through one 32-bit buffer offset, as every fused launch does its planes)
  if (!(in.persist && rows > 0 && in.out_span_ok && in.hot_geometry)) {
    L.form = LaunchDecision::FUSED;
    const int nsum = std::max(8, std::min(count, in.round_capacity)) + L.sum_first;  // at the tail: as many summing workgroups as the chip holds
    L.sum_queue_draws = (uint32_t)(count + nsum);  // every workgroup draws one position past the end
    L.grid += (unsigned)nsum;
    return L;
  }
  L.form = LaunchDecision::PERSISTENT, L.rows = rows;
  L.variant = !in.k_cached ? LaunchDecision::PLAIN : L.plane_nt ? LaunchDecision::K_CACHED_PLANES_NT : LaunchDecision::K_CACHED;
  // a head summing workgroup would idle through the first patch period (no tile is complete before that): it computes one patch
  // of its XCD's chunk first (RPSF_HEAD_PATCHES=0: off)
  L.head_patches = in.head_patches;
  L.prefetch = in.prefetch ? 1 : 0;
  L.k_prefetch = N256 && !L.head_patches ? in.k_prefetch : 0;
  // persistent workgroups keep the phase they start with: holding the resident ones back by up to 10 us spreads the
  // store bursts of the chip over the patch period (profiles/r02ai, r02ak: -2..3 % from four rounds of patches on; with the
  // plane stores kept in the Infinity Cache, r02av: 0.210 / 0.208 / 0.193 / 0.190 / 0.189 / 0.191 / 0.195 ms at 0 / 5 / 8 / 10 / 12 / 15 / 20 us)
  // (and smaller launches too: 2048^2 0.0811 -> 0.0787 ms, 3072^2 0.138 -> 0.131 ms, a band of 520 patches 128 -> 121 us)
  // (long launches take more: 8192^2 0.736 / 0.726 / 0.714 / 0.703 / 0.698 / 0.719 ms at 6 / 12 / 18 / 24 / 30 / 36 us)
  // (round 4, seven-barrier pass, profiles/r04az: 4096^2 at 12 / 16 / 20 us - the repeated frame 0.1835 / 0.1843 / 0.1880 ms, a NEW frame every step
  // 0.2019 / 0.1962 / 0.1933: 16 us from 1024 patches of the 256-pixel plan on; 8192^2 0.714 / 0.688 / 0.691 / 0.690 at 12 / 16 / 20 / 24)
  if (in.stagger_us < 0 && (long)in.n_patches * tune_frames >= 256) {
    const long work = (long)in.n_patches * tune_frames;
    L.stagger_ticks = work >= 2048 ? 2400 : (work >= 1024 && N256) ? 1600 : 1200;
    // The 128-pixel plan - four workgroups per CU, out of step with one another anyway - is better off WITHOUT it since round 4 (profiles/r04ba):
    // 2048^2 0.0655 -> 0.0603 ms (-8 %), 3072^2 -6 %, 8 x 2048^2 0.3252 -> 0.3198; only single frames of 4096^2 and more still take a short one
    // (6 us: -1 ... -3 %).
    if (N128) L.stagger_ticks = tune_frames == 1 && in.n_patches >= 4096 ? 600 : 0;
  }
  for (int x = 0; x < 8; ++x) {
    // draws of this launch: one per slot and frame, plus the one past the end that tells each of the chunk's workgroups to stop
    // (the first sum_first / 8 positions of a chunk go to the head summing workgroups without a draw when those compute a patch first)
    const int slots_x = std::min(L.chunk, std::max(0, in.n_patches - x * L.chunk)) * in.frames;
    L.xq_draws[x] = (uint32_t)(std::max(0, slots_x - (L.head_patches ? L.sum_first / 8 : 0)) + rows);
  }
  const int wgs = L.sum_first + 8 * rows;
  L.sum_queue_draws = (uint32_t)(count + wgs);  // every workgroup draws one position past the end
  L.grid = (unsigned)wgs;
  return L;
}

}  // namespace rpsf
