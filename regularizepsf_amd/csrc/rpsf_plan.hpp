// rpsf_plan.hpp - what the host units of librpsf_hip.so that see a plan share (csrc/rpsf.hip, rpsf_host.hip, rpsf_saturated.hip,
// rpsf_construct.hip): the development-environment switch, the owning device array, struct rpsf_plan with its per-path state, the
// compiled patch plans as the host sees them with their table upload, and the declarations of the functions that cross these units.
// Errors: fail / HIP_TRY of rpsf_side_unit.hpp.  The units that need no plan (rpsf_shard.hip and the side units) do not include this.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "rpsf_device.hpp"
#include "rpsf_hostpipe.hpp"
#include "rpsf_lanes.hpp"
#include "rpsf_lattice.hpp"
#include "rpsf_saturation.hpp"
#include "rpsf_side_unit.hpp"

RPSF_PLANS_V1(RPSF_DECL_V1)
RPSF_PLANS_V2(RPSF_DECL_V2)
RPSF_PLANS_V3(RPSF_DECL_V3)

// Development sweeps read their knobs from the environment ONLY in builds made with -DRPSF_DEV_ENV (scripts/, never the product): a stray variable
// in a production environment must not change which kernel runs.  The shipped library reads two variables, both about the host-side thread pool
// (rpsf_hostpipe.hpp: RPSF_HOST_THREADS, RPSF_HOST_AFFINITY, documented in include/rpsf.h); everything a caller or a test may want to
// choose is a plan option (rpsf_plan_set_option).
static const char* dev_env(const char* name) {
#if defined(RPSF_DEV_ENV)
  return std::getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

// One device allocation of T[count], owned by the handle (move-only) and freed with it.  Free = hipHostFree: page-locked host memory.
// For what is sized once and replaced whole (Buf, rpsf_side_unit.hpp: scratch kept between calls that only grows).
template <class T, hipError_t (*Free)(void*) = hipFree>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p, o.p);
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)Free(p);
    p = nullptr;
  }
  hipError_t alloc(size_t count) {
    reset();
    return hipMalloc(&p, count * sizeof(T));
  }
  hipError_t upload(const T* host, size_t count) {
    const hipError_t e = alloc(count);
    return e != hipSuccess ? e : hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice);
  }
  operator T*() const { return p; }
};

struct PipeRelease {
  void operator()(rpsf_host::HostPipe* q) const {
    q->destroy();
    delete q;
  }
};
struct FftPlanRelease {
  void operator()(void* h) const;  // hipfftDestroy (g_hipfft, below)
};
struct SatDeviceRelease {
  void operator()(SatDevice* d) const { rpsf_sat_destroy(d); }
};

// Host scratch of the saturation branch (rpsf_apply_host_saturated), per staging slot, kept between calls
struct SatScratch {
  std::vector<double> padded;
  std::vector<uint8_t> mask;
  struct Raw {
    int64_t idx;
    double value;
  };
  std::vector<Raw> raw;
};

// ------------------------------------------------------------------------------------------------
// plan
// ------------------------------------------------------------------------------------------------
// The fallback through hipFFT: any patch size without a compiled kernel
struct FftPath {
  DevBuf<cf> d_kfull;       // the caller's K, (n, N, N) complex64, unfolded
  DevBuf<cf> d_buf;         // chunk x N x N complex work buffer
  DevBuf<float> d_win;
  DevBuf<uint8_t> d_colour;  // colour class per patch when the corners allow one (generic_colours), else null: atomic adds
  std::unique_ptr<void, FftPlanRelease> plan;  // hipfftHandle for `chunk` patches
  int chunk = 0;
};

// The patch kernels: first generation (N = 16 ... 64, colour planes or atomics) and second (N = 128, 256: fused plane sum, persistent
// queues, opt-in direct mode).  A view's tables and packed K are its parent's (owner()).
struct PatchPath {
  DevBuf<uint16_t> d_tab;
  DevBuf<uint32_t> d_pairtab;
  DevBuf<cf> d_tw;
  DevBuf<cf> d_g, d_gs;
  size_t g_elems = 0, gs_elems = 0;
  DevBuf<unsigned long long> d_stamps;
  DevBuf<float> d_sink;  // write-only scratch for the out-of-image pixels of rim patches
  int stagger_us = -1;  // -1: automatic (12 us for persistent launches of 256 patches and more, else none)
  int round_capacity = 0;  // patches the chip holds at once (CUs x resident workgroups x patches per workgroup)
  bool direct_ok = false;  // lattice and one patch per workgroup
  bool v2 = false;         // second-generation kernel (rpsf_core2.hpp): N = 128, 256
  // Fused plane sum (second-generation kernels, one frame, aligned geometry): the workgroups behind the patches in the
  // grid sum a lattice tile as soon as all its contributors have published their (write-through) plane stores, so
  // the sum runs on the CUs the partial last round leaves idle and no second kernel is needed.
  DevBuf<uint32_t> d_tile_done;   // per tile: contributors done, never reset (epoch * contributors after every apply; the epoch: lanes.done_epoch)
  DevBuf<uint32_t> d_sum_order;   // all tiles, the ones whose contributors run first first
  size_t done_frames = 1;            // frames the tile counters are sized for (batches: one set per frame)
  DevBuf<uint32_t> d_sum_queue;   // position in d_sum_order, never reset: one word per launch lane, each on a 128-byte line of its own
  // Launch lanes (rpsf_lanes.hpp): which stream an apply takes, where the lanes join, the queue positions each lane's launches own, the epoch of
  // the tile counters and the sequence number of the gate
  LaneBook lanes;
  DevBuf<uint32_t> d_tile_summed;  // per tile: sequence number of the last apply whose sum of the tile is complete (gated kernel: patch_kernel2_256p)
  bool no_fuse = false;
  int sum_first = -1;                // RPSF_SUM_FIRST override of sum_first_for(), -1 = none
  bool prefetch = false;             // persistent launches: head summing workgroups touch the image first (RPSF_PREFETCH)
  DevBuf<uint32_t> d_prefetch_tiles;  // per chunk: lattice tiles in the order the chunk's patches first need them
  uint32_t prefetch_first[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int k_prefetch = 0;                // (measured a loss, DESIGN.md 5.10: off) 256-pixel persistent launches: the head summing workgroups touch the first
                                     // round's K before they sum (RPSF_OPT_HEAD_KPREFETCH)
  int head_patches = 0;              // (measured neutral, profiles/r03i: off) persistent launches: patches a head summing workgroup computes before it sums (RPSF_HEAD_PATCHES)
  bool fuse_pays = false;            // the second-generation plans (N = 128, 256)
  // Persistent patch workgroups (patch_kernel2_256p; fused launches of the 256-pixel plan): per-XCD slot queues, never reset
  bool persist = false;
  bool k_cached = false;             // 128-pixel persistent launches take patch_kernel2_128pc (plain loads of the pair words): see rpsf_plan_create
  int reserved_cus = 0;              // persistent launches leave this many CUs without a patch workgroup (rpsf_plan_set_reserved_cus)
  DevBuf<uint32_t> d_xq;          // 8 counters per launch lane, one per 128-byte line (their bases: lanes.xq_base)
  DevBuf<uint4> d_quads;        // per processing-order slot: quadrant words (rpsf_core.hpp, store_patch_direct)
  DevBuf<uint8_t> d_tile_info;  // per lattice tile: static side mask | 16 if any patch covers it
  DevBuf<uint32_t> d_flags;     // per (frame, tile)
  DevBuf<uint32_t> d_dyn;       // per (frame, tile)
  DevBuf<uint32_t> d_chunk_xcc; // 8 words
  size_t flag_frames = 0;
  uint32_t epoch = 0;
  int orphan_mod = 0;              // testing aid (RPSF_OPT_DEBUG_ORPHAN)
  int plane_nt_opt = -1;           // rpsf_plan_set_option; -1: the library decides
  DevBuf<float> d_planes;
  size_t planes_floats = 0;  // per plane
  size_t planes_frames = 0;  // frames the allocation holds (4 planes each)
};

// The sweep kernel (third generation, rpsf_kernels3.hpp, N <= 64 on a complete lattice of at least 2 x 2 patches): regions, job lists,
// packed K.  A view's packed K and error word are its parent's (owner()).
struct SweepPath {
  bool ok = false;
  DevBuf<Job3> d_jobs;
  DevBuf<Region3> d_regions;
  int n_regions = 0, ks = 0, par_j = 0;
  std::vector<int32_t> slot;  // lattice cell -> transfer-kernel slot
  long slabs = 0, patch_slots = 0;
  DevBuf<float> d_k3;      // n_patches x Cfg3::K_FLOATS
  size_t k3_floats = 0;
  DevBuf<float> d_zero;    // 16 bytes of zeros
  DevBuf<uint32_t, hipHostFree> err;  // page-locked word the sweep kernel sets when a job waited for its predecessors beyond the bound
  uint32_t* d_err = nullptr;          // ... as the device sees it
  DevBuf<unsigned long long> d_stamps;  // development builds (-DRPSF3_STAMPS)
};

// The plan's stream and events: a base, so that they are destroyed after the plan's buffers (members go before bases)
struct PlanStream {
  hipStream_t stream = nullptr;
  bool borrowed_stream = false;  // a view runs on its parent's
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_busy = nullptr;    // end of the last apply (applies on different streams are serialised); recorded once the plan has seen a second stream
  // the second launch lane (rpsf_lanes.hpp; 256-pixel plans that are not views): its stream, the end of its work (recorded at a join) and the point
  // of the public stream it was last forked from
  hipStream_t lane1 = nullptr;
  hipEvent_t ev_lane = nullptr, ev_fork = nullptr;
  ~PlanStream() {
    if (ev_busy) (void)hipEventDestroy(ev_busy);
    if (ev_lane) (void)hipEventDestroy(ev_lane);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (lane1) (void)hipStreamDestroy(lane1);
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (stream && !borrowed_stream) (void)hipStreamDestroy(stream);
  }
};

struct rpsf_plan : PlanStream {
  int device = 0, N = 0, n_patches = 0;
  DevBuf<int32_t> d_coords;
  DevBuf<float> d_win;  // read by the patch kernels and the sweep kernel; uploaded with the first-generation tables (a view reads its parent's)
  std::unique_ptr<rpsf_host::HostPipe, PipeRelease> pipe;  // host-array entry points: staging slots, copy streams (rpsf_hostpipe.hpp)
  std::unique_ptr<SatDevice, SatDeviceRelease> sat_dev;  // rpsf_apply_device_saturated: device scratch of the saturation branch (csrc/saturation.hip), made at the first such call
  std::vector<SatScratch> sat;  // rpsf_apply_host_saturated: per staging slot, the 2N-padded float64 frame, its mask and the raw values (host scratch, kept between calls)
  // Views: a plan over a subset of another plan's patches that shares its tables, its packed K (desc.z = the patch's index in the
  // parent), its error word and its stream - the row bands a single large host frame is cut into so that its upload, its patches and
  // its download overlap (host_one_frame).  Owned by the parent, which destroys them before its own buffers; built for one frame shape.
  rpsf_plan* parent = nullptr;
  std::vector<int32_t> k_index;           // view: patch i of this plan is patch k_index[i] of the parent
  std::vector<std::unique_ptr<rpsf_plan>> bands;  // parent: its row-band views
  std::vector<int> band_rows;             // bands.size() + 1 output row boundaries
  std::vector<int> band_in_rows;          // per band: image rows [0, band_in_rows[b]) must be resident before it runs
  int bands_h = 0, bands_w = 0, bands_mode = -1, bands_want = -1;
  bool have_k = false;
  std::vector<int32_t> h_coords;
  // overlap-add strategy: on regular half-overlap lattices direct accumulation through the XCD's L2 (three-stage
  // plans) or colour planes + plane sum (the small-patch plans); float atomics for any other corner list
  int overlap_mode = 0;  // 0 auto, 1 atomics, 2 planes, 3 direct, 4 sweep
  int cu_count = 256;
  bool lattice = false;
  int host_bands_opt = -1, stream_group_opt = 0, stream_depth_opt = 0;  // rpsf_plan_set_option; -1 / 0: the library decides
  int sat_group_opt = 0;            // RPSF_OPT_SAT_GROUP: frames per frame-group of the batched device saturation route (0: by the scratch budget)
  int sat_batch_info[4] = {};       // rpsf_saturation_batch_info
  // rpsf_apply_view / rpsf_apply_batch_view: dense float32 staging of the sides that are not zero copy (4 B per pixel per frame of the call and side,
  // frames rounded up to 4 pixels; made at the first such call, grown on demand), and the end of the last call that used it
  DevBuf<float> d_view_in, d_view_out;
  size_t view_in_floats = 0, view_out_floats = 0;
  // rpsf_apply_frames_host_masked_device: the host masks of a frame-group as uploaded (1 B per pixel per frame, or one shared mask)
  DevBuf<uint8_t> d_host_masks;
  size_t host_mask_bytes = 0;
  hipEvent_t ev_view = nullptr;
  hipStream_t view_stream = nullptr;
  bool view_busy = false;
  int last_host_bands = 0;  // row bands the last single host frame was cut into (rpsf_plan_host_bands)
  hipStream_t last_stream = nullptr;
  bool busy_valid = false;
  bool multi_stream = false;  // the plan has been applied on more than one stream: applies record ev_busy (launch_apply)
  // the lattice (setup_lattice): read by the planes, the sweep kernel and host_one_frame
  int lat_r0 = 0, lat_c0 = 0, nti = 0, ntj = 0;
  DevBuf<uint8_t> d_cover;
  DevBuf<int4> d_desc;
  std::vector<int32_t> h_order;
  int corner_min[2] = {0, 0}, corner_max[2] = {0, 0};  // extreme patch corners (row, col)
  bool generic = false;
  FftPath fft;
  PatchPath patch;
  SweepPath sweep;

  ~rpsf_plan() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (lane1) (void)hipStreamSynchronize(lane1);
    if (ev_view) (void)hipEventDestroy(ev_view);
    bands.clear();
  }
};

// The plan whose tables, packed K and sweep error word a plan reads: a view borrows its parent's
static const rpsf_plan* owner(const rpsf_plan* p) { return p->parent ? p->parent : p; }

enum OverlapKind { OV_ATOMIC = 0, OV_PLANES = 1, OV_DIRECT = 2, OV_SWEEP = 3 };

template <class F>
static int dispatch_n(int N, F&& f) {
  switch (N) {
    case 256: return f.template operator()<Cfg256>();
    case 128: return f.template operator()<Cfg128>();
    case 64: return f.template operator()<Cfg64>();
    case 32: return f.template operator()<Cfg32>();
    case 16: return f.template operator()<Cfg16>();
    default: return fail(RPSF_E_UNSUPPORTED, "patch size " + std::to_string(N) + " has no compiled plan (16..256, powers of two)");
  }
}

// A compiled patch plan as the host sees it: the first generation (Gen2 = false: every N; N = 128, 256 only under the RPSF_V1 development
// switch) or the second (N = 128, 256)
template <class C, bool Gen2>
struct PatchPlan {
  using Cfg = C;
  using L = std::conditional_t<Gen2, Launch2<C>, Launch<C>>;
  static constexpr bool V2 = Gen2;
  static constexpr int WG = L::WG, TEAMS = WG / C::T;  // (Launch<C>::TEAMS; the second generation has one patch per workgroup)
  static constexpr size_t LDS_BYTES = L::LDS_BYTES;
  static constexpr size_t PACK_PER_PATCH = C::G_PER_PATCH + (Gen2 ? C::GS_PER_PATCH : 0);  // elements one thread each of the pack kernels writes
  static_assert(TEAMS == patch_teams(C::N), "lattice_build cuts the chunks by patch_teams()");
  // (functions, not members: only the generation's own templates are instantiated for C)
  static constexpr auto kernel() { if constexpr (Gen2) return &patch_kernel2<C>; else return &patch_kernel<C>; }
  static constexpr auto pack() { if constexpr (Gen2) return &pack_kernel2<C>; else return &pack_kernel<C>; }
  static constexpr auto pack_spectra() { if constexpr (Gen2) return &pack_spectra_kernel2<C>; else return &pack_spectra_kernel<C>; }
};

static void host_tables(int N, std::vector<cf>& tw, std::vector<float>& win) {
  tw.resize(N);
  win.resize(N);
  for (int k = 0; k < N; ++k) {
    double a = -2.0 * M_PI * k / N;
    tw[k] = cf{(float)std::cos(a), (float)std::sin(a)};
    win[k] = (float)std::sin((k + 0.5) * (M_PI / N));  // transform.py:151-154
  }
}

// Slot table, twiddles and (d_win) window of a compiled plan; d_pairtab: the bin pairs of the special slots (first generation, two-stage plans) or
// of the self-paired groups (second)
template <class T>
static int upload_tables(int device, DevBuf<uint16_t>& d_tab, DevBuf<cf>& d_tw, DevBuf<float>* d_win = nullptr, DevBuf<uint32_t>* d_pairtab = nullptr) {
  using C = typename T::Cfg;
  std::vector<uint16_t> tab((size_t)C::T * C::NSLOT * 2);
  std::vector<uint32_t> pt;
  if constexpr (T::V2) {
    build_slot_table2<C>(tab.data());
    pt.resize((size_t)C::ORBIT_ROUNDS * 64);
    if (special_slots2<C>() > 64 || build_orbit_table2<C>(tab.data(), pt.data()) != C::NORBIT)
      return fail(RPSF_E_STATE, "slot / orbit table inconsistent (internal)");
  } else {
    build_slot_table<C>(tab.data());
    pt.resize((size_t)C::PT_WORDS + 1);
    if (d_pairtab && build_pair_table<C>(tab.data(), pt.data()) > C::NP) return fail(RPSF_E_STATE, "pair table overflow (internal)");
  }
  std::vector<cf> tw;
  std::vector<float> win;
  host_tables(C::N, tw, win);
  HIP_TRY(hipSetDevice(device));
  if (d_pairtab) HIP_TRY(d_pairtab->upload(pt.data(), pt.size()));
  HIP_TRY(d_tab.upload(tab.data(), tab.size()));
  HIP_TRY(d_tw.upload(tw.data(), tw.size()));
  if (d_win) HIP_TRY(d_win->upload(win.data(), win.size()));
  return RPSF_OK;
}

// A batch of frames that share the plan's transfer kernel: frame f at image + f*im_stride, out + f*out_stride (floats)
struct Batch {
  int frames = 1;
  size_t im_stride = 0, out_stride = 0;
};

// ------------------------------------------------------------------------------------------------
// what crosses the units (comments and contracts: at the definitions)
// ------------------------------------------------------------------------------------------------
// rpsf.hip
RPSF_HIDDEN OverlapKind rpsf_detail_overlap_kind(const rpsf_plan* p);
RPSF_HIDDEN int rpsf_detail_check_geometry(const rpsf_plan* p, const rpsf_geometry* g);
RPSF_HIDDEN bool rpsf_detail_lattice_covers_window(const rpsf_plan* p, const rpsf_geometry& g);
RPSF_HIDDEN int rpsf_detail_launch_apply(rpsf_plan* p, const float* d_img, float* d_out, const rpsf_geometry& g, hipStream_t st,
                                         hipEvent_t ev_k0, hipEvent_t ev_k1 = nullptr, Batch b = Batch(), bool may_pipeline = false);
RPSF_HIDDEN int rpsf_detail_join_lanes(rpsf_plan* p);
RPSF_HIDDEN void rpsf_detail_clear_error(rpsf_plan* p);
RPSF_HIDDEN int rpsf_detail_launch_batch(rpsf_plan* p, const float* d_imgs, float* d_outs, int n_frames, size_t im_stride, size_t out_stride,
                                         const rpsf_geometry& g, hipStream_t st, hipEvent_t ev_k0 = nullptr, hipEvent_t ev_k1 = nullptr);
RPSF_HIDDEN int rpsf_detail_plan_create_impl(rpsf_plan** out, int device, int patch_size, int n_patches, const int32_t* coords_rc, rpsf_plan* parent,
                                             const int32_t* k_index);
RPSF_HIDDEN void rpsf_detail_drop_bands(rpsf_plan* p);
RPSF_HIDDEN int rpsf_detail_sweep_check(rpsf_plan* p);
RPSF_HIDDEN int rpsf_detail_drain_after_error(rpsf_plan* p, hipError_t err, const char* where);
// rpsf_host.hip
RPSF_HIDDEN int rpsf_detail_pipe_ensure(rpsf_plan* p, size_t slot_floats, int depth);
RPSF_HIDDEN int rpsf_detail_host_parts_for(size_t bytes);
