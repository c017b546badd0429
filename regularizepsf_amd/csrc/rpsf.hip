// rpsf.hip - host side of librpsf_hip.so: plans, launches and the C ABI of include/rpsf.h; the RCCL and
// hipFFT loaders.  The device code is in rpsf_kernels.hpp (kernels) and rpsf_core.hpp (per-thread phases).  What follows from a corner
// list and a frame geometry alone - lattice tables, processing order, row bands, the geometry predicates of the launch forms - is plain
// C++ in rpsf_lattice.hpp (as the job lists of the sweep kernel are in rpsf_plan3.hpp): this file uploads what those return.
//
// Kernels (rpsf_kernels.hpp):
//   patch_kernel<C>        K1: fused gather+pad+window -> 2-D DFT -> x folded K -> inverse DFT -> window ->
//                          overlap-add; one workgroup per patch (or several small patches per workgroup),
//                          patch resident in registers, LDS used only for the inter-stage transposes.
//                          Stands in for regularizepsf/transform.py:151-169.
//   pack_kernel<C>         folds K to K_h = (K(k)+conj K(-k))/2 and re-orders it into the per-thread
//                          streaming layout of K1 (one-time, at set_transfer).
//   build_transfer_kernel  K2: transform.py:78-82 element-wise.
//   psf_fft_kernel<C>      K3: psf.py:216-219, forward half of K1 written out as a full spectrum.
//   add_rows_kernel        K4: seam accumulate for the multi-GPU row-band split.
//   sum_planes_kernel      K5: output = sum of the four colour planes the patches of one parity class write.
//   generic_*_kernel       gather / multiply / scatter around hipFFT for patch sizes without a plan.
// Development-only build switches (never set by regularizepsf_amd/build.py): RPSF_STAMPS / RPSF_WAVE_STAMPS (per-phase
// timestamps, scripts/stamps.py) and the RPSF2_ABL_* timing ablations of rpsf_kernels2.hpp (results are wrong, timing only).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#define RPSF_HOST_TU 1
#include "rpsf_device.hpp"
#include "rpsf_hostpipe.hpp"
#include "rpsf_lattice.hpp"
#include "rpsf_saturation.hpp"
#include "rpsf_core_saturation_batch.hpp"
#include "rpsf_convert.hpp"
#include "rpsf_core_convert.hpp"

RPSF_PLANS_V1(RPSF_DECL_V1)
RPSF_PLANS_V2(RPSF_DECL_V2)
RPSF_PLANS_V3(RPSF_DECL_V3)

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return fail(e_ == hipErrorOutOfMemory ? RPSF_E_NOMEM : RPSF_E_HIP,                                \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                                   \
  } while (0)

// the same for the translation units that implement entry points of their own (csrc/builder.hip)
__attribute__((visibility("hidden"))) int rpsf_detail_fail(int code, const std::string& msg) { return fail(code, msg); }

extern "C" const char* rpsf_last_error(void) { return g_err.c_str(); }

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

template <class F>
static int dispatch_v3(int N, F&& f) {
  switch (N) {
    case 64: return f.template operator()<Cfg3_64>();
    case 32: return f.template operator()<Cfg3_32>();
    case 16: return f.template operator()<Cfg3_16>();
    default: return fail(RPSF_E_UNSUPPORTED, "no third-generation plan for this patch size");
  }
}
static bool has_v3(int N) { return sweep_patch_size(N); }

// Python's slice arithmetic for [start, stop) over a length-n axis (a negative bound wraps once): the window rule of the saturation fill
static void py_slice(long start, long stop, long n, long* lo, long* hi) {
  if (start < 0) start = std::max(start + n, 0L);
  if (stop < 0) stop = std::max(stop + n, 0L);
  *lo = std::min(start, n);
  *hi = std::min(stop, n);
}

// One device allocation of T[count], owned by the handle (move-only) and freed with it.  Free = hipHostFree: page-locked host memory.
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
  DevBuf<uint32_t> d_tile_done;   // per tile: contributors done, never reset (epoch * contributors after every apply)
  DevBuf<uint32_t> d_sum_order;   // all tiles, the ones whose contributors run first first
  uint32_t done_epoch = 0;
  size_t done_frames = 1;            // frames the tile counters are sized for (batches: one set per frame)
  int done_last_frames = 1;          // frames of the last fused launch (the counters restart when the number changes)
  DevBuf<uint32_t> d_sum_queue;   // position in d_sum_order, never reset
  uint32_t sum_queue_base = 0;
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
  DevBuf<uint32_t> d_xq;          // 8 counters, one per 128-byte line
  uint32_t xq_base[8] = {0, 0, 0, 0, 0, 0, 0, 0};
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
  ~PlanStream() {
    if (ev_busy) (void)hipEventDestroy(ev_busy);
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
    if (ev_view) (void)hipEventDestroy(ev_view);
    bands.clear();
  }
};

// The plan whose tables, packed K and sweep error word a plan reads: a view borrows its parent's
static const rpsf_plan* owner(const rpsf_plan* p) { return p->parent ? p->parent : p; }

enum OverlapKind { OV_ATOMIC = 0, OV_PLANES = 1, OV_DIRECT = 2, OV_SWEEP = 3 };
static OverlapKind overlap_kind(const rpsf_plan* p);

// Regions and job lists of the sweep kernel for `target_regions` workgroups (rpsf_plan3.hpp); replaces the plan's previous lists
static int build_sweep_lists(rpsf_plan* p, int target_regions) {
  const int nli = p->nti - 1, nlj = p->ntj - 1;
  Plan3 plan;
  const bool built = dispatch_v3(p->N, [&]<class C>() -> int {
    return plan3_build(C::N, C::KSMAX, C::WAVES, nli, nlj, p->sweep.slot.data(), p->sweep.par_j, target_regions, plan) ? RPSF_OK : RPSF_E_STATE;
  }) == RPSF_OK;
  if (!built) return RPSF_OK;  // (the plan keeps its other paths)
  SweepPath& sw = p->sweep;
  sw.ok = false;
  HIP_TRY(sw.d_jobs.upload(plan.jobs.data(), plan.jobs.size()));
  HIP_TRY(sw.d_regions.upload(plan.regions.data(), plan.regions.size()));
  if (!sw.d_zero) {
    HIP_TRY(sw.d_zero.alloc(16));
    HIP_TRY(hipMemset(sw.d_zero, 0, 64));
  }
  if (!p->parent && !sw.err) {  // (a view's kernel reports through its parent's word)
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&sw.err.p), 64, hipHostMallocMapped));
    std::memset(sw.err, 0, 64);
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&sw.d_err), sw.err, 0));
  }
  p->sweep.n_regions = (int)plan.regions.size(), p->sweep.ks = plan.ks, p->sweep.slabs = plan.slabs, p->sweep.patch_slots = plan.patch_slots;
  p->sweep.ok = true;
#if defined(RPSF3_STAMPS) || defined(RPSF3_DUMP)
  HIP_TRY(p->sweep.d_stamps.alloc((size_t)std::max(512, p->sweep.n_regions) * 8 * 8 * 16));
  HIP_TRY(hipMemset(p->sweep.d_stamps, 0, (size_t)std::max(512, p->sweep.n_regions) * 8 * 8 * 16 * sizeof(unsigned long long)));
#endif
  return RPSF_OK;
}

// Regular lattice test + colour classes + tile tables + processing order (rpsf_lattice.hpp), uploaded at plan creation
static int setup_lattice(rpsf_plan* p) {
  LatticeKnobs knobs;  // development sweeps
  if (const char* e = dev_env("RPSF_STRIPS")) knobs.strips = std::max(1, std::atoi(e));
  if (const char* e = dev_env("RPSF_ORDER_MEET")) knobs.meet = std::atoi(e) != 0;
  if (dev_env("RPSF_NO_RIM_FIRST")) knobs.rim_first = false;
  if (const char* e = dev_env("RPSF_RIM_LAST")) knobs.rim_last = std::atoi(e) != 0;
  const LatticeParent parent = p->parent ? LatticeParent{p->parent->lat_r0, p->parent->lat_c0, p->parent->lattice} : LatticeParent{};
  LatticeTables t = lattice_build(p->N, p->n_patches, p->h_coords.data(), p->k_index.empty() ? nullptr : p->k_index.data(), p->patch.v2,
                                  p->parent ? &parent : nullptr, knobs);
  const size_t n = (size_t)p->n_patches;
  p->lattice = t.lattice, p->patch.direct_ok = t.direct_ok;
  p->h_order = std::move(t.order);
  static_assert(sizeof(PatchDesc) == sizeof(int4) && sizeof(QuadWords) == sizeof(uint4), "uploaded as they are");
  HIP_TRY(p->d_desc.upload(reinterpret_cast<const int4*>(t.desc.data()), n));
  if (!t.lattice) return RPSF_OK;
  p->lat_r0 = t.r0, p->lat_c0 = t.c0, p->nti = t.nti, p->ntj = t.ntj;
  // ---- third generation: regions and job lists (rpsf_plan3.hpp) when every lattice cell has its patch ----
  if (!t.sweep_slot.empty()) {
    p->sweep.slot = std::move(t.sweep_slot);
    p->sweep.par_j = t.par_j;
    const int rc3 = build_sweep_lists(p, std::max(8, p->cu_count));
    if (rc3 != RPSF_OK) return rc3;
  }
  HIP_TRY(p->d_cover.upload(t.cover.data(), t.cover.size()));
  if (p->patch.v2) {  // fused plane sum: tile order and counters
    HIP_TRY(p->patch.d_sum_order.upload(t.sum_order.data(), t.sum_order.size()));
    HIP_TRY(p->patch.d_tile_done.alloc(t.sum_order.size()));
    HIP_TRY(hipMemset(p->patch.d_tile_done, 0, t.sum_order.size() * sizeof(uint32_t)));
    HIP_TRY(p->patch.d_sum_queue.alloc(1));
    HIP_TRY(hipMemset(p->patch.d_sum_queue, 0, sizeof(uint32_t)));
    HIP_TRY(p->patch.d_xq.alloc(8 * 32));
    HIP_TRY(hipMemset(p->patch.d_xq, 0, 8 * 32 * sizeof(uint32_t)));
    std::copy_n(t.prefetch_first, 9, p->patch.prefetch_first);
    HIP_TRY(p->patch.d_prefetch_tiles.alloc(std::max<size_t>(1, t.prefetch_tiles.size())));
    HIP_TRY(hipMemcpy(p->patch.d_prefetch_tiles, t.prefetch_tiles.data(), t.prefetch_tiles.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  if (p->patch.direct_ok) {
    HIP_TRY(p->patch.d_quads.upload(reinterpret_cast<const uint4*>(t.quads.data()), n));
    HIP_TRY(p->patch.d_tile_info.upload(t.tile_info.data(), t.tile_info.size()));
    HIP_TRY(p->patch.d_chunk_xcc.alloc(8));
    HIP_TRY(hipMemset(p->patch.d_chunk_xcc, 0, 8 * sizeof(uint32_t)));
  }
  return RPSF_OK;
}

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

// The patch plan a rpsf_plan runs (v2 = PatchPath::v2); dispatch_n: the first-generation configurations alone (psf_fft_impl runs their forward half for every N)
template <class F>
static int dispatch_patch(bool v2, int N, F&& f) {
  if (!v2) return dispatch_n(N, [&]<class C>() -> int { return f.template operator()<PatchPlan<C, false>>(); });
  switch (N) {
    case 256: return f.template operator()<PatchPlan<Cfg256v2, true>>();
    case 128: return f.template operator()<PatchPlan<Cfg128v2, true>>();
    default: return fail(RPSF_E_UNSUPPORTED, "no second-generation plan for this patch size");
  }
}
static bool has_v2(int N) { return (N == 256 || N == 128) && !dev_env("RPSF_V1"); }

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

extern "C" int rpsf_device_count(int* count) {
  if (!count) return fail(RPSF_E_BADARG, "count is null");
  HIP_TRY(hipGetDeviceCount(count));
  return RPSF_OK;
}

extern "C" int rpsf_device_info(int device, int* compute_units, char* name, size_t name_len) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (compute_units) *compute_units = prop.multiProcessorCount;
  if (name && name_len) {
    std::snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
  }
  return RPSF_OK;
}


// ------------------------------------------------------------------------------------------------
// Colour classes for the fallback's overlap-add (any N, odd ones too): calculate_covering (regularizepsf/util.py:10-53) lays four sub-grids of
// pitch N - corner rows k N and k N - ceil(N / 2), the same for columns - so the corner rows of a covering take at most two residues modulo
// N, and so do the columns.  Colour = (row residue class, column residue class): two distinct patches of one colour differ by a multiple of N
// in a coordinate, i.e. they do not overlap.  False (atomic adds) for corner lists without that structure or with a corner listed twice.
static bool generic_colours(int N, const int32_t* coords_rc, int n, std::vector<uint8_t>& colours) {
  int res[2][2], nres[2] = {0, 0};
  colours.assign((size_t)n, 0);
  std::vector<std::pair<int32_t, int32_t>> seen((size_t)n);
  for (int i = 0; i < n; ++i) {
    seen[(size_t)i] = {coords_rc[2 * i], coords_rc[2 * i + 1]};
    for (int axis = 0; axis < 2; ++axis) {
      const int r = ((coords_rc[2 * i + axis] % N) + N) % N;
      int cls = -1;
      for (int k = 0; k < nres[axis]; ++k)
        if (res[axis][k] == r) cls = k;
      if (cls < 0) {
        if (nres[axis] == 2) return false;
        cls = nres[axis], res[axis][nres[axis]++] = r;
      }
      colours[(size_t)i] |= (uint8_t)(cls << (1 - axis));
    }
  }
  std::sort(seen.begin(), seen.end());
  return std::adjacent_find(seen.begin(), seen.end()) == seen.end();
}

// Any other patch size: fallback through hipFFT (loaded with dlopen, like RCCL).
// The reference accepts every square patch size (odd ones included, transform.py:151-164); the
// hand-written plans cover 16..256.  For the rest: gather+pad+window into a complex batch, batched
// 2-D C2C forward, times the caller's full K (no folding: Re(ifft2(.)) is taken literally), C2C
// inverse, window again, float atomic overlap-add.  Correctness path, not a tuned one.
// ------------------------------------------------------------------------------------------------
struct HipfftApi {
  void* lib = nullptr;
  int (*plan_many)(void**, int, int*, int*, int, int, int*, int, int, int, int) = nullptr;
  int (*set_stream)(void*, hipStream_t) = nullptr;
  int (*exec_c2c)(void*, void*, void*, int) = nullptr;
  int (*destroy)(void*) = nullptr;
  std::string error;
  std::mutex guard;  // plans may be created from several threads
  bool load() {
    std::lock_guard<std::mutex> lock(guard);
    if (lib) return true;
    if (!error.empty()) return false;
    for (const char* n : {"libhipfft.so", "libhipfft.so.0", "/opt/rocm/lib/libhipfft.so"}) {
      lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
      if (lib) break;
    }
    if (!lib) {
      error = "patch sizes other than 16, 32, 64, 128, 256 need libhipfft.so, which could not be loaded";
      return false;
    }
    plan_many = reinterpret_cast<decltype(plan_many)>(dlsym(lib, "hipfftPlanMany"));
    set_stream = reinterpret_cast<decltype(set_stream)>(dlsym(lib, "hipfftSetStream"));
    exec_c2c = reinterpret_cast<decltype(exec_c2c)>(dlsym(lib, "hipfftExecC2C"));
    destroy = reinterpret_cast<decltype(destroy)>(dlsym(lib, "hipfftDestroy"));
    if (!plan_many || !set_stream || !exec_c2c || !destroy) {
      error = "libhipfft.so lacks hipfftPlanMany / hipfftSetStream / hipfftExecC2C / hipfftDestroy";
      lib = nullptr;
      return false;
    }
    return true;
  }
};
static HipfftApi g_hipfft;
void FftPlanRelease::operator()(void* h) const {
  if (g_hipfft.destroy) (void)g_hipfft.destroy(h);
}

static void set_corner_extremes(rpsf_plan* p) {
  for (int d = 0; d < 2; ++d) p->corner_min[d] = p->corner_max[d] = p->h_coords[d];
  for (int i = 1; i < p->n_patches; ++i)
    for (int d = 0; d < 2; ++d) {
      p->corner_min[d] = std::min(p->corner_min[d], p->h_coords[2 * i + d]);
      p->corner_max[d] = std::max(p->corner_max[d], p->h_coords[2 * i + d]);
    }
}

// parent / k_index: a view of `parent` (shares its tables, packed K and stream; k_index[i] = the parent's index of patch i)
static int plan_create_impl(rpsf_plan** out, int device, int patch_size, int n_patches, const int32_t* coords_rc, rpsf_plan* parent,
                            const int32_t* k_index) {
  if (!out || !coords_rc) return fail(RPSF_E_BADARG, "null argument");
  if (n_patches <= 0) return fail(RPSF_E_BADARG, "n_patches must be positive");
  const int N = patch_size;
  const bool compiled = dispatch_n(N, []<class C>() { return RPSF_OK; }) == RPSF_OK;
  if (!compiled) {
    if (N < 2 || N > 4096) return fail(RPSF_E_UNSUPPORTED, "patch size " + std::to_string(N) + " is outside 2..4096");
    if (!g_hipfft.load()) return fail(RPSF_E_UNSUPPORTED, g_hipfft.error);
  }
  auto* p = new rpsf_plan;
  p->device = device, p->N = N, p->n_patches = n_patches;
  p->generic = !compiled;
  p->parent = parent;
  if (parent) p->k_index.assign(k_index, k_index + n_patches);
  auto body = [&]() -> int {
    HIP_TRY(hipSetDevice(device));
    if (parent) {
      if (p->generic) return fail(RPSF_E_UNSUPPORTED, "views need a compiled plan");
      p->stream = parent->stream, p->borrowed_stream = true;
    } else {
      HIP_TRY(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    }
    for (auto& e : p->ev) HIP_TRY(hipEventCreate(&e));
    if (p->generic) {
      HIP_TRY(p->d_coords.upload(coords_rc, 2 * (size_t)n_patches));
      p->h_coords.assign(coords_rc, coords_rc + 2 * (size_t)n_patches);
      set_corner_extremes(p);
      std::vector<float> win(N);
      for (int i = 0; i < N; ++i) win[i] = (float)std::sin((i + 0.5) * M_PI / N);  // transform.py:151-155
      HIP_TRY(p->fft.d_win.upload(win.data(), N));
      {
        std::vector<uint8_t> colours;
        if (generic_colours(N, p->h_coords.data(), n_patches, colours)) {
          HIP_TRY(p->fft.d_colour.upload(colours.data(), colours.size()));
          p->lattice = true;  // (what rpsf_plan_set_overlap_mode(2) and the automatic mode ask for)
        }
      }
      const size_t per = (size_t)N * N;
      HIP_TRY(p->fft.d_kfull.alloc(per * n_patches));
      p->fft.chunk = (int)std::min<size_t>((size_t)n_patches, std::max<size_t>(1, ((size_t)256 << 20) / (per * sizeof(cf))));
      HIP_TRY(p->fft.d_buf.alloc(per * p->fft.chunk));
      int dims[2] = {N, N};
      void* fft_plan = nullptr;
      const int made = g_hipfft.plan_many(&fft_plan, 2, dims, nullptr, 1, (int)per, nullptr, 1, (int)per, /*HIPFFT_C2C*/ 0x29, p->fft.chunk);
      p->fft.plan.reset(fft_plan);
      if (made != 0) return fail(RPSF_E_HIP, "hipfftPlanMany failed");
      if (g_hipfft.set_stream(p->fft.plan.get(), p->stream) != 0) return fail(RPSF_E_HIP, "hipfftSetStream failed");
      return RPSF_OK;
    }
    {
      hipDeviceProp_t prop;
      HIP_TRY(hipGetDeviceProperties(&prop, device));
      p->cu_count = prop.multiProcessorCount;
    }
    HIP_TRY(p->d_coords.upload(coords_rc, 2 * (size_t)n_patches));
    p->h_coords.assign(coords_rc, coords_rc + 2 * (size_t)n_patches);
    set_corner_extremes(p);
    HIP_TRY(p->patch.d_sink.alloc(128));
#if defined(RPSF_STAMPS)
#if defined(RPSF_WAVE_STAMPS)
    constexpr size_t STAMP_WAVES = 8;
#else
    constexpr size_t STAMP_WAVES = 1;
#endif
    HIP_TRY(p->patch.d_stamps.alloc(16 * STAMP_WAVES * (size_t)n_patches));
    HIP_TRY(hipMemset(p->patch.d_stamps, 0, sizeof(unsigned long long) * 16 * STAMP_WAVES * (size_t)n_patches));
#endif
    p->patch.v2 = has_v2(N);
    // (measured, profiles/r02u, r02v: 32 of them are worth -1 % at 4096^2 and -2.5 % at 8192^2; 48 cost more patch time than they hide)
    p->patch.sum_first = -1;  // decided per launch (sum_first_for) unless the environment pins it
    if (const char* e = dev_env("RPSF_SUM_FIRST")) p->patch.sum_first = std::max(0, std::atoi(e)) / 8 * 8;
    if (const char* e = dev_env("RPSF_HEAD_PATCHES")) p->patch.head_patches = std::atoi(e) > 0 ? 1 : 0;
    if (const char* e = dev_env("RPSF_PREFETCH")) p->patch.prefetch = std::atoi(e) != 0;
    if (const char* e = dev_env("RPSF_STAGGER_US")) p->patch.stagger_us = std::max(0, std::atoi(e));  // development sweeps
    if (const char* e = dev_env("RPSF_RESERVED_CUS")) p->patch.reserved_cus = std::min(128, std::max(0, std::atoi(e)));
    // (until the plane stores were kept in the Infinity Cache the fused sum cost the 128-pixel plan 3 %; now it gains 3 ... 6 %)
    p->patch.fuse_pays = N >= 128 || dev_env("RPSF_FUSE_ALWAYS") != nullptr;
    // (256-pixel plan: profiles/r02ag, -3.7 % per apply at 4096^2 from the re-entry alone; 128-pixel plan, whose four workgroups per CU
    // hide one another's dispatch: 8 x 2048^2 0.334 vs 0.343 ms, single frames unchanged)
    p->patch.persist = N == 256 || N == 128;  // (rpsf_plan_set_option RPSF_OPT_PERSIST)
    if (p->patch.persist) {
      if (N == 256)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&patch_kernel2_256p), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)Launch2<Cfg256v2>::LDS_BYTES));
      else {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&patch_kernel2_128p), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)Launch2<Cfg128v2>::LDS_BYTES));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&patch_kernel2_128pc), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)Launch2<Cfg128v2>::LDS_BYTES));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&patch_kernel2_128pcs), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)Launch2<Cfg128v2>::LDS_BYTES));
        // Plain instead of streaming loads of the pair words where the plan's K (66,560 B per patch) fits the 256 MiB Infinity Cache beside the
        // planes: measured (profiles/r04av) -6 % per apply at 72 MB of K, +6.6 % at 160 MB; RPSF_K_CACHED=0/1 overrides (tests run both forms).
        p->patch.k_cached = (size_t)(parent ? parent->n_patches : n_patches) * Cfg128v2::G_PER_PATCH * sizeof(cf) <= ((size_t)96 << 20);
      }
    }
    int rl = dispatch_patch(p->patch.v2, N, [&]<class T>() -> int {
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(T::kernel()), hipFuncAttributeMaxDynamicSharedMemorySize, (int)T::LDS_BYTES));
      int per_cu = 0;
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, T::kernel(), T::WG, T::LDS_BYTES));
      p->patch.round_capacity = p->cu_count * std::max(1, per_cu) * T::TEAMS;
      return RPSF_OK;
    });
    if (rl != RPSF_OK) return rl;
    HIP_TRY(hipEventCreateWithFlags(&p->ev_busy, hipEventDisableTiming));
    rl = setup_lattice(p);
    if (rl != RPSF_OK) return rl;
    if (p->sweep.ok) {
      rl = dispatch_v3(N, [&]<class C>() -> int {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&sweep_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&sweep_kernel_kc<C>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)C::LDS_BYTES));
        if (!parent) {
          p->sweep.k3_floats = (size_t)C::K_FLOATS * n_patches;
          HIP_TRY(p->sweep.d_k3.alloc(p->sweep.k3_floats));
        }
        return RPSF_OK;
      });
      if (rl != RPSF_OK) return rl;
      if (parent && !parent->sweep.d_k3) p->sweep.ok = false;  // (the parent's lattice was not complete: it has no third-generation K)
    }
    if (parent) {  // tables, packed K and error word are the parent's (owner())
      p->have_k = parent->have_k;
      p->overlap_mode = parent->overlap_mode, p->patch.stagger_us = parent->patch.stagger_us, p->patch.k_prefetch = parent->patch.k_prefetch;
      return RPSF_OK;
    }
    return dispatch_patch(p->patch.v2, N, [&]<class T>() -> int {
      int r2 = upload_tables<T>(device, p->patch.d_tab, p->patch.d_tw, &p->d_win, &p->patch.d_pairtab);
      if (r2 != RPSF_OK) return r2;
      p->patch.g_elems = (size_t)T::Cfg::G_PER_PATCH * n_patches;
      p->patch.gs_elems = (size_t)T::Cfg::GS_PER_PATCH * n_patches;
      HIP_TRY(p->patch.d_g.alloc(p->patch.g_elems));
      HIP_TRY(p->patch.d_gs.alloc(p->patch.gs_elems + 1));
      return RPSF_OK;
    });
  };
  const int rc = body();
  if (rc != RPSF_OK) {
    std::string keep = g_err;
    delete p;
    g_err = keep;
    return rc;
  }
  *out = p;
  return RPSF_OK;
}

extern "C" int rpsf_plan_create(rpsf_plan** out, int device, int patch_size, int n_patches, const int32_t* coords_rc) {
  return plan_create_impl(out, device, patch_size, n_patches, coords_rc, nullptr, nullptr);
}

extern "C" void* rpsf_plan_stream(rpsf_plan* p) { return p ? (void*)p->stream : nullptr; }

extern "C" void rpsf_plan_destroy(rpsf_plan* p) { delete p; }

static void drop_bands(rpsf_plan* p) {
  p->bands.clear(), p->band_rows.clear(), p->band_in_rows.clear();
  p->bands_h = p->bands_w = 0, p->bands_mode = -1, p->bands_want = -1;
}

// Where install_transfer reads K from: the caller's full K, or the spectra it is built from (transform.py:78-82 evaluated where the packer
// reads K)
struct KSource {
  const cf* k = nullptr;  // (n, N, N) complex64, unfolded: on the device (the packers read nothing else), or on the host for the fallback's copy
  hipMemcpyKind k_kind = hipMemcpyDeviceToDevice;
  const cf *s = nullptr, *t = nullptr;
  double alpha = 0.0, epsilon = 0.0;
};

// K of patches [first, first + count) - `src` holds these patches only, from its start - into every representation the plan holds: the
// fallback's unfolded copy, or the patch kernels' (first generation, or second) and the sweep kernel's beside them.  The plan and its views
// have K once its last patch is in.
static int install_transfer(rpsf_plan* p, const KSource& src, int first, int count) {
  if (p->parent) return fail(RPSF_E_STATE, "a view shares its parent's transfer kernel");
  const size_t at = (size_t)first * p->N * p->N;
  const cf *k = src.k, *s = src.s, *t = src.t;
  const float alpha = (float)src.alpha, epsilon = (float)src.epsilon;
  auto grid = [](size_t total) { return dim3((unsigned)((total + 255) / 256)); };
  int rc = RPSF_OK;
  if (p->generic) {  // the fallback multiplies by the caller's unfolded K
    const size_t elems = (size_t)p->N * p->N * count;
    if (k) HIP_TRY(hipMemcpy(p->fft.d_kfull + at, k, elems * sizeof(cf), src.k_kind));
    else rc = rpsf_build_transfer_device(p->device, elems, s, t, 0, src.alpha, src.epsilon, p->fft.d_kfull + at, p->stream);
  } else {
    if (p->sweep.d_k3)
      rc = dispatch_v3(p->N, [&]<class C>() -> int {
        cf* k3 = reinterpret_cast<cf*>(p->sweep.d_k3 + (size_t)first * C::K_FLOATS);
        const dim3 g = grid((size_t)(C::K_FLOATS / 2) * count);
        if (k) pack_kernel3<C><<<g, dim3(256), 0, p->stream>>>(k, count, k3);
        else pack_spectra_kernel3<C><<<g, dim3(256), 0, p->stream>>>(s, t, alpha, epsilon, count, k3);
        HIP_TRY(hipGetLastError());
        return RPSF_OK;
      });
    if (rc == RPSF_OK)
      rc = dispatch_patch(p->patch.v2, p->N, [&]<class T>() -> int {
        using C = typename T::Cfg;
        cf *g = p->patch.d_g + (size_t)first * C::G_PER_PATCH, *gs = p->patch.d_gs + (size_t)first * C::GS_PER_PATCH;
        const dim3 gr = grid(T::PACK_PER_PATCH * count);
        if (k) T::pack()<<<gr, dim3(256), 0, p->stream>>>(k, count, p->patch.d_tab, p->patch.d_pairtab, g, gs);
        else T::pack_spectra()<<<gr, dim3(256), 0, p->stream>>>(s, t, alpha, epsilon, count, p->patch.d_tab, p->patch.d_pairtab, g, gs);
        HIP_TRY(hipGetLastError());
        return RPSF_OK;
      });
  }
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipStreamSynchronize(p->stream));
  if (first + count == p->n_patches) {
    p->have_k = true;
    for (auto& band : p->bands) band->have_k = true;
  }
  return RPSF_OK;
}

extern "C" int rpsf_plan_set_transfer(rpsf_plan* p, const float* k_host) {
  if (!p || !k_host) return fail(RPSF_E_BADARG, "null argument");
  HIP_TRY(hipSetDevice(p->device));
  const cf* k = reinterpret_cast<const cf*>(k_host);
  if (p->generic) return install_transfer(p, KSource{k, hipMemcpyHostToDevice}, 0, p->n_patches);
  // the packers read K from the device: it goes up 64 MiB at a time
  const size_t per = (size_t)p->N * p->N;
  const int chunk = std::min(p->n_patches, (int)std::max<size_t>(1, (size_t)(64u << 20) / (per * sizeof(cf))));
  DevBuf<cf> d_tmp;
  HIP_TRY(d_tmp.alloc(per * chunk));
  for (int first = 0; first < p->n_patches; first += chunk) {
    const int cnt = std::min(chunk, p->n_patches - first);
    HIP_TRY(hipMemcpyAsync(d_tmp, k + (size_t)first * per, per * sizeof(cf) * cnt, hipMemcpyHostToDevice, p->stream));
    const int rc = install_transfer(p, KSource{d_tmp}, first, cnt);
    if (rc != RPSF_OK) return rc;
  }
  return RPSF_OK;
}

extern "C" int rpsf_plan_set_transfer_device(rpsf_plan* p, const void* k_dev) {
  if (!p || !k_dev) return fail(RPSF_E_BADARG, "null argument");
  HIP_TRY(hipSetDevice(p->device));
  return install_transfer(p, KSource{reinterpret_cast<const cf*>(k_dev)}, 0, p->n_patches);
}

// construct -> pack in one pass: complex64 spectra of the plan's patches on its device
extern "C" int rpsf_plan_set_transfer_spectra_device(rpsf_plan* p, const void* s_c64_dev, const void* t_c64_dev, double alpha, double epsilon) {
  if (!p || !s_c64_dev || !t_c64_dev) return fail(RPSF_E_BADARG, "null argument");
  HIP_TRY(hipSetDevice(p->device));
  return install_transfer(p, KSource{nullptr, hipMemcpyDeviceToDevice, reinterpret_cast<const cf*>(s_c64_dev), reinterpret_cast<const cf*>(t_c64_dev),
                                     alpha, epsilon}, 0, p->n_patches);
}

extern "C" int rpsf_plan_transfer_bytes(const rpsf_plan* p, size_t* bytes) {
  if (!p || !bytes) return fail(RPSF_E_BADARG, "null argument");
  // (the representation the plan's applies read: the third generation's when the sweep kernel runs them)
  if (p->generic) *bytes = (size_t)p->N * p->N * p->n_patches * sizeof(cf);
  else if (p->sweep.ok && overlap_kind(p) == OV_SWEEP) *bytes = p->sweep.k3_floats * sizeof(float);
  else *bytes = (p->patch.g_elems + p->patch.gs_elems) * sizeof(cf);
  return RPSF_OK;
}

static int check_geometry(const rpsf_plan* p, const rpsf_geometry* g) {
  if (!g) return fail(RPSF_E_BADARG, "geometry is null");
  if (g->height <= 0 || g->width <= 0) return fail(RPSF_E_BADARG, "image shape must be positive");
  if (g->pad_mode < 0 || g->pad_mode > RPSF_PAD_WRAP) return fail(RPSF_E_BADARG, "unknown pad mode");
  if (g->ld_image < g->width || g->ld_out < g->width) return fail(RPSF_E_BADARG, "row stride smaller than the image width");
  if (g->image_row0 < 0 || g->image_rows <= 0 || g->image_row0 + g->image_rows > g->height || g->out_row0 < 0 ||
      g->out_rows <= 0 || g->out_row0 + g->out_rows > g->height)
    return fail(RPSF_E_BADARG, "resident row window lies outside the image");
  const int N = p->N;
  // same reach as the reference's 2N padding (transform.py:119-123,141-149); the extreme corners decide
  const long rlo = (long)p->corner_min[0] + g->origin_row, rhi = (long)p->corner_max[0] + g->origin_row;
  const long clo = (long)p->corner_min[1] + g->origin_col, chi = (long)p->corner_max[1] + g->origin_col;
  if (rlo < -2L * N || rhi > (long)g->height + N || clo < -2L * N || chi > (long)g->width + N) {
    for (int i = 0; i < p->n_patches; ++i) {  // name the first offender
      long r = (long)p->h_coords[2 * i] + g->origin_row, c = (long)p->h_coords[2 * i + 1] + g->origin_col;
      if (r < -2L * N || r > (long)g->height + N || c < -2L * N || c > (long)g->width + N)
        return fail(RPSF_E_BADARG, "patch corner (" + std::to_string(r) + ", " + std::to_string(c) +
                                       ") lies outside the 2N-padded image");
    }
  }
  return RPSF_OK;
}

// A batch of frames that share the plan's transfer kernel: frame f at image + f*im_stride, out + f*out_stride (floats)
struct Batch {
  int frames = 1;
  size_t im_stride = 0, out_stride = 0;
};

// Whether the plan's lattice tiles cover the resident output window (rpsf_lattice.hpp): where they do not, the window is cleared first
static bool lattice_covers_window(const rpsf_plan* p, const rpsf_geometry& g) {
  return lattice_covers_window(p->N, p->lat_r0, p->lat_c0, p->nti, p->ntj, g);
}

// Zeroes the resident output window of every frame
static int clear_window(float* d_out, const rpsf_geometry& g, Batch b, hipStream_t st) {
  for (int f = 0; f < b.frames; ++f)
    HIP_TRY(hipMemset2DAsync(d_out + (size_t)f * b.out_stride, (size_t)g.ld_out * sizeof(float), 0, (size_t)g.width * sizeof(float), g.out_rows, st));
  return RPSF_OK;
}

// Kernels that take the frames of a batch along grid.y: launch(first frame, frames) for [0, frames) in slices within the grid.y limit
template <class F>
static void for_frame_slices(int frames, F&& launch) {
  for (int f0 = 0; f0 < frames; f0 += 65535) launch(f0, (unsigned)std::min(65535, frames - f0));
}

// The planes, the output window and the lattice origin as TileSum, SumParams and FixParams all hold them
template <class P>
static void fill_plane_sum(P& s, const rpsf_plan* p, float* d_out, const rpsf_geometry& g, Batch b) {
  s.planes = p->patch.d_planes, s.plane_stride = p->patch.planes_floats, s.planes_frame_floats = 4 * p->patch.planes_floats, s.ld_planes = g.width;
  s.out = d_out, s.ld_out = g.ld_out, s.out_frame_floats = b.out_stride;
  s.rows = g.out_rows, s.W = g.width, s.row0 = g.out_row0;
  s.lat_r0 = p->lat_r0 + g.origin_row, s.lat_c0 = p->lat_c0 + g.origin_col, s.ntj = p->ntj;
}

// Summing workgroups that run beside the patches from the start of a fused launch (multiple of 8: one per XCD), by the
// amount of work in the launch.  256-pixel plan (512-thread workgroups, one per CU): r02y, a band of 520 patches 130-138 us
// with 8, 131-146 with 32; r02av, plane stores kept in the Infinity Cache: 4096^2 0.193 / 0.190 / 0.196 ms with 8 / 16 / 24,
// 8192^2 0.78 / 0.77 / 0.74 / 0.765 ms with 8 / 16 / 32 / 48 - the sooner a tile is summed, the likelier its planes are still
// cached.  128-pixel plan (128-thread workgroups, four per CU): 4096^2 0.217 / 0.214 / 0.212 / 0.206 ms with 16 / 64 / 96 / 128
// against 0.218 ms with the separate sum kernel; 2048^2 0.067 ms with 0 ... 24 against 0.069; 8 x 2048^2 0.372 / 0.360 / 0.352 /
// 0.343 / 0.340 ms with 8 / 32 / 64 / 128 / 192 against 0.362.
static int sum_first_for(const rpsf_plan* p, int frames) {
  if (p->patch.sum_first >= 0) return p->patch.sum_first;
  const long work = (long)p->n_patches * frames;
  if (p->N == 128) return work >= 4096 ? 160 : work >= 2048 ? 128 : work >= 512 ? 8 : 0;  // (160 from 4096 patch-frames on: -2 ... -4 %, profiles/r04bf)
  return work >= 2048 ? 32 : work >= 1024 ? 16 : work >= 512 ? 8 : 0;
}

// What the persistent kernels are compiled for (hot_geometry, rpsf_lattice.hpp), for this plan, image and frame stride
static bool hot_geometry(const rpsf_plan* p, const float* d_img, const rpsf_geometry& g, size_t im_stride) {
  const bool aligned16 = im_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(d_img) & 15) == 0 && p->patch.planes_floats % 4 == 0;
  return hot_geometry(g, p->lattice, p->lat_c0, aligned16);
}

// What the patch launch of one apply is: decided by patch_launch_for from the plan as it stands, committed by launch_apply (the queue positions the
// launch takes) and turned into PatchParams and a kernel by launch_patches.
struct PatchLaunch {
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
  uint32_t xq_base[8], xq_draws[8];      // persistent: where this launch's draws from the slot queue of each XCD start, and how many it makes
  uint32_t sum_queue_base, sum_queue_draws;  // fused and persistent: the same for the tile queue
};

// A patch launch is one grid of at most 2^31 - 1 workgroups: one per frame and patch_teams() patches of each chunk
static bool patch_launch_too_large(const rpsf_plan* p, int frames) {
  const int teams = patch_teams(p->N);
  return (size_t)8 * (chunk_patches(p->n_patches, teams) / teams) * frames > 0x7fffffffu;
}

// fused: the plane sum runs in this launch (see PatchPath::d_tile_done)
template <class T>
static PatchLaunch patch_launch_for(const rpsf_plan* p, const float* d_img, const rpsf_geometry& g, Batch b, bool fused) {
  constexpr bool N256 = T::V2 && T::Cfg::N == 256, N128 = T::V2 && T::Cfg::N == 128;
  PatchLaunch L{};
  L.chunk = chunk_patches(p->n_patches, T::TEAMS);
  L.stagger_ticks = std::max(0, p->patch.stagger_us) * 100;
  L.grid = (unsigned)((size_t)8 * (L.chunk / T::TEAMS) * b.frames);  // (patch_launch_too_large: it fits)
  L.form = T::V2 ? PatchLaunch::GEN2 : PatchLaunch::GEN1;
  L.stagger_blocks = T::V2 ? p->patch.round_capacity : p->cu_count * std::max(1, 512 / T::WG);
  L.patch_blocks = T::V2 ? (int)L.grid : 0;  // (the first-generation kernel does not read it)
  if (!fused) return L;                      // (fused: second-generation plans only, launch_apply)
  const int count = p->nti * p->ntj * b.frames;  // positions of the tile list
  // Persistent batches whose planes would not fit the Infinity Cache side by side run frame after frame in one launch: every
  // frame keeps the cache behaviour of a single apply, and the next frame's patches take the CUs the previous one's last
  // patches leave idle (RPSF_FRAME_MAJOR=0/1 overrides).
  bool frame_major = N256 && p->patch.persist && b.frames > 1 && p->n_patches >= 1024 &&
                     16.0 * (double)p->patch.planes_floats * b.frames > 256.0 * 1048576.0;  // (8 x 2048^2: 0.056 ms per frame side by side, 0.061 in turn)
  if (const char* e = dev_env("RPSF_FRAME_MAJOR"))  // development sweeps: 0 = never, 2 = any persistent batch
    frame_major = std::atoi(e) == 2 ? (p->patch.persist && b.frames > 1) : (frame_major && std::atoi(e) != 0);
  L.frame_major = frame_major ? 1 : 0;
  // Frames of a batch side by side keep the planes of ALL of them live at once (8 x 2048^2: 537 MB against a 256 MiB Infinity Cache): the 128-pixel
  // kernels then store them with the streaming hint - 0.3156 -> 0.3009 ms (-4.7 %); a single frame loses 8 % that way, and so does the 256-pixel
  // plan at either size (profiles/r04bd).  RPSF_PLANE_NT=0/1 overrides (development sweeps).
  // (needs the plain-load form of K - a batch shares it - and planes well beyond the Infinity Cache: 4 x 2048^2, 268 MB, still loses 3 %; 6 x, 403 MB, gains 5 %)
  L.plane_nt = N128 && p->patch.k_cached && b.frames > 1 && !frame_major && 16.0 * (double)p->patch.planes_floats * b.frames > 300.0 * 1048576.0;
  if (p->patch.plane_nt_opt >= 0) L.plane_nt = p->patch.plane_nt_opt != 0 && N128 && p->patch.k_cached;  // (RPSF_OPT_PLANE_NT)
  const int tune_frames = b.frames;  // (the settings of a single apply measured worse here: 0.203 vs 0.186 ms per frame at 8 x 4096^2)
  L.sum_first = sum_first_for(p, tune_frames);
  L.sum_queue_base = p->patch.sum_queue_base;
  // persistent form: as many patch workgroups as the chip holds beside the summing ones; each works through the slots
  // of its XCD's chunk and ends as a summing workgroup itself (no workgroups behind the patches).
  // FORWARD PROGRESS.  HIP promises neither that a grid is resident as a whole nor an order of dispatch, and other launches
  // (a second plan on another stream, RCCL's kernels) may hold CUs.  What this launch needs: (1) every patch slot is drawn
  // from its chunk's queue - none is tied to a particular workgroup - so the slots of chunk x are worked off by whichever
  // workgroups with blockIdx % 8 == x are resident, and a workgroup turns to summing only when its chunk's queue is empty,
  // i.e. when every remaining patch of the chunk is in the hands of a resident workgroup that does not wait for anything;
  // (2) summing workgroups wait (poll + s_sleep) only for tiles whose patches are drawn or will be drawn by (1).  So the
  // launch completes as soon as, for every chunk, ONE patch workgroup gets a CU: in dispatch order the first sum_first + 8
  // workgroups.  The only workgroups that hold a CU without progress of their own are the sum_first head summing ones (<= 32 of
  // 512 threads for the 256-pixel plan; up to 160 of 128 threads - four to a CU, 40 CUs' worth - for the 128-pixel plan from 4096
  // patch-frames on, sum_first_for); concurrent persistent launches therefore cannot starve one another unless their head summing
  // workgroups alone fill the chip (tests: test_two_persistent_plans_on_two_streams, 256- and 128-pixel plans).
  // (queue positions of an XCD: chunk slots x frames, the frames of a slot side by side)
  const int rows = std::min(L.chunk * b.frames, std::max(1, (p->patch.round_capacity - L.sum_first - p->patch.reserved_cus) / 8));
  if (!(p->patch.persist && rows > 0 && hot_geometry(p, d_img, g, b.im_stride))) {
    L.form = PatchLaunch::FUSED;
    const int nsum = std::max(8, std::min(count, p->patch.round_capacity)) + L.sum_first;  // at the tail: as many summing workgroups as the chip holds
    L.sum_queue_draws = (uint32_t)(count + nsum);  // every workgroup draws one position past the end
    L.grid += (unsigned)nsum;
    return L;
  }
  L.form = PatchLaunch::PERSISTENT, L.rows = rows;
  L.variant = !p->patch.k_cached ? PatchLaunch::PLAIN : L.plane_nt ? PatchLaunch::K_CACHED_PLANES_NT : PatchLaunch::K_CACHED;
  // a head summing workgroup would idle through the first patch period (no tile is complete before that): it computes one patch
  // of its XCD's chunk first (RPSF_HEAD_PATCHES=0: off)
  L.head_patches = p->patch.head_patches;
  L.prefetch = p->patch.prefetch && p->patch.d_prefetch_tiles ? 1 : 0;
  L.k_prefetch = N256 && !L.head_patches ? p->patch.k_prefetch : 0;
  // persistent workgroups keep the phase they start with: holding the resident ones back by up to 10 us spreads the
  // store bursts of the chip over the patch period (profiles/r02ai, r02ak: -2..3 % from four rounds of patches on; with the
  // plane stores kept in the Infinity Cache, r02av: 0.210 / 0.208 / 0.193 / 0.190 / 0.189 / 0.191 / 0.195 ms at 0 / 5 / 8 / 10 / 12 / 15 / 20 us)
  // (and smaller launches too: 2048^2 0.0811 -> 0.0787 ms, 3072^2 0.138 -> 0.131 ms, a band of 520 patches 128 -> 121 us)
  // (long launches take more: 8192^2 0.736 / 0.726 / 0.714 / 0.703 / 0.698 / 0.719 ms at 6 / 12 / 18 / 24 / 30 / 36 us)
  // (round 4, seven-barrier pass, profiles/r04az: 4096^2 at 12 / 16 / 20 us - the repeated frame 0.1835 / 0.1843 / 0.1880 ms, a NEW frame every step
  // 0.2019 / 0.1962 / 0.1933: 16 us from 1024 patches of the 256-pixel plan on; 8192^2 0.714 / 0.688 / 0.691 / 0.690 at 12 / 16 / 20 / 24)
  if (p->patch.stagger_us < 0 && (long)p->n_patches * tune_frames >= 256) {
    const long work = (long)p->n_patches * tune_frames;
    L.stagger_ticks = work >= 2048 ? 2400 : (work >= 1024 && N256) ? 1600 : 1200;
    // The 128-pixel plan - four workgroups per CU, out of step with one another anyway - is better off WITHOUT it since round 4 (profiles/r04ba):
    // 2048^2 0.0655 -> 0.0603 ms (-8 %), 3072^2 -6 %, 8 x 2048^2 0.3252 -> 0.3198; only single frames of 4096^2 and more still take a short one
    // (6 us: -1 ... -3 %).
    if (N128) L.stagger_ticks = tune_frames == 1 && p->n_patches >= 4096 ? 600 : 0;
  }
  for (int x = 0; x < 8; ++x) {
    L.xq_base[x] = p->patch.xq_base[x];
    // draws of this launch: one per slot and frame, plus the one past the end that tells each of the chunk's workgroups to stop
    // (the first sum_first / 8 positions of a chunk go to the head summing workgroups without a draw when those compute a patch first)
    const int slots_x = std::min(L.chunk, std::max(0, p->n_patches - x * L.chunk)) * b.frames;
    L.xq_draws[x] = (uint32_t)(std::max(0, slots_x - (L.head_patches ? L.sum_first / 8 : 0)) + rows);
  }
  const int wgs = L.sum_first + 8 * rows;
  L.sum_queue_draws = (uint32_t)(count + wgs);  // every workgroup draws one position past the end
  L.grid = (unsigned)wgs;
  return L;
}

static PatchParams patch_params(const rpsf_plan* p, const PatchLaunch& L, const float* d_img, float* d_out, const rpsf_geometry& g, OverlapKind kind,
                                Batch b) {
  PatchParams pp{};
  pp.im = ImageView{d_img, g.height, g.width, g.ld_image, g.pad_mode, g.pad_value, g.image_row0, g.image_rows};
  if (kind != OV_ATOMIC)
    pp.ov = OutView{p->patch.d_planes, g.height, g.width, g.width, g.out_row0, g.out_rows, p->patch.planes_floats, p->patch.d_sink};
  else
    pp.ov = OutView{d_out, g.height, g.width, g.ld_out, g.out_row0, g.out_rows, 0, p->patch.d_sink};
  pp.origin_row = g.origin_row, pp.origin_col = g.origin_col;
  pp.desc = p->d_desc, pp.n_patches = p->n_patches, pp.seq_base = 0;
  const rpsf_plan* o = owner(p);
  pp.tab = o->patch.d_tab, pp.pairtab = o->patch.d_pairtab, pp.tw = o->patch.d_tw, pp.win = o->d_win, pp.g = o->patch.d_g, pp.gs = o->patch.d_gs;
  pp.stamps = p->patch.d_stamps;
  pp.chunk = L.chunk, pp.slot0 = 0, pp.patch_blocks = L.patch_blocks;
  pp.stagger_ticks = L.stagger_ticks, pp.stagger_blocks = L.stagger_blocks;
  pp.n_frames = b.frames, pp.im_frame_floats = b.im_stride;
  pp.ov_frame_floats = kind != OV_ATOMIC ? 4 * p->patch.planes_floats : b.out_stride;
  pp.dv = OutView{nullptr, 0, 0, 0, 0, 0, 0, nullptr};
  if (kind == OV_DIRECT) {
    pp.dv = OutView{d_out, g.height, g.width, g.ld_out, g.out_row0, g.out_rows, 0, p->patch.d_sink};
    pp.dv_frame_floats = b.out_stride;
    pp.quads = p->patch.d_quads, pp.flags = p->patch.d_flags, pp.dyn_side = p->patch.d_dyn, pp.chunk_xcc = p->patch.d_chunk_xcc;
    pp.flag_epoch = p->patch.epoch, pp.n_tiles = (uint32_t)(p->nti * p->ntj), pp.orphan_mod = p->patch.orphan_mod;
  }
  if (L.form != PatchLaunch::FUSED && L.form != PatchLaunch::PERSISTENT) return pp;
  const int n_tiles = p->nti * p->ntj;
  pp.tile_done = p->patch.d_tile_done, pp.quads = p->patch.d_quads, pp.n_tiles = (uint32_t)n_tiles;
  pp.sum_first = L.sum_first, pp.frame_major = L.frame_major, pp.plane_nt = L.plane_nt;
  TileSum& ts = pp.ts;
  fill_plane_sum(ts, p, d_out, g, b);
  ts.half = p->N / 2, ts.cover = p->d_cover, ts.tiles = p->patch.d_sum_order, ts.count = n_tiles * b.frames;
  ts.done = p->patch.d_tile_done, ts.epoch = p->patch.done_epoch;
  ts.n_frames = b.frames, ts.n_tiles = (uint32_t)n_tiles, ts.n_tiles_listed = (uint32_t)n_tiles, ts.frame_major = L.frame_major;
  ts.queue = p->patch.d_sum_queue, ts.queue_base = L.sum_queue_base;
  if (L.form != PatchLaunch::PERSISTENT) return pp;
  pp.persist = L.rows, pp.xq = p->patch.d_xq;
  pp.head_patches = L.head_patches, pp.prefetch = L.prefetch, pp.prefetch_tiles = p->patch.d_prefetch_tiles;
  pp.k_prefetch = L.k_prefetch, pp.k_patches = o->n_patches;
  for (int x = 0; x < 9; ++x) pp.prefetch_first[x] = p->patch.prefetch_first[x];
  for (int x = 0; x < 8; ++x) pp.xq_base[x] = L.xq_base[x];
  return pp;
}

// The patch kernels of one apply, in the form patch_launch_for decided (the FORWARD PROGRESS argument of the persistent form is there)
static int launch_patches(const rpsf_plan* p, const PatchLaunch& L, const float* d_img, float* d_out, const rpsf_geometry& g, OverlapKind kind,
                          hipStream_t st, Batch b) {
  const PatchParams pp = patch_params(p, L, d_img, d_out, g, kind, b);
  return dispatch_patch(p->patch.v2, p->N, [&]<class T>() -> int {
    const dim3 grid(L.grid), wg(T::WG);
    if (L.form != PatchLaunch::PERSISTENT) T::kernel()<<<grid, wg, T::LDS_BYTES, st>>>(pp);
    else if constexpr (T::V2) {
      using Persistent = PersistentKernel2<typename T::Cfg>;
      switch (L.variant) {
        case PatchLaunch::PLAIN: Persistent::fn<<<grid, wg, T::LDS_BYTES, st>>>(pp); break;
        case PatchLaunch::K_CACHED: Persistent::fn_k_cached<<<grid, wg, T::LDS_BYTES, st>>>(pp); break;
        case PatchLaunch::K_CACHED_PLANES_NT: Persistent::fn_k_cached_planes_nt<<<grid, wg, T::LDS_BYTES, st>>>(pp); break;
      }
    }
    HIP_TRY(hipGetLastError());
    return RPSF_OK;
  });
}

static int launch_fixup(const rpsf_plan* p, float* d_out, const rpsf_geometry& g, hipStream_t st, Batch b) {
  FixParams fp{};
  fill_plane_sum(fp, p, d_out, g, b);
  fp.half = p->N / 2;
  fp.tile_info = p->patch.d_tile_info, fp.flags = p->patch.d_flags, fp.dyn_side = p->patch.d_dyn;
  fp.epoch = p->patch.epoch, fp.n_tiles = (uint32_t)(p->nti * p->ntj);
  for_frame_slices(b.frames, [&](int f0, unsigned frames) {
    FixParams q = fp;
    q.planes += (size_t)f0 * q.planes_frame_floats, q.out += (size_t)f0 * q.out_frame_floats;
    q.flags += (size_t)f0 * q.n_tiles, q.dyn_side += (size_t)f0 * q.n_tiles;
    fixup_kernel<<<dim3(fp.n_tiles * FIX_SUB, frames), dim3(256), 0, st>>>(q);
  });
  HIP_TRY(hipGetLastError());
  return RPSF_OK;
}

// The separate plane sum over the whole resident window
static int launch_sum(const rpsf_plan* p, float* d_out, const rpsf_geometry& g, hipStream_t st, Batch b) {
  SumParams sp{};
  fill_plane_sum(sp, p, d_out, g, b);
  sp.row_begin = 0, sp.nti = p->nti, sp.cover = p->d_cover;
  sp.half_shift = 0;
  while ((1 << (sp.half_shift + 1)) < p->N) ++sp.half_shift;
  const size_t total = (size_t)((g.width + 3) / 4) * sp.rows;
  for_frame_slices(b.frames, [&](int f0, unsigned frames) {
    SumParams q = sp;
    q.planes += (size_t)f0 * q.planes_frame_floats, q.out += (size_t)f0 * q.out_frame_floats;
    sum_planes_kernel<<<dim3((unsigned)((total + 255) / 256), frames), dim3(256), 0, st>>>(q);
  });
  HIP_TRY(hipGetLastError());
  return RPSF_OK;
}

static OverlapKind overlap_kind(const rpsf_plan* p) {
  switch (p->overlap_mode) {
    case 1: return OV_ATOMIC;
    case 2: return OV_PLANES;
    case 3: return OV_DIRECT;
    case 4: return OV_SWEEP;
    default: return p->sweep.ok ? OV_SWEEP : p->lattice ? OV_PLANES : OV_ATOMIC;  // direct stays opt-in until it beats the planes
  }
}

static int launch_apply_generic(rpsf_plan* p, const float* d_img, float* d_out, const rpsf_geometry& g, hipStream_t st,
                                hipEvent_t ev_k0, hipEvent_t ev_k1, Batch b) {
  if (g.image_row0 != 0 || g.image_rows != g.height || g.out_row0 != 0 || g.out_rows != g.height)
    return fail(RPSF_E_UNSUPPORTED, "row-band windows need a patch size with a compiled plan (16, 32, 64, 128, 256)");
  if (st != p->stream) {
    HIP_TRY(hipStreamSynchronize(p->stream));  // the FFT plan is bound to one stream at a time
    if (g_hipfft.set_stream(p->fft.plan.get(), st) != 0) return fail(RPSF_E_HIP, "hipfftSetStream failed");
  }
  const size_t per = (size_t)p->N * p->N;
  const float scale = 1.0f / (float)per;  // hipFFT's inverse is unnormalised
  if (ev_k0) HIP_TRY(hipEventRecord(ev_k0, st));
  for (int f = 0; f < b.frames; ++f) {
    const float* img = d_img + (size_t)f * b.im_stride;
    float* out = d_out + (size_t)f * b.out_stride;
    if (const int rc = clear_window(out, g, Batch(), st); rc != RPSF_OK) return rc;
    for (int first = 0; first < p->n_patches; first += p->fft.chunk) {
      GenericGeom gg;
      gg.N = p->N, gg.first = first, gg.count = std::min(p->fft.chunk, p->n_patches - first);
      gg.origin_row = g.origin_row, gg.origin_col = g.origin_col;
      gg.im = ImageView{img, g.height, g.width, g.ld_image, g.pad_mode, g.pad_value, 0, g.height};
      gg.ov = OutView{out, g.height, g.width, g.ld_out, 0, g.height, 0, nullptr};
      const size_t total = per * gg.count;
      const unsigned grid = (unsigned)((total + 255) / 256);
      generic_gather_kernel<<<dim3(grid), dim3(256), 0, st>>>(gg, p->d_coords, p->fft.d_win, p->fft.d_buf);
      // a short last chunk still runs the full-size plan: the surplus patches hold stale data and are never scattered
      if (g_hipfft.exec_c2c(p->fft.plan.get(), p->fft.d_buf, p->fft.d_buf, /*HIPFFT_FORWARD*/ -1) != 0)
        return fail(RPSF_E_HIP, "hipfftExecC2C (forward) failed");
      generic_multiply_kernel<<<dim3(grid), dim3(256), 0, st>>>(p->fft.d_buf, p->fft.d_kfull + (size_t)first * per, total, scale);
      if (g_hipfft.exec_c2c(p->fft.plan.get(), p->fft.d_buf, p->fft.d_buf, /*HIPFFT_BACKWARD*/ 1) != 0)
        return fail(RPSF_E_HIP, "hipfftExecC2C (inverse) failed");
      if (p->fft.d_colour && overlap_kind(p) != OV_ATOMIC) {
        for (int colour = 0; colour < 4; ++colour)
          generic_scatter_kernel<<<dim3(grid), dim3(256), 0, st>>>(gg, p->d_coords, p->fft.d_win, p->fft.d_buf, p->fft.d_colour, colour);
      } else {
        generic_scatter_kernel<<<dim3(grid), dim3(256), 0, st>>>(gg, p->d_coords, p->fft.d_win, p->fft.d_buf, nullptr, -1);
      }
      HIP_TRY(hipGetLastError());
    }
  }
  if (ev_k1) HIP_TRY(hipEventRecord(ev_k1, st));
  if (st != p->stream) {
    HIP_TRY(hipStreamSynchronize(st));
    if (g_hipfft.set_stream(p->fft.plan.get(), p->stream) != 0) return fail(RPSF_E_HIP, "hipfftSetStream failed");
  }
  return RPSF_OK;
}

// Third generation (N <= 64): the whole apply is this one launch (rpsf_kernels3.hpp); frames of a batch along grid.y
static int launch_sweep(rpsf_plan* p, const float* d_img, float* d_out, const rpsf_geometry& g, hipStream_t st, hipEvent_t ev_k0, hipEvent_t ev_k1,
                        Batch b) {
  const long r0 = (long)p->lat_r0 + g.origin_row, c0 = (long)p->lat_c0 + g.origin_col;
  if (const int rc = lattice_covers_window(p, g) ? RPSF_OK : clear_window(d_out, g, b, st); rc != RPSF_OK) return rc;
  SweepParams sp{};
  sp.im = ImageView{d_img, g.height, g.width, g.ld_image, g.pad_mode, g.pad_value, g.image_row0, g.image_rows};
  const bool col_aligned = (c0 & 3) == 0;
  sp.aligned_in = col_aligned && g.ld_image % 4 == 0 && b.im_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(d_img) & 15) == 0;
  const int aligned_out = col_aligned && g.ld_out % 4 == 0 && b.out_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0;
  sp.fl = Flush3{d_out, g.ld_out, g.out_row0, g.out_rows, g.height, g.width, aligned_out};
  sp.lat_r0 = (int)r0, sp.lat_c0 = (int)c0;
  sp.jobs = p->sweep.d_jobs, sp.regions = p->sweep.d_regions, sp.n_regions = p->sweep.n_regions, sp.group = (p->sweep.n_regions + 7) / 8;
  const rpsf_plan* o = owner(p);
  sp.k3 = o->sweep.d_k3, sp.win = o->d_win, sp.zeros = p->sweep.d_zero, sp.err = o->sweep.d_err, sp.stamps = p->sweep.d_stamps;
  sp.im_frame_floats = b.im_stride, sp.out_frame_floats = b.out_stride;
  // K by plain loads when frames share it or it is small enough to stay in the Infinity Cache from one apply to the next, else streamed
  const bool k_plain = b.frames > 1 || o->sweep.k3_floats * sizeof(float) <= ((size_t)96 << 20);
  if (ev_k0) HIP_TRY(hipEventRecord(ev_k0, st));
  for_frame_slices(b.frames, [&](int f0, unsigned frames) {
    SweepParams q = sp;
    q.im.img += (size_t)f0 * b.im_stride, q.fl.out += (size_t)f0 * b.out_stride;
    const dim3 grid((unsigned)(8 * sp.group), frames);
    (void)dispatch_v3(p->N, [&]<class C>() -> int {  // (a plan with sweep lists has a third-generation configuration)
      if (k_plain) sweep_kernel_kc<C><<<grid, dim3(C::WG), C::LDS_BYTES, st>>>(q);
      else sweep_kernel<C><<<grid, dim3(C::WG), C::LDS_BYTES, st>>>(q);
      return RPSF_OK;
    });
  });
  HIP_TRY(hipGetLastError());
  if (ev_k1) HIP_TRY(hipEventRecord(ev_k1, st));
  return RPSF_OK;
}

// One apply.  ev_k0 / ev_k1 (optional) bracket the patch-kernel launches for timing.
// In this order: every refusal; growth of the plan's scratch (harmless before a launch that fails); the decision, which reads the scratch sizes; then
// what a launch must not be refused after - epochs, counter restarts, queue positions -; the clear; the launches.
static int launch_apply(rpsf_plan* p, const float* d_img, float* d_out, const rpsf_geometry& g, hipStream_t st,
                        hipEvent_t ev_k0, hipEvent_t ev_k1 = nullptr, Batch b = Batch()) {
  if (p->generic) return launch_apply_generic(p, d_img, d_out, g, st, ev_k0, ev_k1, b);
  const OverlapKind kind = overlap_kind(p);
  if (kind == OV_SWEEP) {
    if (!p->sweep.ok) return fail(RPSF_E_STATE, "the sweep kernel needs a 16-, 32- or 64-pixel patch on a complete lattice of at least 2 x 2 patches");
    return launch_sweep(p, d_img, d_out, g, st, ev_k0, ev_k1, b);
  }
  if (kind != OV_ATOMIC && !p->lattice) return fail(RPSF_E_STATE, "colour planes need a regular half-overlap lattice of patch corners");
  if (kind == OV_DIRECT && !p->patch.direct_ok) return fail(RPSF_E_STATE, "direct overlap-add needs a lattice and a 128- or 256-pixel patch");
  if (kind == OV_DIRECT && (size_t)g.out_rows * g.ld_out * sizeof(float) >= ((size_t)1 << 32))
    return fail(RPSF_E_UNSUPPORTED, "direct overlap-add addresses the output through a 32-bit buffer offset: frame too large");
  if (patch_launch_too_large(p, b.frames)) return fail(RPSF_E_BADARG, "batch too large for one launch");
  // Fused plane sum: what the plan must have, and the geometry the summing workgroups are written for (fused_geometry, rpsf_lattice.hpp)
  const bool fused = kind == OV_PLANES && p->patch.v2 && p->patch.fuse_pays && p->patch.d_tile_done && !p->patch.no_fuse && b.frames <= 255 &&
                     fused_geometry(g, p->lat_c0, (reinterpret_cast<uintptr_t>(d_out) & 15) == 0);
  const size_t n_tiles = (size_t)p->nti * p->ntj;
  // The plan's scratch (planes, flags) serves one apply at a time: an apply on another stream waits for the last one.
  // A plan that has only ever been applied on one stream records nothing behind its launches (stream order is all it needs, and back-to-back
  // applies then have nothing between them but what the caller puts there).  The first apply that arrives on another stream waits on the host,
  // once, for what the plan has enqueued so far - device-wide, because the previous stream is the caller's and may be gone by now - and from
  // then on every apply records the event and an apply on another stream waits for it.
  if (p->busy_valid && st != p->last_stream) {
    if (p->multi_stream) HIP_TRY(hipStreamWaitEvent(st, p->ev_busy, 0));
    else {
      HIP_TRY(hipDeviceSynchronize());
      p->multi_stream = true;
    }
  }
  if (kind != OV_ATOMIC) {
    const size_t need = plane_floats_needed(g);
    if (need > p->patch.planes_floats || (size_t)b.frames > p->patch.planes_frames) {  // four planes per frame in flight
      const size_t per = std::max(need, p->patch.planes_floats), frames = std::max((size_t)b.frames, p->patch.planes_frames);
      HIP_TRY(hipDeviceSynchronize());  // earlier applies, on whatever stream, may still use the old planes
      p->patch.planes_floats = 0, p->patch.planes_frames = 0;
      HIP_TRY(p->patch.d_planes.alloc(4 * per * frames));
      p->patch.planes_floats = per, p->patch.planes_frames = frames;
    }
  }
  if (kind == OV_DIRECT && (size_t)b.frames > p->patch.flag_frames) {
    HIP_TRY(hipDeviceSynchronize());
    p->patch.d_flags.reset(), p->patch.d_dyn.reset(), p->patch.flag_frames = 0;
    HIP_TRY(p->patch.d_flags.alloc(n_tiles * b.frames));
    HIP_TRY(p->patch.d_dyn.alloc(n_tiles * b.frames));
    HIP_TRY(hipMemset(p->patch.d_flags, 0, n_tiles * b.frames * sizeof(uint32_t)));
    HIP_TRY(hipMemset(p->patch.d_dyn, 0, n_tiles * b.frames * sizeof(uint32_t)));
    p->patch.flag_frames = (size_t)b.frames;
  }
  if (fused && (size_t)b.frames > p->patch.done_frames) {  // one set of tile counters per frame of a batch
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(p->patch.d_tile_done.alloc(n_tiles * b.frames));
    HIP_TRY(hipMemset(p->patch.d_tile_done, 0, n_tiles * b.frames * sizeof(uint32_t)));
    p->patch.done_frames = (size_t)b.frames;  // (more frames than any launch before, the last one included: a new count starts below)
  }
  PatchLaunch L{};
  (void)dispatch_patch(p->patch.v2, p->N, [&]<class T>() -> int {
    L = patch_launch_for<T>(p, d_img, g, b, fused);
    return RPSF_OK;
  });
  // ---- nothing refuses the launch from here on: the plan's epochs, counters and queue positions advance ----
  if (kind == OV_DIRECT && ++p->patch.epoch >= (1u << 24) - 1) {  // the epoch field of the flag words is 24 bits wide
    HIP_TRY(hipMemsetAsync(p->patch.d_flags, 0, n_tiles * p->patch.flag_frames * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(p->patch.d_chunk_xcc, 0, 8 * sizeof(uint32_t), st));
    p->patch.epoch = 1;
  }
  if (fused) {
    // A launch advances the counters of frames [0, b.frames) only, and a tile is complete at epoch x contributors: when the frame
    // count differs from the previous fused launch's (batch -> single apply -> batch, or the short last group of a batch) the
    // counters of the higher frames would lag behind the epoch for ever - and the summing workgroups would wait for ever.
    // Start a new count whenever the frame count changes (and when the epoch would overflow the counters).
    const bool restart = b.frames != p->patch.done_last_frames || p->patch.done_epoch + 1 >= (1u << 29);  // the counters hold epoch * contributors
    if (restart) HIP_TRY(hipMemsetAsync(p->patch.d_tile_done, 0, n_tiles * p->patch.done_frames * sizeof(uint32_t), st));
    p->patch.done_last_frames = b.frames;
    p->patch.done_epoch = restart ? 1 : p->patch.done_epoch + 1;
  }
  for (int x = 0; x < 8; ++x) p->patch.xq_base[x] += L.xq_draws[x];
  p->patch.sum_queue_base += L.sum_queue_draws;
  // atomics accumulate into the output; the tile sums and the direct mode's fix-up write lattice tiles only
  const bool clear = kind == OV_ATOMIC || ((kind == OV_DIRECT || fused) && !lattice_covers_window(p, g));
  if (const int rc = clear ? clear_window(d_out, g, b, st) : RPSF_OK; rc != RPSF_OK) return rc;
  if (ev_k0) HIP_TRY(hipEventRecord(ev_k0, st));
  int rc = launch_patches(p, L, d_img, d_out, g, kind, st, b);
  if (rc != RPSF_OK) return rc;
  if (ev_k1) HIP_TRY(hipEventRecord(ev_k1, st));
  if (kind == OV_PLANES && !fused) rc = launch_sum(p, d_out, g, st, b);
  if (kind == OV_DIRECT) rc = launch_fixup(p, d_out, g, st, b);
  if (rc != RPSF_OK) return rc;
  if (p->multi_stream) HIP_TRY(hipEventRecord(p->ev_busy, st));
  p->last_stream = st, p->busy_valid = true;
  return RPSF_OK;
}

extern "C" int rpsf_plan_set_overlap_mode(rpsf_plan* p, int mode) {
  if (!p || mode < 0 || mode > 4) return fail(RPSF_E_BADARG, "mode must be 0 (auto), 1 (atomics), 2 (colour planes), 3 (direct) or 4 (sweep)");
  if (mode == 4 && !p->sweep.ok) return fail(RPSF_E_STATE, "the sweep kernel needs a 16-, 32- or 64-pixel patch on a complete lattice of at least 2 x 2 patches");
  if (mode == 2 && !p->lattice) return fail(RPSF_E_STATE, "colour planes need a regular half-overlap lattice of patch corners");
  if (mode == 3 && !p->patch.direct_ok) return fail(RPSF_E_STATE, "direct overlap-add needs a regular half-overlap lattice and a 128- or 256-pixel patch");
  p->overlap_mode = mode;
  drop_bands(p);
  return RPSF_OK;
}

extern "C" int rpsf_plan_set_option(rpsf_plan* p, int option, int value) {
  if (!p) return fail(RPSF_E_BADARG, "null plan");
  switch (option) {
    case RPSF_OPT_PERSIST:
      if (value != 0 && value != 1) return fail(RPSF_E_BADARG, "RPSF_OPT_PERSIST takes 0 or 1");
      p->patch.persist = value != 0 && (p->N == 256 || p->N == 128);
      break;
    case RPSF_OPT_FUSE:
      if (value != 0 && value != 1) return fail(RPSF_E_BADARG, "RPSF_OPT_FUSE takes 0 or 1");
      p->patch.no_fuse = value == 0;
      break;
    case RPSF_OPT_K_CACHED:
      if (value != 0 && value != 1) return fail(RPSF_E_BADARG, "RPSF_OPT_K_CACHED takes 0 or 1");
      p->patch.k_cached = value != 0;
      break;
    case RPSF_OPT_PLANE_NT:
      if (value < -1 || value > 1) return fail(RPSF_E_BADARG, "RPSF_OPT_PLANE_NT takes -1 (automatic), 0 or 1");
      p->patch.plane_nt_opt = value;
      break;
    case RPSF_OPT_HOST_BANDS:
      if (value < -1 || value > 64) return fail(RPSF_E_BADARG, "RPSF_OPT_HOST_BANDS takes -1 (automatic) or 0..64");
      p->host_bands_opt = value;
      break;
    case RPSF_OPT_STREAM_GROUP:
      if (value < 0 || value > 64) return fail(RPSF_E_BADARG, "RPSF_OPT_STREAM_GROUP takes 0 (automatic) or 1..64");
      p->stream_group_opt = value;
      break;
    case RPSF_OPT_STREAM_DEPTH:
      if (value < 0 || value > 16) return fail(RPSF_E_BADARG, "RPSF_OPT_STREAM_DEPTH takes 0 (automatic) or 1..16");
      p->stream_depth_opt = value;
      break;
    case RPSF_OPT_HEAD_KPREFETCH:
      if (value != 0 && value != 1) return fail(RPSF_E_BADARG, "RPSF_OPT_HEAD_KPREFETCH takes 0 or 1");
      p->patch.k_prefetch = p->N == 256 ? value : 0;
      break;
    case RPSF_OPT_SAT_GROUP:
      if (value < 0 || value > 65535) return fail(RPSF_E_BADARG, "RPSF_OPT_SAT_GROUP takes 0 (automatic) or 1..65535");
      p->sat_group_opt = value;
      return RPSF_OK;  // (no launch of the correction depends on it: the band views stay)
    case RPSF_OPT_DEBUG_ORPHAN:
      if (value < 0) return fail(RPSF_E_BADARG, "RPSF_OPT_DEBUG_ORPHAN takes 0 (off) or a positive modulus");
      p->patch.orphan_mod = value;
      break;
    default: return fail(RPSF_E_BADARG, "unknown plan option");
  }
  drop_bands(p);  // (views inherit nothing: they are rebuilt with the parent's settings at the next host frame)
  return RPSF_OK;
}

extern "C" int rpsf_plan_set_sweep_regions(rpsf_plan* p, int target_regions) {
  if (!p || target_regions < 1 || target_regions > (1 << 20)) return fail(RPSF_E_BADARG, "target_regions must be 1..2^20");
  if (!p->sweep.ok) return fail(RPSF_E_STATE, "the sweep kernel needs a 16-, 32- or 64-pixel patch on a complete lattice of at least 2 x 2 patches");
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  HIP_TRY(hipDeviceSynchronize());  // (applies on other streams may still read the old lists)
  drop_bands(p);
  return build_sweep_lists(p, target_regions);
}
extern "C" int rpsf_plan_host_bands(const rpsf_plan* p, int* bands) {
  if (!p || !bands) return fail(RPSF_E_BADARG, "null argument");
  *bands = p->last_host_bands;
  return RPSF_OK;
}
extern "C" int rpsf_plan_sweep_info(const rpsf_plan* p, int* regions, long* jobs, long* patch_slots, int* slabs_per_phase) {
  if (!p) return fail(RPSF_E_BADARG, "null plan");
  if (regions) *regions = p->sweep.ok ? p->sweep.n_regions : 0;
  if (jobs) *jobs = p->sweep.ok ? p->sweep.slabs : 0;
  if (patch_slots) *patch_slots = p->sweep.ok ? p->sweep.patch_slots : 0;
  if (slabs_per_phase) *slabs_per_phase = p->sweep.ok ? p->sweep.ks : 0;
  return RPSF_OK;
}

// Diagnostic builds only (-DRPSF_STAMPS): copy out the 16 per-patch phase timestamps (10 ns ticks).
extern "C" int rpsf_plan_debug_stamps(rpsf_plan* p, unsigned long long* host, size_t count) {
  if (!p || !host) return fail(RPSF_E_BADARG, "null argument");
  if (p->sweep.d_stamps) {  // third generation: [region][wave][job slot < 8][16]
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipDeviceSynchronize());
    count = std::min(count, (size_t)std::max(512, p->sweep.n_regions) * 8 * 8 * 16);
    HIP_TRY(hipMemcpy(host, p->sweep.d_stamps, count * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RPSF_OK;
  }
  if (!p->patch.d_stamps) return fail(RPSF_E_STATE, "phase timestamps exist only in builds with -DRPSF_STAMPS");
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipDeviceSynchronize());
#if defined(RPSF_WAVE_STAMPS)
  count = std::min(count, (size_t)16 * 8 * p->n_patches);
#else
  count = std::min(count, (size_t)16 * p->n_patches);
#endif
  HIP_TRY(hipMemcpy(host, p->patch.d_stamps, count * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return RPSF_OK;
}


extern "C" int rpsf_plan_set_reserved_cus(rpsf_plan* p, int cus) {
  if (!p || cus < 0 || cus > 128) return fail(RPSF_E_BADARG, "reserved CUs must be 0..128");
  p->patch.reserved_cus = cus;
  return RPSF_OK;
}

// Confine the plan's own stream - and with it every launch the plan makes on it - to the compute units of `mask` (bit i of word i / 32:
// hipExtStreamCreateWithCUMask's numbering), and size its persistent launches for that many.  With a second stream masked to the complement
// (rpsf_stream_create) a caller gets two partitions of the chip that cannot take each other's CUs: the persistent patch launch needs whole
// CUs, and small kernels dispatched beside it on an unmasked stream land on CUs its workgroups are waiting for (profiles/r05m).
extern "C" int rpsf_plan_set_cu_mask(rpsf_plan* p, const uint32_t* mask, int words) {
  if (!p || !mask || words <= 0) return fail(RPSF_E_BADARG, "bad argument");
  if (p->parent) return fail(RPSF_E_STATE, "a view runs on its parent's stream");
  int cus = 0;
  for (int i = 0; i < words; ++i) cus += __builtin_popcount(mask[i]);
  if (cus < 8) return fail(RPSF_E_BADARG, "the mask must leave the plan at least 8 compute units");
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipStreamSynchronize(p->stream));
  drop_bands(p);
  hipStream_t masked = nullptr;
  HIP_TRY(hipExtStreamCreateWithCUMask(&masked, (uint32_t)words, mask));
  if (p->generic && g_hipfft.set_stream(p->fft.plan.get(), masked) != 0) {
    (void)hipStreamDestroy(masked);
    return fail(RPSF_E_HIP, "hipfftSetStream failed");
  }
  (void)hipStreamDestroy(p->stream);
  p->stream = masked;
  p->busy_valid = false;
  if (p->cu_count > 0) p->patch.round_capacity = p->patch.round_capacity / p->cu_count * cus;
  p->cu_count = cus;
  return RPSF_OK;
}

extern "C" int rpsf_stream_create(int device, const uint32_t* mask, int words, void** stream) {
  if (!stream) return fail(RPSF_E_BADARG, "null argument");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  if (mask && words > 0)
    HIP_TRY(hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask));
  else
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  *stream = st;
  return RPSF_OK;
}
extern "C" int rpsf_stream_destroy(void* stream) {
  if (stream) HIP_TRY(hipStreamDestroy(reinterpret_cast<hipStream_t>(stream)));
  return RPSF_OK;
}

extern "C" int rpsf_plan_set_image_prefetch(rpsf_plan* p, int on) {
  if (!p) return fail(RPSF_E_BADARG, "null plan");
  p->patch.prefetch = on != 0;
  return RPSF_OK;
}

extern "C" int rpsf_plan_set_stagger(rpsf_plan* p, int microseconds) {
  if (!p || microseconds < 0 || microseconds > 1000) return fail(RPSF_E_BADARG, "stagger must be 0..1000 us");
  p->patch.stagger_us = microseconds;
  drop_bands(p);
  return RPSF_OK;
}


extern "C" int rpsf_apply_device(rpsf_plan* p, const void* image_dev, void* out_dev, const rpsf_geometry* geom,
                                 void* stream) {
  if (!p || !image_dev || !out_dev) return fail(RPSF_E_BADARG, "null argument");
  if (!p->have_k) return fail(RPSF_E_STATE, "no transfer kernel installed (call rpsf_plan_set_transfer first)");
  int rc = check_geometry(p, geom);
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : p->stream;
  return launch_apply(p, reinterpret_cast<const float*>(image_dev), reinterpret_cast<float*>(out_dev), *geom, st, nullptr);
}


// Frames per launch group: the colour planes take 16 bytes per output pixel per frame in flight; keep
// them under a quarter of the device memory.  (One frame is one group: nothing is asked of the device.)
static int batch_group_frames(const rpsf_plan* p, const rpsf_geometry& g, int n_frames) {
  if (n_frames == 1 || p->generic || overlap_kind(p) == OV_ATOMIC || overlap_kind(p) == OV_SWEEP) return n_frames;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) total_b = (size_t)64 << 30;
  const size_t per_frame = 16 * plane_floats_needed(g);
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)n_frames, (total_b / 4) / per_frame));
}

static int check_batch(rpsf_plan* p, const void* a, const void* b, int n_frames, size_t im_stride, size_t out_stride,
                       const rpsf_geometry* geom) {
  if (!p || !a || !b) return fail(RPSF_E_BADARG, "null argument");
  if (n_frames <= 0) return fail(RPSF_E_BADARG, "n_frames must be positive");
  if (!p->have_k) return fail(RPSF_E_STATE, "no transfer kernel installed (call rpsf_plan_set_transfer first)");
  int rc = check_geometry(p, geom);
  if (rc != RPSF_OK) return rc;
  if (n_frames > 1 && (im_stride < (size_t)(geom->image_rows - 1) * geom->ld_image + geom->width ||
                       out_stride < (size_t)(geom->out_rows - 1) * geom->ld_out + geom->width))
    return fail(RPSF_E_BADARG, "frame stride smaller than one frame");
  return RPSF_OK;
}

static int launch_batch(rpsf_plan* p, const float* d_imgs, float* d_outs, int n_frames, size_t im_stride, size_t out_stride,
                        const rpsf_geometry& g, hipStream_t st, hipEvent_t ev_k0 = nullptr, hipEvent_t ev_k1 = nullptr) {
  const int group = batch_group_frames(p, g, n_frames);
  for (int f0 = 0; f0 < n_frames; f0 += group) {
    Batch b;
    b.frames = std::min(group, n_frames - f0), b.im_stride = im_stride, b.out_stride = out_stride;
    const bool first = f0 == 0, last = f0 + group >= n_frames;
    // (with several groups the kernel-time bracket covers everything between the first group's patch launch
    //  and the last group's, plane sums of the earlier groups included)
    int rc = launch_apply(p, d_imgs + (size_t)f0 * im_stride, d_outs + (size_t)f0 * out_stride, g, st,
                          first ? ev_k0 : nullptr, last ? ev_k1 : nullptr, b);
    if (rc != RPSF_OK) return rc;
  }
  return RPSF_OK;
}

extern "C" int rpsf_apply_batch_device(rpsf_plan* p, const void* images_dev, void* outs_dev, int n_frames,
                                       size_t image_stride, size_t out_stride, const rpsf_geometry* geom, void* stream) {
  int rc = check_batch(p, images_dev, outs_dev, n_frames, image_stride, out_stride, geom);
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : p->stream;
  return launch_batch(p, reinterpret_cast<const float*>(images_dev), reinterpret_cast<float*>(outs_dev), n_frames,
                      image_stride, out_stride, *geom, st);
}

// `iters` applies BACK TO BACK on the plan's stream, each bracketed by its own events (four per iteration, created here and destroyed on
// return), one synchronisation at the end: the launches queue up behind one another exactly as in a caller's loop, so the event times are
// those of the loop's kernels (with a host synchronisation after every apply, as until round 4, every launch started on an idle device
// and read 2 % longer than the wall-clock step that contains it).  total_ms[i]: the whole apply i, kernel_ms[i]: its patch-kernel launches.
template <class Launch>
static int timed_loop(rpsf_plan* p, int iters, float* total_ms, float* kernel_ms, Launch&& launch) {
  std::vector<hipEvent_t> ev((size_t)4 * iters, nullptr);
  auto cleanup = [&] {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  };
  int rc = RPSF_OK;
  hipError_t err = hipSuccess;
  for (auto& e : ev)
    if (err == hipSuccess) err = hipEventCreate(&e);
  for (int i = 0; i < iters && err == hipSuccess && rc == RPSF_OK; ++i) {
    err = hipEventRecord(ev[4 * i], p->stream);
    if (err == hipSuccess) rc = launch(ev[4 * i + 1], ev[4 * i + 2]);
    if (err == hipSuccess && rc == RPSF_OK) err = hipEventRecord(ev[4 * i + 3], p->stream);
  }
  if (err == hipSuccess && rc == RPSF_OK) err = hipStreamSynchronize(p->stream);
  for (int i = 0; i < iters && err == hipSuccess && rc == RPSF_OK; ++i) {
    float ms = 0.f;
    if (total_ms) {
      err = hipEventElapsedTime(&ms, ev[4 * i], ev[4 * i + 3]);
      total_ms[i] = ms;
    }
    if (kernel_ms && err == hipSuccess) {
      err = hipEventElapsedTime(&ms, ev[4 * i + 1], ev[4 * i + 2]);
      kernel_ms[i] = ms;
    }
  }
  if (err != hipSuccess || rc != RPSF_OK) (void)hipStreamSynchronize(p->stream);
  cleanup();
  if (rc != RPSF_OK) return rc;
  if (err != hipSuccess) return fail(RPSF_E_HIP, std::string("timed applies: ") + hipGetErrorString(err));
  return RPSF_OK;
}

extern "C" int rpsf_apply_batch_device_timed(rpsf_plan* p, const void* images_dev, void* outs_dev, int n_frames,
                                             size_t image_stride, size_t out_stride, const rpsf_geometry* geom, int iters,
                                             float* total_ms, float* kernel_ms) {
  if (iters <= 0) return fail(RPSF_E_BADARG, "bad argument");
  int rc = check_batch(p, images_dev, outs_dev, n_frames, image_stride, out_stride, geom);
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  return timed_loop(p, iters, total_ms, kernel_ms, [&](hipEvent_t k0, hipEvent_t k1) {
    return launch_batch(p, reinterpret_cast<const float*>(images_dev), reinterpret_cast<float*>(outs_dev), n_frames, image_stride,
                        out_stride, *geom, p->stream, k0, k1);
  });
}

// ------------------------------------------------------------------------------------------------
// Host arrays in, host arrays out (what ArrayPSFTransform.apply hands over and gets back: transform.py:117 astype on the
// way in, :174-177 a float64 result on the way out).  Nothing below creates a thread or allocates per call once a plan
// has seen its frame size: conversions run on the persistent pool, staging lives in the plan's HostPipe.
// ------------------------------------------------------------------------------------------------
using rpsf_host::HostPipe;
using rpsf_host::HostPool;

static int pipe_ensure(rpsf_plan* p, size_t slot_floats, int depth) {
  if (!p->pipe) p->pipe.reset(new HostPipe);
  HostPipe& q = *p->pipe;
  if (!q.st_in) {
    HIP_TRY(hipStreamCreateWithFlags(&q.st_in, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&q.st_out, hipStreamNonBlocking));
    for (auto* evs : {q.ev_in, q.ev_k, q.ev_out})
      for (int s = 0; s < HostPipe::MAX_DEPTH; ++s) HIP_TRY(hipEventCreateWithFlags(&evs[s], hipEventDisableTiming));
    for (auto& e : q.ev_chunk) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto* evs : {q.ev_band_in, q.ev_band_k})
      for (int s = 0; s < HostPipe::MAX_BANDS; ++s) HIP_TRY(hipEventCreateWithFlags(&evs[s], hipEventDisableTiming));
  }
  if (slot_floats <= q.slot_floats && depth <= q.depth) return RPSF_OK;
  // grow (every host entry point drains its own work before it returns: nothing is in flight on these buffers)
  const size_t want = std::max(slot_floats, q.slot_floats);
  const int d = std::max(depth, q.depth);
  HIP_TRY(hipStreamSynchronize(p->stream));
  q.release_buffers();
  for (int s = 0; s < d; ++s) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&q.h_in[s]), want * sizeof(float), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&q.h_out[s]), want * sizeof(float), hipHostMallocDefault));
    HIP_TRY(hipMalloc(&q.d_in[s], want * sizeof(float)));
    HIP_TRY(hipMalloc(&q.d_out[s], want * sizeof(float)));
  }
  q.depth = d, q.slot_floats = want;
  return RPSF_OK;
}

// Parts of one pool job over `bytes` of staging: a few per thread, so that a thread on a slow core (or the caller's, which may
// sit on the other socket) simply takes fewer of them; at least 128 KiB each
static int host_parts_for(size_t bytes) {
  return (int)std::min<size_t>((size_t)HostPool::get().width() * 4, std::max<size_t>(1, bytes >> 17));
}

// Frames the caller keeps in page-locked memory (rpsf_host_alloc, or memory registered with hipHostRegister) need no staging when no dtype
// conversion is due: the copy engines read / write them directly and the host touches no pixel.
static bool is_pinned_host(const void* ptr) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, ptr) != hipSuccess) {
    (void)hipGetLastError();  // (an ordinary pageable pointer is "invalid value" to the runtime: not an error of ours)
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}
static bool all_pinned(const void* const* ptrs, int n) {
  for (int i = 0; i < n; ++i)
    if (!is_pinned_host(ptrs[i])) return false;
  return true;
}

// The sweep kernel bounds every wait of a job for its predecessors (a protocol error must not hang the GPU) and reports a wait that ran out through a
// page-locked word; every entry point that has just waited for the plan's work looks at it, so such an apply fails instead of returning a wrong image.
static int sweep_check(rpsf_plan* p) {
  volatile uint32_t* word = owner(p)->sweep.err;
  if (!word || *word == 0) return RPSF_OK;
  *word = 0;
  return fail(RPSF_E_HIP, "sweep kernel: a job waited for the jobs it follows beyond the bound (internal protocol error; the output of this apply is not valid)");
}

static int drain_after_error(rpsf_plan* p, hipError_t err, const char* where) {
  (void)hipStreamSynchronize(p->pipe->st_in);
  (void)hipStreamSynchronize(p->stream);
  (void)hipStreamSynchronize(p->pipe->st_out);
  if (err == hipErrorUnknown && !g_err.empty()) return RPSF_E_HIP;  // launch_apply already set the message
  return fail(RPSF_E_HIP, std::string(where) + ": " + hipGetErrorString(err));
}

// Row bands of one large host frame: the lattice rows are cut into `want` groups; band b owns the output rows from its first lattice
// row to the next band's and runs every patch that reaches into them - its own lattice rows and the one above, which both neighbours
// compute (the collective-free seam of regularizepsf_amd/sharding.py, on one GPU) - as a view of the plan.  A band can run as soon as the
// image rows its patches read are on the device, and its rows can leave while the next band is still arriving: upload, patches and download
// of one frame overlap.  Returns the number of bands (0: this plan / frame is not cut - the caller takes the whole-frame path).
static int ensure_bands(rpsf_plan* p, const rpsf_geometry& g, int want) {
  if (p->bands_h == g.height && p->bands_w == g.width && p->bands_mode == g.pad_mode && p->bands_want == want) return (int)p->bands.size();
  drop_bands(p);
  p->bands_h = g.height, p->bands_w = g.width, p->bands_mode = g.pad_mode, p->bands_want = want;  // (remembered also when the answer is "no bands")
  if (p->generic || p->parent || !p->lattice || (overlap_kind(p) != OV_PLANES && overlap_kind(p) != OV_SWEEP) || g.pad_mode == RPSF_PAD_WRAP || want < 2) return 0;
  RowBands cuts;
  const int B = row_bands(p->N, p->n_patches, p->h_coords.data(), g.height, want, (int)HostPipe::MAX_BANDS, cuts);
  std::vector<std::unique_ptr<rpsf_plan>> bands;
  for (int b = 0; b < B; ++b) {
    std::vector<int32_t> coords;
    for (const int32_t i : cuts.patches[b]) coords.push_back(p->h_coords[2 * i]), coords.push_back(p->h_coords[2 * i + 1]);
    rpsf_plan* view = nullptr;
    if (plan_create_impl(&view, p->device, p->N, (int)cuts.patches[b].size(), coords.data(), p, cuts.patches[b].data()) != RPSF_OK) return 0;
    bands.emplace_back(view);
  }
  if (B) p->bands = std::move(bands), p->band_rows = std::move(cuts.cut), p->band_in_rows = std::move(cuts.in_rows);
  return B;
}

// One large frame in row bands, ONE pool job for both directions.  The workers stage the input piece by piece in row order (256 KiB
// pieces, claimed with fetch_add: no barrier between chunks, so the sixteen of them stream at the rate scripts/micro/host_copy.hip measures
// instead of the 78 GB/s of a job per 4 MiB chunk) and count finished pieces per chunk; the calling thread watches the counters, enqueues
// a chunk's H2D the moment it is complete, launches a band behind the chunk that completes the rows it reads, enqueues the band's D2H
// in pieces, polls the pieces' events and publishes each landed piece to the same workers, which widen it into the caller's array once
// no staging piece is left.  Widening of band 0 therefore runs while the last chunks are still going in (round 5 staged everything, then
// widened: "staged 1.0" + "out: waits 0.5 + conversions 0.9" one after the other, profiles/r05l_host_frame_row_bands.log).
static int host_one_frame_banded(rpsf_plan* p, const void* image, int in_f64, void* out, int out_f64, const rpsf_geometry& g, int B,
                                 bool direct_in, bool direct_out) {
  HostPipe& q = *p->pipe;
  HostPool& pool = HostPool::get(p->device);
  const int W = g.width, H = g.height;
  const size_t count = (size_t)H * W, bytes = count * sizeof(float);
  constexpr size_t PIECE = (size_t)1 << 16;                      // floats per unit of work of a worker
  static const bool trace = dev_env("RPSF_HOST_TRACE") != nullptr;
  static const int frame_every = dev_env("RPSF_FRAME_EVERY") ? std::atoi(dev_env("RPSF_FRAME_EVERY")) : 0;
  static const int frame_workers = dev_env("RPSF_FRAME_WORKERS") ? std::atoi(dev_env("RPSF_FRAME_WORKERS")) : 0;
  const auto t_start = std::chrono::steady_clock::now();
  auto ms_since = [&](std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  struct Range {
    size_t lo, hi;
  };
  // input pieces: chunk by chunk, in row order
  std::vector<Range> in_pieces;
  std::vector<int> piece_chunk, chunk_pieces;
  std::vector<Range> chunks;
  // One upload per band - the rows it reads beyond the band before it - because every copy on a stream costs about 10 us of dead time
  // before the next one starts (sixteen 4 MiB uploads: 45 GB/s against the 57 GB/s of one copy, profiles/r06v_host_frame_timeline.txt); a
  // staged frame sends the first band's rows in four copies, so that the first one leaves when a sixteenth of the band is staged.
  std::vector<int> cuts{0};
  for (int b = 0; b < B; ++b) {
    const int hi = b + 1 == B ? H : p->band_in_rows[b], lo = cuts.back();
    if (hi <= lo) continue;
    if (b == 0 && !direct_in)
      for (int part = 1; part < 4; ++part) cuts.push_back(lo + (int)((long)(hi - lo) * part / 4));
    cuts.push_back(hi);
  }
  for (size_t i = 0; i + 1 < cuts.size(); ++i) {
    const size_t lo = (size_t)cuts[i] * W, hi = (size_t)cuts[i + 1] * W;
    if (hi <= lo) continue;
    int n = 0;
    for (size_t a = lo; a < hi && !direct_in; a += PIECE, ++n) in_pieces.push_back({a, std::min(hi, a + PIECE)}), piece_chunk.push_back((int)chunks.size());
    chunks.push_back({lo, hi}), chunk_pieces.push_back(n);
  }
  std::vector<std::atomic<int>> chunk_done(chunks.size());
  for (auto& c : chunk_done) c.store(0, std::memory_order_relaxed);
  // output pieces: appended by the calling thread as D2H pieces land (storage reserved up front: the workers index it while it grows)
  std::vector<Range> out_pieces(direct_out ? 0 : count / PIECE + HostPipe::MAX_PIECES + 2);
  std::atomic<size_t> next_in{0}, next_out{0}, out_avail{0};
  std::atomic<int> closed{0};
  const size_t n_in = in_pieces.size();
  auto worker = [&](int) {
    for (;;) {
      if (next_in.load(std::memory_order_relaxed) < n_in) {
        const size_t i = next_in.fetch_add(1, std::memory_order_relaxed);
        if (i < n_in) {
          rpsf_host::narrow_or_copy(q.h_in[0], image, in_f64 != 0, in_pieces[i].lo, in_pieces[i].hi);
          chunk_done[piece_chunk[i]].fetch_add(1, std::memory_order_release);
          continue;
        }
      }
      size_t o = next_out.load(std::memory_order_relaxed);
      if (o < out_avail.load(std::memory_order_acquire)) {
        if (next_out.compare_exchange_weak(o, o + 1, std::memory_order_relaxed))
          rpsf_host::widen_or_copy(out, out_f64 != 0, q.h_out[0], out_pieces[o].lo, out_pieces[o].hi);
        continue;
      }
      if (closed.load(std::memory_order_acquire) && next_out.load(std::memory_order_relaxed) >= out_avail.load(std::memory_order_acquire)) return;
      __builtin_ia32_pause();
    }
  };
  hipError_t err = hipSuccess;
  const bool inline_mode = pool.width() < 2;  // (HostPool::run with one part runs `meanwhile` BEFORE the part: the conductor would wait for staging that has not begun)
  std::vector<Range> landed;  // D2H pieces in the order they were enqueued; event c is q.ev_chunk[c]
  double t_enqueued = 0.0, t_first_out = 0.0, t_last_out = 0.0;
  auto conductor = [&] {
    size_t c = 0, published = 0, n_avail = 0;
    int next_band = 0;
    while (err == hipSuccess && (c < chunks.size() || published < landed.size())) {
      bool progress = false;
      if (c < chunks.size() && (direct_in || chunk_done[c].load(std::memory_order_acquire) == chunk_pieces[c])) {
        const size_t lo = chunks[c].lo, hi = chunks[c].hi;
        const int r1 = (int)(hi / W);
        err = hipMemcpyAsync(q.d_in[0] + lo, (direct_in ? static_cast<const float*>(image) : q.h_in[0]) + lo, (hi - lo) * sizeof(float),
                             hipMemcpyHostToDevice, q.st_in);
        while (err == hipSuccess && next_band < B && p->band_in_rows[next_band] <= r1) {
          const int b = next_band++;
          const int R0 = p->band_rows[b], R1 = p->band_rows[b + 1];
          rpsf_geometry gb = g;
          gb.out_row0 = R0, gb.out_rows = R1 - R0;
          err = hipEventRecord(q.ev_band_in[b], q.st_in);
          if (err == hipSuccess) err = hipStreamWaitEvent(p->stream, q.ev_band_in[b], 0);
          float* const host_out = direct_out ? static_cast<float*>(out) : q.h_out[0];
          if (err == hipSuccess && launch_apply(p->bands[b].get(), q.d_in[0], q.d_out[0] + (size_t)R0 * W, gb, p->stream, nullptr) != RPSF_OK)
            err = hipErrorUnknown;
          if (err == hipSuccess) err = hipEventRecord(q.ev_band_k[b], p->stream);
          // (one download stream: a second one for every other band - to hide the 20 us between two copies of a stream - made the frame 8 % slower,
          // and letting the band's kernel write the page-locked rows itself instead of a download 5 %: profiles/r06y, r06z_host_frame_knobs.log)
          const hipStream_t so = q.st_out;
          if (err == hipSuccess) err = hipStreamWaitEvent(so, q.ev_band_k[b], 0);
          // one download per band; the last band of a frame that is widened afterwards in four, so that only a quarter of it is left
          // to widen when the last byte has landed
          const int sub = (b + 1 == B && !direct_out) ? 4 : 1;
          const int rows_per_piece = (R1 - R0 + sub - 1) / sub;
          for (int s0 = R0; s0 < R1 && err == hipSuccess; s0 += rows_per_piece) {
            const size_t plo = (size_t)s0 * W, phi = (size_t)std::min(R1, s0 + rows_per_piece) * W;
            err = hipMemcpyAsync(host_out + plo, q.d_out[0] + plo, (phi - plo) * sizeof(float), hipMemcpyDeviceToHost, so);
            if (err == hipSuccess) err = hipEventRecord(q.ev_chunk[landed.size()], so);
            landed.push_back({plo, phi});
          }
        }
        if (++c == chunks.size()) t_enqueued = ms_since(t_start);
        progress = true;
      }
      if (err == hipSuccess && published < landed.size()) {
        // (while chunks are still to go in: a look; afterwards: a wait - nothing else is left for this thread to do)
        const hipError_t qe = c < chunks.size() ? hipEventQuery(q.ev_chunk[published]) : hipEventSynchronize(q.ev_chunk[published]);
        if (qe == hipSuccess) {
          if (published == 0) t_first_out = ms_since(t_start);
          if (!direct_out && inline_mode) {  // (no workers: this thread widens the piece itself)
            rpsf_host::widen_or_copy(out, out_f64 != 0, q.h_out[0], landed[published].lo, landed[published].hi);
          } else if (!direct_out) {
            for (size_t a = landed[published].lo; a < landed[published].hi; a += PIECE) out_pieces[n_avail++] = {a, std::min(landed[published].hi, a + PIECE)};
            out_avail.store(n_avail, std::memory_order_release);
          }
          ++published, progress = true;
        } else if (qe != hipErrorNotReady) {
          err = qe;
        }
      }
      if (!progress) __builtin_ia32_pause();
    }
    t_last_out = ms_since(t_start);
    closed.store(1, std::memory_order_release);
  };
  if (direct_in && direct_out) conductor();  // nothing for the pool: the copy engines read and write the caller's pages
  else if (inline_mode) {  // RPSF_HOST_THREADS=1: no workers - stage everything, then conduct and widen on this thread (no overlap of the host's own steps)
    for (size_t i = 0; i < n_in; ++i) {
      rpsf_host::narrow_or_copy(q.h_in[0], image, in_f64 != 0, in_pieces[i].lo, in_pieces[i].hi);
      chunk_done[piece_chunk[i]].fetch_add(1, std::memory_order_release);
    }
    conductor();
  } else {
    // every second worker (one per CCD at the default width): sixteen threads streaming beside the copy engines slow the copies down more than they
    // gain (H2D busy 1.78 ms of a 67 MB frame with 16 workers, 1.48 with 8, 1.28 with 4 - which then cannot keep up: profiles/r06x_host_frame_matrix.log)
    const int every = frame_every > 0 ? frame_every : (pool.width() >= 16 ? 2 : 1);
    pool.run(std::max(1, (frame_workers > 0 ? std::min(frame_workers, pool.width()) : pool.width()) / every), worker, conductor, every);
  }
  if (trace)
    std::fprintf(stderr, "[rpsf host frame] %zu chunks, %d bands, %zu + %zu pieces: last chunk enqueued %.3f ms, first piece back %.3f, last %.3f, total %.3f ms\\n",
                 chunks.size(), B, n_in, (size_t)out_avail.load(), t_enqueued, t_first_out, t_last_out, ms_since(t_start));
  if (err != hipSuccess) return drain_after_error(p, err, "host frame");
  return sweep_check(p);
}

// One frame.  The conversions run chunk by chunk (>= 4 MiB) on the pool, each chunk's H2D copy starts as soon as it is staged,
// and on the way back each chunk is widened as soon as it has landed: conversion and PCIe overlap inside the frame.
static int host_one_frame(rpsf_plan* p, const void* image, int in_f64, void* out, int out_f64, const rpsf_geometry& g) {
  const size_t count = (size_t)g.height * g.width, bytes = count * sizeof(float);
  int rc = pipe_ensure(p, count, 1);
  if (rc != RPSF_OK) return rc;
  HostPipe& q = *p->pipe;
  HostPool& pool = HostPool::get(p->device);
  const int T = host_parts_for(bytes / std::max<size_t>(1, std::min<size_t>(HostPipe::MAX_CHUNKS, std::max<size_t>(1, bytes >> 22))));
  const int n_chunks = (int)std::min<size_t>(HostPipe::MAX_CHUNKS, std::max<size_t>(1, bytes >> 22));
  const size_t per_chunk = ((count + n_chunks - 1) / n_chunks + 1023) & ~(size_t)1023;
  auto chunk_range = [&](int c, size_t& lo, size_t& hi) { lo = std::min(count, c * per_chunk), hi = std::min(count, lo + per_chunk); };
  hipError_t err = hipSuccess;
  static const bool trace = dev_env("RPSF_HOST_TRACE") != nullptr;  // development: where a host frame's milliseconds go (stderr)
  const auto t_start = std::chrono::steady_clock::now();
  auto ms_since = [&](std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  double t_conv_in = 0.0, t_conv_out = 0.0, t_wait_out = 0.0;
  const bool direct_in = !in_f64 && is_pinned_host(image), direct_out = !out_f64 && is_pinned_host(out);
  // Large frames are cut into row bands (views of this plan) so that the upload of band b + 1, the patches of band b and the download of
  // band b - 1 overlap (RPSF_HOST_BANDS=0: off, =n: that many).
  // (a band per 8 MiB, at most eight: 4096^2 end to end 2.30 / 2.21 / 2.20 ms at 4 / 6 / 8 bands, page-locked 1.83 / 1.80 / 1.79, profiles/r06w_host_bands.log)
  int want_bands = bytes >= ((size_t)24 << 20) ? (int)std::min<size_t>(8, bytes >> 23) : 0;
  if (p->host_bands_opt >= 0) want_bands = p->host_bands_opt;  // (RPSF_OPT_HOST_BANDS)
  const int B = ensure_bands(p, g, want_bands);
  p->last_host_bands = B;
  struct OutChunk {
    size_t lo, hi;
  };
  std::vector<OutChunk> out_chunks;  // in the order their download was enqueued; event c is q.ev_chunk[c]
  if (B >= 2) return host_one_frame_banded(p, image, in_f64, out, out_f64, g, B, direct_in, direct_out);
  {
  // (a frame of one chunk - under 8 MiB - has nothing to overlap with itself: everything on the plan's stream, no events to tie three together;
  // 512^2: 0.179 -> see profiles/r05v)
  const bool one_stream = n_chunks == 1;
  const hipStream_t s_in = one_stream ? p->stream : q.st_in, s_out = one_stream ? p->stream : q.st_out;
  if (direct_in) err = hipMemcpyAsync(q.d_in[0], image, bytes, hipMemcpyHostToDevice, s_in);
  for (int c = 0; c < n_chunks && err == hipSuccess && !direct_in; ++c) {
    size_t lo, hi;
    chunk_range(c, lo, hi);
    const auto t0 = std::chrono::steady_clock::now();
    pool.run(T, [&](int t) {
      size_t a, b;
      rpsf_host::split_range(lo, hi, t, T, a, b);
      rpsf_host::narrow_or_copy(q.h_in[0], image, in_f64 != 0, a, b);
    });
    t_conv_in += ms_since(t0);
    if (hi > lo) err = hipMemcpyAsync(q.d_in[0] + lo, q.h_in[0] + lo, (hi - lo) * sizeof(float), hipMemcpyHostToDevice, s_in);
  }
  if (!one_stream) {
    if (err == hipSuccess) err = hipEventRecord(q.ev_in[0], s_in);
    if (err == hipSuccess) err = hipStreamWaitEvent(p->stream, q.ev_in[0], 0);
  }
  // A small frame through the sweep kernel: the kernel's one store per output pixel goes straight to the page-locked result rows (the staging buffer, or
  // the caller's own page-locked array) - no download behind the launch, whose start-up and 1 MiB are a fifth of such a frame's time (512^2 / 64:
  // 0.140 -> see profiles/r06zu_small_frame_zero_copy_out.log).  Only where every pixel of the window is written by the launch (the lattice covers it).
  float* zc_out = nullptr;
  if (one_stream && err == hipSuccess && overlap_kind(p) == OV_SWEEP && p->sweep.ok && !dev_env("RPSF_NO_ZC_OUT")) {
    void* dev = nullptr;
    if (lattice_covers_window(p, g) && hipHostGetDevicePointer(&dev, direct_out ? out : static_cast<void*>(q.h_out[0]), 0) == hipSuccess) zc_out = static_cast<float*>(dev);
    else (void)hipGetLastError();
  }
  if (err == hipSuccess && launch_apply(p, q.d_in[0], zc_out ? zc_out : q.d_out[0], g, p->stream, nullptr) != RPSF_OK) err = hipErrorUnknown;
  if (zc_out && err == hipSuccess) {
    err = hipEventRecord(q.ev_chunk[0], p->stream);
    out_chunks.push_back({0, count});
  }
  if (!one_stream || trace) {
    if (err == hipSuccess) err = hipEventRecord(q.ev_k[0], p->stream);
    if (err == hipSuccess && !one_stream) err = hipStreamWaitEvent(s_out, q.ev_k[0], 0);
    if (err == hipSuccess && one_stream) err = hipEventRecord(q.ev_in[0], p->stream);  // (trace only)
  }
  if (direct_out && !zc_out && err == hipSuccess) {
    err = hipMemcpyAsync(out, q.d_out[0], bytes, hipMemcpyDeviceToHost, s_out);
    if (err == hipSuccess) err = hipEventRecord(q.ev_chunk[0], s_out);
    out_chunks.push_back({0, count});
  }
  for (int c = 0; c < n_chunks && err == hipSuccess && !direct_out && !zc_out; ++c) {
    size_t lo, hi;
    chunk_range(c, lo, hi);
    if (hi > lo) err = hipMemcpyAsync(q.h_out[0] + lo, q.d_out[0] + lo, (hi - lo) * sizeof(float), hipMemcpyDeviceToHost, s_out);
    if (err == hipSuccess) err = hipEventRecord(q.ev_chunk[out_chunks.size()], s_out);
    out_chunks.push_back({lo, hi});
  }
  }
  const double t_enqueued = ms_since(t_start);
  double t_in_done = 0.0, t_kernel_done = 0.0;
  if (trace && err == hipSuccess && B < 2) {
    (void)hipEventSynchronize(q.ev_in[0]);
    t_in_done = ms_since(t_start);
    (void)hipEventSynchronize(q.ev_k[0]);
    t_kernel_done = ms_since(t_start);
  }
  for (size_t c = 0; c < out_chunks.size() && err == hipSuccess; ++c) {
    auto t0 = std::chrono::steady_clock::now();
    err = hipEventSynchronize(q.ev_chunk[c]);
    t_wait_out += ms_since(t0);
    if (err != hipSuccess || direct_out) continue;
    const size_t lo = out_chunks[c].lo, hi = out_chunks[c].hi;
    t0 = std::chrono::steady_clock::now();
    pool.run(T, [&](int t) {
      size_t a, b;
      rpsf_host::split_range(lo, hi, t, T, a, b);
      rpsf_host::widen_or_copy(out, out_f64 != 0, q.h_out[0], a, b);
    });
    t_conv_out += ms_since(t0);
  }
  if (trace)
    std::fprintf(stderr, "[rpsf host frame] %d chunks x %d parts, %d bands: staged+enqueued %.3f ms (conversions %.3f), H2D done %.3f, kernel done %.3f, "
                 "out: waits %.3f + conversions %.3f, total %.3f ms\n", n_chunks, T, B, t_enqueued, t_conv_in, t_in_done, t_kernel_done, t_wait_out,
                 t_conv_out, ms_since(t_start));
  if (err != hipSuccess) return drain_after_error(p, err, "host frame");
  return sweep_check(p);
}

// Frames per group of the streamed pipeline: small frames go through the shared-K batch launch a few at a time (the packed K is
// read once per group, and a launch / a copy of a few hundred KiB is all overhead: up to 32 frames or 16 MiB per group); from 16 MiB per
// frame on (2048^2), where a frame's copies take several times its kernel, one by one - a short batch then pays the shortest ramp.
static int stream_group_frames(size_t frame_bytes, int n_frames, int stream_group_opt) {
  int g = (int)std::max<size_t>(1, std::min<size_t>(32, ((size_t)16 << 20) / std::max<size_t>(1, frame_bytes)));
  if (stream_group_opt > 0) g = std::max(1, std::min(64, stream_group_opt));  // (RPSF_OPT_STREAM_GROUP)
  return std::min(g, n_frames);
}

// A sequence of frames of one geometry: `depth` groups in flight.  The calling thread stages group i (conversion on the pool),
// enqueues H2D(i) on the copy-in stream, the shared-K launch of the group on the plan's stream behind it, D2H(i) on the copy-out
// stream behind that, and - in the same pool job as the staging of the next group - widens whichever earlier group has landed.
// H2D of group i + 1, the kernel of group i and D2H of group i - 1 therefore run at the same time (PCIe is full duplex), and the
// host conversions of both directions share the pool.
static int host_frames(rpsf_plan* p, const void* const* images, int in_f64, void* const* outs, int out_f64, int n_frames,
                       const rpsf_geometry& g) {
  if (n_frames == 1) return host_one_frame(p, images[0], in_f64, outs[0], out_f64, g);
  const size_t count = (size_t)g.height * g.width, bytes = count * sizeof(float);
  // Groups: `first[i]` ... `first[i + 1]` are the frames of group i.  Small frames: equal groups.  Frames that go one by one (16 MiB and more) go two
  // by two in the MIDDLE of a long sequence - a staging job and an enqueue per two frames instead of per frame: 32 x 2048^2 float32 0.473 -> 0.415 ms
  // per frame - while the first and the last groups stay single frames, so that the ramps (the first upload, the last download) stay short
  // (groups of two throughout cost an 8-frame batch 0.48 -> 0.57 ms per frame; profiles/r05y).  RPSF_OPT_STREAM_GROUP fixes one size for all.
  const int G0 = stream_group_frames(bytes, n_frames, p->stream_group_opt);
  std::vector<int> first{0};
  {
    const bool pinned_size = p->stream_group_opt > 0;
    int pairs_from = 12;
    if (const char* e = dev_env("RPSF_STREAM_PAIRS_FROM")) pairs_from = std::max(4, std::atoi(e));  // development sweeps
    const bool pairs = !pinned_size && G0 == 1 && n_frames >= pairs_from && bytes * 2 <= ((size_t)128 << 20);
    while (first.back() < n_frames) {
      const int at = first.back(), left = n_frames - at;
      const int size = pairs ? ((at >= 2 && left >= 4) ? 2 : 1) : G0;
      first.push_back(at + std::min(size, left));
    }
  }
  const int n_groups = (int)first.size() - 1;
  int G = 1;
  for (int i = 0; i < n_groups; ++i) G = std::max(G, first[i + 1] - first[i]);
  int depth = bytes * G >= ((size_t)128 << 20) ? 3 : HostPipe::MAX_DEPTH;
  if (p->stream_depth_opt > 0) depth = std::max(1, std::min((int)HostPipe::MAX_DEPTH, p->stream_depth_opt));  // (RPSF_OPT_STREAM_DEPTH)
  depth = std::min(depth, n_groups);
  int rc = pipe_ensure(p, count * G, depth);
  if (rc != RPSF_OK) return rc;
  HostPipe& q = *p->pipe;
  HostPool& pool = HostPool::get(p->device);
  const int T = host_parts_for(bytes * G);  // (a job stages / unstages a whole group: small frames still give every worker a part)
  auto frames_of = [&](int grp) { return first[grp + 1] - first[grp]; };
  const bool direct_in = !in_f64 && all_pinned(images, n_frames);
  const bool direct_out = !out_f64 && all_pinned(const_cast<const void* const*>(outs), n_frames);
  hipError_t err = hipSuccess;
  int next_in = 0, next_out = 0;
  static const bool trace = dev_env("RPSF_HOST_TRACE") != nullptr;  // development: where the host's time goes (stderr)
  double t_jobs = 0.0, t_enqueue = 0.0, t_wait = 0.0;
  const auto t_start = std::chrono::steady_clock::now();
  auto ms_since = [&](std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  // enqueue group `grp` (staged in slot grp % depth): H2D -> shared-K launch -> D2H on the three streams
  auto enqueue = [&](int grp) {
    const int sg = grp % depth, fg = frames_of(grp);
    const size_t gb = (size_t)fg * bytes;
    if (direct_in) {
      for (int f = 0; f < fg && err == hipSuccess; ++f)
        err = hipMemcpyAsync(q.d_in[sg] + (size_t)f * count, images[first[grp] + f], bytes, hipMemcpyHostToDevice, q.st_in);
    } else {
      err = hipMemcpyAsync(q.d_in[sg], q.h_in[sg], gb, hipMemcpyHostToDevice, q.st_in);
    }
    if (err == hipSuccess) err = hipEventRecord(q.ev_in[sg], q.st_in);
    if (err == hipSuccess) err = hipStreamWaitEvent(p->stream, q.ev_in[sg], 0);
    if (err == hipSuccess && launch_batch(p, q.d_in[sg], q.d_out[sg], fg, count, count, g, p->stream) != RPSF_OK) err = hipErrorUnknown;
    if (err == hipSuccess) err = hipEventRecord(q.ev_k[sg], p->stream);
    if (err == hipSuccess) err = hipStreamWaitEvent(q.st_out, q.ev_k[sg], 0);
    if (direct_out) {
      for (int f = 0; f < fg && err == hipSuccess; ++f)
        err = hipMemcpyAsync(outs[first[grp] + f], q.d_out[sg] + (size_t)f * count, bytes, hipMemcpyDeviceToHost, q.st_out);
    } else if (err == hipSuccess) {
      err = hipMemcpyAsync(q.h_out[sg], q.d_out[sg], gb, hipMemcpyDeviceToHost, q.st_out);
    }
    if (err == hipSuccess) err = hipEventRecord(q.ev_out[sg], q.st_out);
  };
  int staged = -1, next_enq = 0;  // a group that is staged but not yet enqueued: its enqueue runs on this thread WHILE the workers do the next job
  while (next_out < n_groups && err == hipSuccess) {
    auto t_phase = std::chrono::steady_clock::now();
    const bool can_in = next_in < n_groups && next_in - next_out < depth;
    bool out_ready = false;
    if (next_out < next_enq) {
      const hipError_t qe = hipEventQuery(q.ev_out[next_out % depth]);
      if (qe == hipSuccess) out_ready = true;
      else if (qe != hipErrorNotReady) err = qe;
      if (err == hipSuccess && !out_ready && !can_in && staged < 0) {  // nothing to stage or enqueue: wait for the oldest group in flight
        err = hipEventSynchronize(q.ev_out[next_out % depth]);
        out_ready = err == hipSuccess;
      }
    }
    if (err != hipSuccess) break;
    t_wait += ms_since(t_phase), t_phase = std::chrono::steady_clock::now();
    const int si = next_in % depth, so = next_out % depth;
    const int fi = can_in ? frames_of(next_in) : 0, fo = out_ready ? frames_of(next_out) : 0;
    const int ci = direct_in ? 0 : fi, co = direct_out ? 0 : fo;  // frames this job stages / unstages
    const int to_enqueue = staged;
    double t_meanwhile = 0.0;
    pool.run(ci + co > 0 ? T : 0,
             [&](int t) {
               // the group's frames laid end to end, cut into T parts: a part covers a run of pixels that may span frames
               const size_t total_in = (size_t)ci * count, total_out = (size_t)co * count;
               size_t a, b;
               rpsf_host::split_range(0, total_in, t, T, a, b);
               while (a < b) {
                 const size_t f = a / count, lo = a % count, hi = std::min(count, lo + (b - a));
                 rpsf_host::narrow_or_copy(q.h_in[si] + f * count, images[first[next_in] + f], in_f64 != 0, lo, hi);
                 a += hi - lo;
               }
               rpsf_host::split_range(0, total_out, t, T, a, b);
               while (a < b) {
                 const size_t f = a / count, lo = a % count, hi = std::min(count, lo + (b - a));
                 rpsf_host::widen_or_copy(outs[first[next_out] + f], out_f64 != 0, q.h_out[so] + f * count, lo, hi);
                 a += hi - lo;
               }
             },
             [&] {
               if (to_enqueue >= 0) {
                 const auto t0 = std::chrono::steady_clock::now();
                 enqueue(to_enqueue);
                 t_meanwhile = ms_since(t0);
               }
             });
    if (to_enqueue >= 0) staged = -1, next_enq = to_enqueue + 1;
    t_enqueue += t_meanwhile;
    t_jobs += ms_since(t_phase) - t_meanwhile;
    if (can_in) staged = next_in++;
    if (out_ready) ++next_out;
  }
  if (trace)
    std::fprintf(stderr, "[rpsf streamed] %d frames in %d groups of up to %d, depth %d, %d parts per job: staging jobs %.3f ms, enqueues %.3f ms, waits %.3f ms, total %.3f ms\n",
                 n_frames, n_groups, G, depth, T, t_jobs, t_enqueue, t_wait, ms_since(t_start));
  if (err != hipSuccess) return drain_after_error(p, err, "streamed frames");
  return sweep_check(p);
}

static int check_host_call(rpsf_plan* p, const void* a, const void* b, int n_frames, int height, int width, int pad_mode, float pad_value,
                           rpsf_geometry* g) {
  if (!p || !a || !b) return fail(RPSF_E_BADARG, "null argument");
  if (n_frames <= 0) return fail(RPSF_E_BADARG, "n_frames must be positive");
  if (!p->have_k) return fail(RPSF_E_STATE, "no transfer kernel installed (call rpsf_plan_set_transfer first)");
  *g = rpsf_geometry{height, width, pad_mode, pad_value, 0, 0, 0, height, width, 0, height, width};
  int rc = check_geometry(p, g);
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  return RPSF_OK;
}

extern "C" int rpsf_apply_frames_host(rpsf_plan* p, const void* const* images_host, int image_is_f64, int n_frames, int height,
                                      int width, int pad_mode, float pad_value, void* const* outs_host, int out_is_f64) {
  rpsf_geometry g;
  int rc = check_host_call(p, images_host, outs_host, n_frames, height, width, pad_mode, pad_value, &g);
  if (rc != RPSF_OK) return rc;
  for (int f = 0; f < n_frames; ++f)
    if (!images_host[f] || !outs_host[f]) return fail(RPSF_E_BADARG, "null frame pointer");
  return host_frames(p, images_host, image_is_f64, outs_host, out_is_f64, n_frames, g);
}

extern "C" int rpsf_apply_batch_host(rpsf_plan* p, const void* images_host, int image_is_f64, int n_frames, int height, int width,
                                     int pad_mode, float pad_value, void* outs_host, int out_is_f64) {
  rpsf_geometry g;
  int rc = check_host_call(p, images_host, outs_host, n_frames, height, width, pad_mode, pad_value, &g);
  if (rc != RPSF_OK) return rc;
  const size_t count = (size_t)height * width;
  std::vector<const void*> in(n_frames);
  std::vector<void*> out(n_frames);
  for (int f = 0; f < n_frames; ++f) {
    in[f] = static_cast<const char*>(images_host) + (size_t)f * count * (image_is_f64 ? 8 : 4);
    out[f] = static_cast<char*>(outs_host) + (size_t)f * count * (out_is_f64 ? 8 : 4);
  }
  return host_frames(p, in.data(), image_is_f64, out.data(), out_is_f64, n_frames, g);
}

extern "C" int rpsf_apply_batch(rpsf_plan* p, const float* images_host, int n_frames, int height, int width, int pad_mode,
                                float pad_value, float* outs_host) {
  return rpsf_apply_batch_host(p, images_host, 0, n_frames, height, width, pad_mode, pad_value, outs_host, 0);
}

extern "C" int rpsf_apply_host(rpsf_plan* p, const void* image_host, int image_is_f64, int height, int width, int pad_mode,
                               float pad_value, void* out_host, int out_is_f64) {
  rpsf_geometry g;
  int rc = check_host_call(p, image_host, out_host, 1, height, width, pad_mode, pad_value, &g);
  if (rc != RPSF_OK) return rc;
  return host_one_frame(p, image_host, image_is_f64, out_host, out_is_f64, g);
}

extern "C" int rpsf_apply(rpsf_plan* p, const float* image_host, int height, int width, int pad_mode, float pad_value,
                          float* out_host) {
  return rpsf_apply_host(p, image_host, 0, height, width, pad_mode, pad_value, out_host, 0);
}

// Page-locked host memory for callers that keep their frames in it (acquisition buffers, result rings): float32 frames in such memory
// cross PCIe without the staging copy of the pageable path.
extern "C" int rpsf_host_alloc(int device, size_t bytes, void** out) {
  if (!out) return fail(RPSF_E_BADARG, "null argument");
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
  return RPSF_OK;
}
extern "C" int rpsf_host_free(void* ptr) {
  if (ptr) HIP_TRY(hipHostFree(ptr));
  return RPSF_OK;
}

// The NUMA node the device hangs off (-1: unknown / a single-node host): where a process that feeds this GPU from host arrays should
// run and allocate (the pool's workers are placed there by themselves).
extern "C" int rpsf_device_numa_node(int device, int* node) {
  if (!node) return fail(RPSF_E_BADARG, "null argument");
  *node = -1;
  char bdf[64] = {};
  HIP_TRY(hipDeviceGetPCIBusId(bdf, sizeof(bdf), device));
  for (char* c = bdf; *c; ++c) *c = (char)std::tolower(*c);
  const std::string path = std::string("/sys/bus/pci/devices/") + bdf + "/numa_node";
  if (FILE* f = std::fopen(path.c_str(), "r")) {
    if (std::fscanf(f, "%d", node) != 1) *node = -1;
    std::fclose(f);
  }
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------
// ArrayPSFTransform.apply with a finite saturation threshold, whole (regularizepsf/transform.py:117-138,171-177): float64 copy, np.pad by 2N
// (the mode's index map, evaluated here on the host), mask = padded > threshold, binary dilation with the cross element (`dilation` >= 1
// iterations = a diamond of that radius; scipy treats the outside as background), NaN, the sequential row-major nanmean fill, the correction of
// the PADDED frame on the GPU (corners shifted by 2N, constant padding: exactly what the reference's slices see), raw values restored on the mask,
// crop.  Everything the reference does on the host stays on the host and in its order; what changed against the NumPy / SciPy route of rounds 1-4
// is the cost: no np.pad / astype / copy temporaries (three passes over a (H + 4N)^2 float64 frame), no scipy.ndimage pass over the whole mask for
// a handful of pixels, no device allocation per call, only the rows the patches read and the rows the caller gets cross PCIe.
// A sequence of frames (rpsf_apply_frames_host_saturated - the reference's example corrects a list of frames this way, docs/source/example.ipynb
// cell 25) alternates between two staging slots: the host steps of frame i + 1 run while the GPU corrects frame i.
// ------------------------------------------------------------------------------------------------
// The correction of the 2N-padded frame of an H x W image: rows [r_lo, r_hi) of it are read, rows [o_lo, o_lo + o_rows) written
static int padded_geometry(const rpsf_plan* p, int H, int W, int* r_lo, int* r_hi, int* o_lo, int* o_rows, rpsf_geometry* g) {
  const int N = p->N;
  const long PH = (long)H + 4L * N, PW = (long)W + 4L * N;
  if (PH * PW >= ((long)1 << 31)) return fail(RPSF_E_UNSUPPORTED, "padded frame too large for this entry point");
  // rows of the padded frame the patches read, and the geometry of the correction on it (the hipFFT fallback takes whole frames only)
  *r_lo = p->generic ? 0 : (int)std::max<long>(0, 2L * N + std::min(0, p->corner_min[0]));
  *r_hi = p->generic ? (int)PH : (int)std::min<long>(PH, 2L * N + p->corner_max[0] + N);
  *o_lo = p->generic ? 0 : 2 * N, *o_rows = p->generic ? (int)PH : H;  // output rows the device hands back
  *g = rpsf_geometry{(int)PH, (int)PW, RPSF_PAD_CONSTANT, 0.f, 2 * N, 2 * N, *r_lo, *r_hi - *r_lo, (int)PW, *o_lo, *o_rows, (int)PW};
  return check_geometry(p, g);
}

struct SatRun {
  rpsf_plan* p;
  int H, W, N, pad_mode, dilation, width, in_f64, out_f64;
  double threshold;
  long PH, PW;
  int r_lo, r_hi, o_lo, o_rows;
  rpsf_geometry g;
  std::vector<int> colmap;

  int init(rpsf_plan* plan, int height, int w, int mode, double thr, int dil, int nbw, int image_is_f64, int out_is_f64, int slots) {
    p = plan, H = height, W = w, N = plan->N, pad_mode = mode, dilation = dil, width = nbw, in_f64 = image_is_f64, out_f64 = out_is_f64, threshold = thr;
    PH = (long)H + 4L * N, PW = (long)W + 4L * N;
    int rc = padded_geometry(p, H, W, &r_lo, &r_hi, &o_lo, &o_rows, &g);
    if (rc != RPSF_OK) return rc;
    HIP_TRY(hipSetDevice(p->device));
    rc = pipe_ensure(p, (size_t)PH * PW, slots);
    if (rc != RPSF_OK) return rc;
    if ((int)p->sat.size() < slots) p->sat.resize(slots);
    colmap.resize(PW);
    for (long c = 0; c < PW; ++c) colmap[c] = pad_index((int)(c - 2L * N), W, pad_mode);
    return RPSF_OK;
  }

  // host steps of one frame into slot s (pad, threshold, dilation, raw values, NaN, sequential fill, narrowing into the pinned staging)
  void prepare(int s, const void* image_host) {
    HostPipe& q = *p->pipe;
    HostPool& pool = HostPool::get(p->device);
    SatScratch& sc = p->sat[s];
    sc.padded.resize((size_t)PH * PW);
    sc.mask.assign((size_t)PH * PW, 0);
    sc.raw.clear();
    double* const padded = sc.padded.data();
    uint8_t* const mask = sc.mask.data();
    const int parts = (int)std::min<long>(PH, (long)pool.width() * 4);
    std::vector<std::vector<int64_t>> hot(parts);  // per part: flat indices of the pixels above the threshold
    // ---- pad (:119-123) + threshold (:129), row blocks in parallel
    pool.run(parts, [&](int part) {
      const long ra = PH * part / parts, rb = PH * (part + 1) / parts;
      for (long r = ra; r < rb; ++r) {
        const int sr = pad_index((int)(r - 2L * N), H, pad_mode);
        double* dst = padded + r * PW;
        if (sr < 0) {
          for (long c = 0; c < PW; ++c) dst[c] = 0.0;  // np.pad(mode="constant") pads with 0
        } else if (in_f64) {
          const double* src = static_cast<const double*>(image_host) + (size_t)sr * W;
          for (long c = 0; c < PW; ++c) dst[c] = colmap[c] < 0 ? 0.0 : src[colmap[c]];
        } else {
          const float* src = static_cast<const float*>(image_host) + (size_t)sr * W;
          for (long c = 0; c < PW; ++c) dst[c] = colmap[c] < 0 ? 0.0 : (double)src[colmap[c]];
        }
        for (long c = 0; c < PW; ++c)
          if (dst[c] > threshold) hot[part].push_back(r * PW + c);
      }
    });
    // ---- dilation (:133): every pixel within `dilation` city-block steps of a saturated one
    std::vector<uint8_t> row_has(PH, 0);
    size_t n_hot = 0;
    for (const auto& list : hot) {
      n_hot += list.size();
      for (const int64_t idx : list) {
        const long r = idx / PW, c = idx % PW;
        for (long dr = -dilation; dr <= dilation; ++dr) {
          const long rr = r + dr;
          if (rr < 0 || rr >= PH) continue;
          const long span = dilation - std::labs(dr);
          const long c0 = std::max<long>(0, c - span), c1 = std::min<long>(PW - 1, c + span);
          std::memset(mask + rr * PW + c0, 1, (size_t)(c1 - c0 + 1));
          row_has[rr] = 1;
        }
      }
    }
    // ---- raw values of the masked pixels the caller will see (:126, :172), NaN (:134), sequential fill (:135-138)
    if (n_hot) {
      for (long r = 0; r < PH; ++r) {
        if (!row_has[r]) continue;
        for (long c = 0; c < PW; ++c)
          if (mask[r * PW + c]) {
            if (r >= 2L * N && r < 2L * N + H && c >= 2L * N && c < 2L * N + W) sc.raw.push_back({r * PW + c, padded[r * PW + c]});
            padded[r * PW + c] = std::nan("");
          }
      }
      const long hw = width / 2;
      for (long i = 0; i < PH; ++i) {
        if (!row_has[i]) continue;
        for (long j = 0; j < PW; ++j) {
          if (!mask[i * PW + j]) continue;
          long r0, r1, c0, c1;
          py_slice(i - hw, i + hw, PH, &r0, &r1);
          py_slice(j - hw, j + hw, PW, &c0, &c1);
          double sum = 0.0;
          long cnt = 0;
          for (long r = r0; r < r1; ++r)
            for (long c = c0; c < c1; ++c) {
              const double v = padded[r * PW + c];
              if (v == v) sum += v, ++cnt;
            }
          padded[i * PW + j] = cnt ? sum / (double)cnt : std::nan("");
        }
      }
    }
    const size_t in_lo = (size_t)r_lo * PW, in_hi = (size_t)r_hi * PW;
    const int T = host_parts_for((in_hi - in_lo) * sizeof(float));
    pool.run(T, [&](int t) {
      size_t a, b;
      rpsf_host::split_range(in_lo, in_hi, t, T, a, b);
      rpsf_host::narrow_or_copy(q.h_in[s], padded, true, a, b);
    });
  }

  // the correction of the padded frame of slot s: rows the patches read in, the caller's rows out; asynchronous on the plan's stream
  hipError_t enqueue(int s) {
    HostPipe& q = *p->pipe;
    const size_t in_lo = (size_t)r_lo * PW, in_hi = (size_t)r_hi * PW, out_lo = (size_t)o_lo * PW, out_hi = out_lo + (size_t)o_rows * PW;
    hipError_t err = hipMemcpyAsync(q.d_in[s], q.h_in[s] + in_lo, (in_hi - in_lo) * sizeof(float), hipMemcpyHostToDevice, p->stream);
    if (err == hipSuccess && launch_apply(p, q.d_in[s], q.d_out[s], g, p->stream, nullptr) != RPSF_OK) err = hipErrorUnknown;
    if (err == hipSuccess) err = hipMemcpyAsync(q.h_out[s] + out_lo, q.d_out[s], (out_hi - out_lo) * sizeof(float), hipMemcpyDeviceToHost, p->stream);
    if (err == hipSuccess) err = hipEventRecord(q.ev_out[s], p->stream);
    return err;
  }

  // wait for slot s, then the crop (:174-177) with the raw values back on the mask (:172)
  hipError_t finish(int s, void* out_host) {
    HostPipe& q = *p->pipe;
    HostPool& pool = HostPool::get(p->device);
    hipError_t err = hipEventSynchronize(q.ev_out[s]);
    if (err != hipSuccess) return err;
    const int rows_parts = std::min(H, pool.width() * 4);
    pool.run(rows_parts, [&](int part) {
      const long ra = (long)H * part / rows_parts, rb = (long)H * (part + 1) / rows_parts;
      for (long r = ra; r < rb; ++r) {
        const float* src = q.h_out[s] + (size_t)(2 * N + r) * PW + 2 * N;  // (h_out is indexed by rows of the padded frame)
        if (out_f64) {
          double* dst = static_cast<double*>(out_host) + (size_t)r * W;
          for (long c = 0; c < W; ++c) dst[c] = (double)src[c];
        } else {
          std::memcpy(static_cast<float*>(out_host) + (size_t)r * W, src, (size_t)W * sizeof(float));
        }
      }
    });
    for (const SatScratch::Raw& x : p->sat[s].raw) {
      const long r = x.idx / PW - 2L * N, c = x.idx % PW - 2L * N;
      if (out_f64) static_cast<double*>(out_host)[(size_t)r * W + c] = x.value;
      else static_cast<float*>(out_host)[(size_t)r * W + c] = (float)x.value;
    }
    return hipSuccess;
  }
};

static int check_saturated_call(rpsf_plan* p, const void* a, const void* b, int height, int width, int pad_mode, int dilation, int neighborhood_width) {
  if (!p || !a || !b) return fail(RPSF_E_BADARG, "null argument");
  if (height <= 0 || width <= 0) return fail(RPSF_E_BADARG, "image shape must be positive");
  if (pad_mode < 0 || pad_mode > RPSF_PAD_WRAP) return fail(RPSF_E_BADARG, "unknown pad mode");
  if (dilation < 1 || neighborhood_width < 0) return fail(RPSF_E_BADARG, "dilation must be >= 1 and the neighbourhood width >= 0 (other values: the NumPy route)");
  if (!p->have_k) return fail(RPSF_E_STATE, "no transfer kernel installed (call rpsf_plan_set_transfer first)");
  return RPSF_OK;
}

extern "C" int rpsf_apply_host_saturated(rpsf_plan* p, const void* image_host, int image_is_f64, int height, int width, int pad_mode,
                                         double threshold, int dilation, int neighborhood_width, void* out_host, int out_is_f64) {
  int rc = check_saturated_call(p, image_host, out_host, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  SatRun run;
  rc = run.init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, image_is_f64, out_is_f64, 1);
  if (rc != RPSF_OK) return rc;
  run.prepare(0, image_host);
  hipError_t err = run.enqueue(0);
  if (err == hipSuccess) err = run.finish(0, out_host);
  if (err != hipSuccess) return drain_after_error(p, err, "saturated host frame");
  return sweep_check(p);
}

extern "C" int rpsf_apply_frames_host_saturated(rpsf_plan* p, const void* const* images_host, int image_is_f64, int n_frames, int height, int width,
                                                int pad_mode, double threshold, int dilation, int neighborhood_width, void* const* outs_host,
                                                int out_is_f64) {
  int rc = check_saturated_call(p, images_host, outs_host, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  if (n_frames <= 0) return fail(RPSF_E_BADARG, "n_frames must be positive");
  for (int f = 0; f < n_frames; ++f)
    if (!images_host[f] || !outs_host[f]) return fail(RPSF_E_BADARG, "null frame pointer");
  SatRun run;
  rc = run.init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, image_is_f64, out_is_f64, std::min(2, n_frames));
  if (rc != RPSF_OK) return rc;
  hipError_t err = hipSuccess;
  for (int f = 0; f < n_frames && err == hipSuccess; ++f) {
    run.prepare(f & 1, images_host[f]);  // (the slot's previous frame, f - 2, was finished in the iteration before)
    err = run.enqueue(f & 1);
    if (err == hipSuccess && f > 0) err = run.finish((f - 1) & 1, outs_host[f - 1]);  // the GPU has had the host steps of frame f to correct frame f - 1
  }
  if (err == hipSuccess) err = run.finish((n_frames - 1) & 1, outs_host[n_frames - 1]);
  if (err != hipSuccess) return drain_after_error(p, err, "saturated host frames");
  return sweep_check(p);
}

// ------------------------------------------------------------------------------------------------
// The same branch with every step on the device (csrc/saturation.hip, csrc/rpsf_core_saturation_batch.hpp): frames of one
// shape are cut into frame-groups; per frame-group F1 - F3 with the frame as a grid index build the filled padded frames from the
// resident H x W frames, one wait, one F4 launch, the shared-K batch launch corrects the padded frames with the geometry above, one F5
// launch restores and crops.  A single frame is a frame-group of one whose F4 takes the groups in the table's own order.
// ------------------------------------------------------------------------------------------------
struct SatDeviceRun {
  SatCall call;
  rpsf_geometry g;
  int r_lo, r_hi;
};

static int sat_device_init(rpsf_plan* p, int height, int width, int pad_mode, double threshold, int dilation, int neighborhood_width,
                           SatDeviceRun* run) {
  if (neighborhood_width / 2 < 1) return fail(RPSF_E_BADARG, "the device route needs neighborhood_width // 2 >= 1 (an always-empty window: the host route)");
  int o_lo, o_rows;
  const int rc = padded_geometry(p, height, width, &run->r_lo, &run->r_hi, &o_lo, &o_rows, &run->g);
  if (rc != RPSF_OK) return rc;
  run->call = SatCall{height, width, p->N, pad_mode, dilation, neighborhood_width, threshold, run->r_lo, o_lo, o_rows};
  HIP_TRY(hipSetDevice(p->device));
  if (!p->sat_dev) p->sat_dev.reset(rpsf_sat_create());
  return RPSF_OK;
}

// What rpsf_saturation_batch_info reports: the frames entry points store it, a single-frame call keeps its own and stores nothing
struct SatBatchStats {
  long frames = 0, frame_groups = 0, groups = 0, masked = 0;
  void store(rpsf_plan* p) const {
    const long v[4] = {frames, frame_groups, groups, masked};
    for (int i = 0; i < 4; ++i) p->sat_batch_info[i] = (int)std::min<long>(v[i], 0x7FFFFFFF);
  }
};

static int sat_group_frames(const rpsf_plan* p, const SatDeviceRun& run) {
  if (p->sat_group_opt > 0) return p->sat_group_opt;
  return rpsfsatb::auto_group_frames((size_t)run.g.height * run.g.width, (size_t)run.call.out_rows * run.g.width);
}

// one frame-group, resident; asynchronous on st but for the one wait inside rpsf_sat_fill_batch
static int sat_device_apply_group(rpsf_plan* p, const SatDeviceRun& run, int frames, const float* images_dev, size_t image_stride, float* outs_dev,
                                  size_t out_stride, int order, hipStream_t st, SatBatchStats* stats, size_t* n_masked_or_null) {
  float *padded = nullptr, *corrected = nullptr;
  size_t p_stride = 0, c_stride = 0;
  SatDevice* sd = p->sat_dev.get();
  int rc = rpsf_sat_fill_batch(sd, run.call, frames, images_dev, image_stride, order, st, &padded, &p_stride, &corrected, &c_stride);
  if (rc != RPSF_OK) return rc;
  rc = launch_batch(p, padded + (size_t)run.r_lo * run.g.width, corrected, frames, p_stride, c_stride, run.g, st);
  if (rc != RPSF_OK) return rc;
  rc = rpsf_sat_restore_batch(sd, run.call, images_dev, image_stride, outs_dev, out_stride, st);
  if (rc != RPSF_OK) return rc;
  long groups = 0, masked = 0;
  rpsf_sat_batch_totals(sd, &groups, &masked);
  stats->frame_groups += 1, stats->groups += groups, stats->masked += masked;
  for (int f = 0; n_masked_or_null && f < frames; ++f) {
    int n_hot, n_mask, n_groups;
    rpsf_sat_frame_counts(sd, f, &n_hot, &n_mask, &n_groups);
    n_masked_or_null[f] = (size_t)n_mask;
  }
  return RPSF_OK;
}

// one frame-group of host arrays through the plan's staging slot 0 (room for `frames` frames: pipe_ensure): staged as float32, uploaded,
// sat_device_apply_group, downloaded, widened; T: parts of the host pool's copies
static int sat_host_group(rpsf_plan* p, const SatDeviceRun& run, int frames, const void* const* images_host, int image_is_f64, void* const* outs_host,
                          int out_is_f64, int order, int T, SatBatchStats* stats) {
  const size_t npix = (size_t)run.call.H * run.call.W, total = npix * frames;
  HostPipe& q = *p->pipe;
  HostPool& pool = HostPool::get(p->device);
  pool.run(T, [&](int t) {  // the group's frames laid end to end, cut into T parts
    size_t a, b;
    rpsf_host::split_range(0, total, t, T, a, b);
    while (a < b) {
      const size_t f = a / npix, lo = a % npix, hi = std::min(npix, lo + (b - a));
      rpsf_host::narrow_or_copy(q.h_in[0] + f * npix, images_host[f], image_is_f64 != 0, lo, hi);
      a += hi - lo;
    }
  });
  hipError_t err = hipMemcpyAsync(q.d_in[0], q.h_in[0], total * sizeof(float), hipMemcpyHostToDevice, p->stream);
  if (err != hipSuccess) return drain_after_error(p, err, "saturated host frames, device route");
  int rc = sat_device_apply_group(p, run, frames, q.d_in[0], npix, q.d_out[0], npix, order, p->stream, stats, nullptr);
  if (rc != RPSF_OK) {
    (void)hipStreamSynchronize(p->stream);
    return rc;
  }
  err = hipMemcpyAsync(q.h_out[0], q.d_out[0], total * sizeof(float), hipMemcpyDeviceToHost, p->stream);
  if (err != hipSuccess) return drain_after_error(p, err, "saturated host frames, device route");
  const int32_t* list = nullptr;
  const int *info = nullptr, *counters = nullptr;
  rc = rpsf_sat_lists_batch(p->sat_dev.get(), p->stream, &list, &info, &counters);  // waits for the stream when there is a list
  if (rc != RPSF_OK) {
    (void)hipStreamSynchronize(p->stream);
    return rc;
  }
  if (!list) {
    err = hipStreamSynchronize(p->stream);
    if (err != hipSuccess) return drain_after_error(p, err, "saturated host frames, device route");
  }
  pool.run(T, [&](int t) {
    size_t a, b;
    rpsf_host::split_range(0, total, t, T, a, b);
    while (a < b) {
      const size_t f = a / npix, lo = a % npix, hi = std::min(npix, lo + (b - a));
      rpsf_host::widen_or_copy(outs_host[f], out_is_f64 != 0, q.h_out[0] + f * npix, lo, hi);
      a += hi - lo;
    }
  });
  if (image_is_f64 && list) {  // the caller's own values on the mask, not their float32 roundings
    for (int f = 0; f < frames; ++f) {
      const double* src = static_cast<const double*>(images_host[f]);
      const int32_t* mine = list + info[rpsfsatb::FRAME_INFO * f + rpsfsatb::I_LIST0];
      const int n = counters[rpsfsatb::FRAME_COUNTERS * f + rpsfsatb::C_HOT] ? counters[rpsfsatb::FRAME_COUNTERS * f + rpsfsatb::C_LIST] : 0;
      for (int k = 0; k < n; ++k) {
        if (out_is_f64) static_cast<double*>(outs_host[f])[mine[k]] = src[mine[k]];
        else static_cast<float*>(outs_host[f])[mine[k]] = (float)src[mine[k]];
      }
    }
  }
  return RPSF_OK;
}

extern "C" int rpsf_apply_device_saturated(rpsf_plan* p, const void* image_dev, void* out_dev, int height, int width, int pad_mode, double threshold,
                                           int dilation, int neighborhood_width, void* stream, size_t* n_masked_or_null) {
  int rc = check_saturated_call(p, image_dev, out_dev, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  SatDeviceRun run;
  rc = sat_device_init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, &run);
  if (rc != RPSF_OK) return rc;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : p->stream;
  const size_t npix = (size_t)height * width;
  SatBatchStats stats;
  return sat_device_apply_group(p, run, 1, static_cast<const float*>(image_dev), npix, static_cast<float*>(out_dev), npix, rpsfsatb::ORDER_FRAMES, st,
                                &stats, n_masked_or_null);
}

extern "C" int rpsf_apply_host_saturated_device(rpsf_plan* p, const void* image_host, int image_is_f64, int height, int width, int pad_mode,
                                                double threshold, int dilation, int neighborhood_width, void* out_host, int out_is_f64) {
  int rc = check_saturated_call(p, image_host, out_host, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  SatDeviceRun run;
  rc = sat_device_init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, &run);
  if (rc != RPSF_OK) return rc;
  const size_t npix = (size_t)height * width;
  rc = pipe_ensure(p, npix, 1);
  if (rc != RPSF_OK) return rc;
  SatBatchStats stats;
  rc = sat_host_group(p, run, 1, &image_host, image_is_f64, &out_host, out_is_f64, rpsfsatb::ORDER_FRAMES, host_parts_for(npix * sizeof(float)), &stats);
  return rc != RPSF_OK ? rc : sweep_check(p);
}

extern "C" int rpsf_apply_batch_device_saturated(rpsf_plan* p, const void* images_dev, void* outs_dev, int n_frames, size_t image_stride,
                                                 size_t out_stride, int height, int width, int pad_mode, double threshold, int dilation,
                                                 int neighborhood_width, void* stream, size_t* n_masked_per_frame_or_null) {
  if (p && n_frames == 0) {
    SatBatchStats().store(p);
    return RPSF_OK;
  }
  int rc = check_saturated_call(p, images_dev, outs_dev, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  if (n_frames < 0) return fail(RPSF_E_BADARG, "n_frames must not be negative");
  if (n_frames > 1 && (image_stride < (size_t)height * width || out_stride < (size_t)height * width))
    return fail(RPSF_E_BADARG, "frame stride smaller than one frame");
  SatDeviceRun run;
  rc = sat_device_init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, &run);
  if (rc != RPSF_OK) return rc;
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : p->stream;
  const int G = sat_group_frames(p, run);
  SatBatchStats stats;
  stats.frames = n_frames;
  for (int f0 = 0; f0 < n_frames; f0 += G) {
    rc = sat_device_apply_group(p, run, std::min(G, n_frames - f0), static_cast<const float*>(images_dev) + (size_t)f0 * image_stride, image_stride,
                                static_cast<float*>(outs_dev) + (size_t)f0 * out_stride, out_stride, rpsfsatb::ORDER_LONGEST_FIRST, st, &stats,
                                n_masked_per_frame_or_null ? n_masked_per_frame_or_null + f0 : nullptr);
    if (rc != RPSF_OK) return rc;
  }
  stats.store(p);
  return RPSF_OK;
}

extern "C" int rpsf_apply_frames_host_saturated_device(rpsf_plan* p, const void* const* images_host, int image_is_f64, int n_frames, int height,
                                                       int width, int pad_mode, double threshold, int dilation, int neighborhood_width,
                                                       void* const* outs_host, int out_is_f64) {
  if (p && n_frames == 0) {
    SatBatchStats().store(p);
    return RPSF_OK;
  }
  int rc = check_saturated_call(p, images_host, outs_host, height, width, pad_mode, dilation, neighborhood_width);
  if (rc != RPSF_OK) return rc;
  if (n_frames < 0) return fail(RPSF_E_BADARG, "n_frames must not be negative");
  for (int f = 0; f < n_frames; ++f)
    if (!images_host[f] || !outs_host[f]) return fail(RPSF_E_BADARG, "null frame pointer");
  SatDeviceRun run;
  rc = sat_device_init(p, height, width, pad_mode, threshold, dilation, neighborhood_width, &run);
  if (rc != RPSF_OK) return rc;
  const size_t npix = (size_t)height * width;
  const int G = std::min(sat_group_frames(p, run), n_frames);
  rc = pipe_ensure(p, npix * G, 1);
  if (rc != RPSF_OK) return rc;
  const int T = host_parts_for(npix * G * sizeof(float));
  SatBatchStats stats;
  stats.frames = n_frames;
  for (int f0 = 0; f0 < n_frames; f0 += G) {
    rc = sat_host_group(p, run, std::min(G, n_frames - f0), images_host + f0, image_is_f64, outs_host + f0, out_is_f64, rpsfsatb::ORDER_LONGEST_FIRST, T,
                        &stats);
    if (rc != RPSF_OK) return rc;
  }
  stats.store(p);
  return sweep_check(p);
}

// ------------------------------------------------------------------------------------------------
// Device-array views (include/rpsf.h, rpsf_view): a side that is what rpsf_geometry describes goes into the launch as it is, any other
// through the plan's staging and kernel C1 / C2 (csrc/convert.hip; predicate and checks: csrc/rpsf_core_convert.hpp)
// ------------------------------------------------------------------------------------------------
// One side of a call: `n` views of one shape.  direct: every view zero copy (dense, for the saturation route), one row stride, evenly
// spaced by a positive multiple of 4 bytes that holds a frame.  uniform: one dtype, one pair of strides, evenly spaced - one C1 / C2 launch.
struct ViewSide {
  bool direct = true, uniform = true;
  int64_t frame_bytes = 0;
};
static ViewSide view_side(const rpsf_view* v, int n, bool need_dense) {
  ViewSide s;
  s.frame_bytes = n > 1 ? static_cast<char*>(v[1].data) - static_cast<char*>(v[0].data) : 0;
  for (int f = 0; f < n; ++f) {
    if (!(need_dense ? rpsfconv::dense_f32(v[f]) : rpsfconv::zero_copy(v[f]))) s.direct = false;
    if (v[f].dtype != v[0].dtype || v[f].row_stride != v[0].row_stride || v[f].col_stride != v[0].col_stride ||
        static_cast<char*>(v[f].data) - static_cast<char*>(v[0].data) != (int64_t)f * s.frame_bytes)
      s.direct = s.uniform = false;
  }
  if (n > 1 && (s.frame_bytes <= 0 || s.frame_bytes % 4 || s.frame_bytes < (int64_t)(v[0].rows - 1) * v[0].row_stride + 4 * (int64_t)v[0].cols))
    s.direct = false;
  return s;
}

static int view_staging(DevBuf<float>& buf, size_t& cap, size_t floats) {
  if (floats <= cap) return RPSF_OK;
  HIP_TRY(hipDeviceSynchronize());  // earlier calls, on whatever stream, may still use the old staging
  cap = 0;
  HIP_TRY(buf.alloc(floats));
  cap = floats;
  return RPSF_OK;
}

static int apply_views(rpsf_plan* p, const rpsf_view* images, const rpsf_view* outs, int n, int pad_mode, float pad_value, double threshold, int dilation,
                       int neighborhood_width, void* stream, int* route_or_null, bool batch) {
  if (route_or_null) *route_or_null = 0;
  if (!p) return fail(RPSF_E_BADARG, "null plan");
  if (n < 0) return fail(RPSF_E_BADARG, "n_frames must not be negative");
  if (n == 0) return RPSF_OK;
  if (!images || !outs) return fail(RPSF_E_BADARG, "null argument");
  bool empty = false;
  for (int f = 0; f < n; ++f) {
    bool e_in, e_out;
    if (const char* why = rpsfconv::view_problem(images + f, false, &e_in)) return fail(RPSF_E_BADARG, std::string("image: ") + why);
    if (const char* why = rpsfconv::view_problem(outs + f, true, &e_out)) return fail(RPSF_E_BADARG, std::string("out: ") + why);
    if (images[f].rows != images[0].rows || images[f].cols != images[0].cols || outs[f].rows != images[0].rows || outs[f].cols != images[0].cols)
      return fail(RPSF_E_BADARG, "every image and every out view must have one shape");
    empty = e_in;
  }
  if (empty) return RPSF_OK;
  if (pad_mode < 0 || pad_mode > RPSF_PAD_WRAP) return fail(RPSF_E_BADARG, "unknown pad mode");
  if (!p->have_k) return fail(RPSF_E_STATE, "no transfer kernel installed (call rpsf_plan_set_transfer first)");
  const int H = images[0].rows, W = images[0].cols;
  const bool saturated = !(threshold == std::numeric_limits<double>::infinity());
  const ViewSide in = view_side(images, n, saturated), out = view_side(outs, n, saturated);
  rpsf_geometry g{H, W, pad_mode, pad_value, 0, 0, 0, H, in.direct ? (int)(images[0].row_stride / 4) : W, 0, H, out.direct ? (int)(outs[0].row_stride / 4) : W};
  SatDeviceRun run;
  int rc;
  if (saturated) {
    if (dilation < 1 || neighborhood_width < 0) return fail(RPSF_E_BADARG, "dilation must be >= 1 and the neighbourhood width >= 0 (other values: the NumPy route)");
    rc = sat_device_init(p, H, W, pad_mode, threshold, dilation, neighborhood_width, &run);
  } else {
    rc = check_geometry(p, &g);
  }
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : p->stream;
  const size_t npix = (size_t)H * W, stage_stride = (npix + 3) / 4 * 4;  // (every staged frame starts on 16 bytes)
  const bool staged = !in.direct || !out.direct;
  if (!in.direct && (rc = view_staging(p->d_view_in, p->view_in_floats, stage_stride * n)) != RPSF_OK) return rc;
  if (!out.direct && (rc = view_staging(p->d_view_out, p->view_out_floats, stage_stride * n)) != RPSF_OK) return rc;
  if (staged) {  // the staging serves one call at a time: a call on another stream waits, on the device, for the last one that used it
    if (!p->ev_view) HIP_TRY(hipEventCreateWithFlags(&p->ev_view, hipEventDisableTiming));
    if (p->view_busy && st != p->view_stream) HIP_TRY(hipStreamWaitEvent(st, p->ev_view, 0));
  }
  const float* d_in = static_cast<const float*>(images[0].data);
  float* d_out = static_cast<float*>(outs[0].data);
  size_t in_stride = (size_t)(in.frame_bytes / 4), out_stride = (size_t)(out.frame_bytes / 4);
  if (!in.direct) {
    if (in.uniform) rc = rpsf_conv_gather(images[0], n, in.frame_bytes, p->d_view_in, (int64_t)stage_stride, st);
    for (int f = 0; !in.uniform && f < n && rc == RPSF_OK; ++f) rc = rpsf_conv_gather(images[f], 1, 0, p->d_view_in + f * stage_stride, 0, st);
    if (rc != RPSF_OK) return rc;
    d_in = p->d_view_in, in_stride = stage_stride;
  }
  if (!out.direct) d_out = p->d_view_out, out_stride = stage_stride;
  if (!saturated) {
    rc = launch_batch(p, d_in, d_out, n, in_stride, out_stride, g, st);
  } else {
    const int G = batch ? sat_group_frames(p, run) : 1;
    SatBatchStats stats;
    stats.frames = n;
    for (int f0 = 0; f0 < n && rc == RPSF_OK; f0 += G)
      rc = sat_device_apply_group(p, run, std::min(G, n - f0), d_in + (size_t)f0 * in_stride, in_stride, d_out + (size_t)f0 * out_stride, out_stride,
                                  batch ? rpsfsatb::ORDER_LONGEST_FIRST : rpsfsatb::ORDER_FRAMES, st, &stats, nullptr);
    if (batch && rc == RPSF_OK) stats.store(p);
  }
  if (rc == RPSF_OK && !out.direct) {
    if (out.uniform) rc = rpsf_conv_scatter(p->d_view_out, (int64_t)stage_stride, outs[0], n, out.frame_bytes, st);
    for (int f = 0; !out.uniform && f < n && rc == RPSF_OK; ++f) rc = rpsf_conv_scatter(p->d_view_out + f * stage_stride, 0, outs[f], 1, 0, st);
  }
  if (staged) {
    HIP_TRY(hipEventRecord(p->ev_view, st));
    p->view_stream = st, p->view_busy = true;
  }
  if (rc == RPSF_OK && route_or_null)
    *route_or_null = (in.direct ? 0 : RPSF_ROUTE_C1 | (batch ? RPSF_ROUTE_STAGED : 0)) | (out.direct ? 0 : RPSF_ROUTE_C2) | (saturated ? RPSF_ROUTE_SATURATED : 0);
  return rc;
}

extern "C" int rpsf_apply_view(rpsf_plan* p, const rpsf_view* image, const rpsf_view* out, int pad_mode, float pad_value, double threshold, int dilation,
                               int neighborhood_width, void* stream, int* route_or_null) {
  return apply_views(p, image, out, 1, pad_mode, pad_value, threshold, dilation, neighborhood_width, stream, route_or_null, false);
}

extern "C" int rpsf_apply_batch_view(rpsf_plan* p, const rpsf_view* images, const rpsf_view* outs, int n_frames, int pad_mode, float pad_value,
                                     double threshold, int dilation, int neighborhood_width, void* stream, int* route_or_null) {
  return apply_views(p, images, outs, n_frames, pad_mode, pad_value, threshold, dilation, neighborhood_width, stream, route_or_null, true);
}

extern "C" int rpsf_saturation_kernel_ms(rpsf_plan* p, double ms[5]) {
  if (!p || !ms) return fail(RPSF_E_BADARG, "null argument");
  for (int i = 0; i < 5; ++i) ms[i] = 0.0;
  if (!p->sat_dev) return RPSF_OK;
  HIP_TRY(hipSetDevice(p->device));
  return rpsf_sat_kernel_ms(p->sat_dev.get(), ms);
}

extern "C" int rpsf_saturation_batch_info(rpsf_plan* p, int info[4]) {
  if (!p || !info) return fail(RPSF_E_BADARG, "null argument");
  for (int i = 0; i < 4; ++i) info[i] = p->sat_batch_info[i];
  return RPSF_OK;
}

// The test entries: F1 - F4 alone on n_frames float32 host frames, frame-group by frame-group; the filled padded frames
// ((H + 4N) x (W + 4N) float32 each) and the masks come back
static int sat_fill_frames(rpsf_plan* p, const float* images_host, int n_frames, int height, int width, int pad_mode, double threshold, int dilation,
                           int neighborhood_width, int order, float* padded_host, uint8_t* masks_host, int* groups_per_frame_or_null,
                           SatBatchStats* stats) {
  if (!p || !images_host || !padded_host || !masks_host) return fail(RPSF_E_BADARG, "null argument");
  if (n_frames < 1) return fail(RPSF_E_BADARG, "n_frames must be positive");
  if (height <= 0 || width <= 0) return fail(RPSF_E_BADARG, "image shape must be positive");
  if (pad_mode < 0 || pad_mode > RPSF_PAD_WRAP) return fail(RPSF_E_BADARG, "unknown pad mode");
  if (dilation < 1 || neighborhood_width / 2 < 1) return fail(RPSF_E_BADARG, "dilation must be >= 1 and neighborhood_width // 2 >= 1");
  if (order < rpsfsatb::ORDER_LONGEST_FIRST || order > rpsfsatb::ORDER_FRAMES) return fail(RPSF_E_BADARG, "order must be 0, 1 or 2");
  const long PH = (long)height + 4L * p->N, PW = (long)width + 4L * p->N;
  if (PH * PW >= ((long)1 << 31)) return fail(RPSF_E_UNSUPPORTED, "padded frame too large for this entry point");
  HIP_TRY(hipSetDevice(p->device));
  if (!p->sat_dev) p->sat_dev.reset(rpsf_sat_create());
  SatDevice* sd = p->sat_dev.get();
  const SatCall call{height, width, p->N, pad_mode, dilation, neighborhood_width, threshold, 0, 0, 1};
  const size_t npix = (size_t)height * width, np = (size_t)PH * PW;
  const int G = std::min(n_frames, p->sat_group_opt > 0 ? p->sat_group_opt : rpsfsatb::auto_group_frames(np, (size_t)height * PW));
  DevBuf<float> d_images;
  HIP_TRY(d_images.upload(images_host, npix * n_frames));
  stats->frames = n_frames;
  for (int f0 = 0; f0 < n_frames; f0 += G) {
    const int fg = std::min(G, n_frames - f0);
    float *padded = nullptr, *corrected = nullptr;
    size_t p_stride = 0, c_stride = 0;
    const float* d_first = d_images;
    int rc = rpsf_sat_fill_batch(sd, call, fg, d_first + (size_t)f0 * npix, npix, order, p->stream, &padded, &p_stride, &corrected, &c_stride);
    if (rc == RPSF_OK) rc = rpsf_sat_masks_batch(sd, call, p->stream, masks_host + (size_t)f0 * np);  // waits for the stream
    if (rc != RPSF_OK) {
      (void)hipStreamSynchronize(p->stream);
      return rc;
    }
    for (int f = 0; f < fg; ++f) {
      HIP_TRY(hipMemcpy(padded_host + (size_t)(f0 + f) * np, padded + f * p_stride, np * sizeof(float), hipMemcpyDeviceToHost));
      int n_hot, n_mask, n_groups;
      rpsf_sat_frame_counts(sd, f, &n_hot, &n_mask, &n_groups);
      if (groups_per_frame_or_null) groups_per_frame_or_null[f0 + f] = n_groups;
    }
    long groups = 0, masked = 0;
    rpsf_sat_batch_totals(sd, &groups, &masked);
    stats->frame_groups += 1, stats->groups += groups, stats->masked += masked;
  }
  return RPSF_OK;
}

// one frame; reverse_groups: F4's workgroups take the groups in the reverse of the batch's order instead of the table's own
extern "C" int rpsf_saturation_fill_device(rpsf_plan* p, const float* image_host, int height, int width, int pad_mode, double threshold, int dilation,
                                           int neighborhood_width, int reverse_groups, float* padded_host, uint8_t* mask_host, int* n_groups_or_null) {
  SatBatchStats stats;
  return sat_fill_frames(p, image_host, 1, height, width, pad_mode, threshold, dilation, neighborhood_width,
                         reverse_groups ? rpsfsatb::ORDER_REVERSED : rpsfsatb::ORDER_FRAMES, padded_host, mask_host, n_groups_or_null, &stats);
}

extern "C" int rpsf_saturation_fill_batch_device(rpsf_plan* p, const float* images_host, int n_frames, int height, int width, int pad_mode,
                                                 double threshold, int dilation, int neighborhood_width, int order, float* padded_host,
                                                 uint8_t* masks_host, int* groups_per_frame_or_null) {
  SatBatchStats stats;
  const int rc = sat_fill_frames(p, images_host, n_frames, height, width, pad_mode, threshold, dilation, neighborhood_width, order, padded_host,
                                 masks_host, groups_per_frame_or_null, &stats);
  if (rc == RPSF_OK) stats.store(p);
  return rc;
}

// Self-test of the host worker pool (no GPU involved: the CPU test suite calls it): `jobs` jobs of `parts` parts from each of `callers` threads at
// once; every part adds its index into a per-job cell and the job must see the exact total when run() returns.  Returns the number of jobs
// whose total was wrong (0 = pass) through *failures.
extern "C" int rpsf_host_pool_selftest(int callers, int jobs, int parts, int* failures) {
  if (!failures || callers <= 0 || jobs <= 0 || parts <= 0) return fail(RPSF_E_BADARG, "bad argument");
  HostPool& pool = HostPool::get();
  std::atomic<int> bad{0};
  auto caller = [&](int id) {
    for (int j = 0; j < jobs; ++j) {
      const int n = 1 + (parts + id + j) % parts;  // varying job sizes, single-part jobs included
      std::atomic<long> sum{0};
      std::vector<int> hits(n, 0);
      pool.run(n, [&](int i) {
        sum.fetch_add(i + 1, std::memory_order_relaxed);
        ++hits[i];  // every part exactly once, by exactly one thread
      });
      bool ok = sum.load() == (long)n * (n + 1) / 2;
      for (int i = 0; i < n && ok; ++i) ok = hits[i] == 1;
      if (!ok) bad.fetch_add(1);
    }
  };
  std::vector<std::thread> threads;
  for (int c = 1; c < callers; ++c) threads.emplace_back(caller, c);
  caller(0);
  for (auto& t : threads) t.join();
  *failures = bad.load();
  return RPSF_OK;
}

extern "C" int rpsf_host_threads(int* threads) {
  if (!threads) return fail(RPSF_E_BADARG, "null argument");
  *threads = HostPool::get().width();
  return RPSF_OK;
}

// What PCIe gives a frame on this box: `bytes` from pinned host memory to the device, back, and both at once on two streams,
// `iters` times each (best).  The floor that the streamed entry points are measured against (end-to-end is reported
// separately from the device-resident figure).
extern "C" int rpsf_pcie_probe(int device, size_t bytes, int iters, double* h2d_ms, double* d2h_ms, double* duplex_ms) {
  if (bytes == 0 || iters <= 0) return fail(RPSF_E_BADARG, "bad argument");
  HIP_TRY(hipSetDevice(device));
  struct Res {
    void *h0 = nullptr, *h1 = nullptr;
    DevBuf<char> d0, d1;
    hipStream_t s0 = nullptr, s1 = nullptr;
    hipEvent_t e[4] = {};
    ~Res() {
      (void)hipHostFree(h0);
      (void)hipHostFree(h1);
      for (auto& x : e)
        if (x) (void)hipEventDestroy(x);
      if (s0) (void)hipStreamDestroy(s0);
      if (s1) (void)hipStreamDestroy(s1);
    }
  } r;
  HIP_TRY(hipHostMalloc(&r.h0, bytes, hipHostMallocDefault));
  HIP_TRY(hipHostMalloc(&r.h1, bytes, hipHostMallocDefault));
  std::memset(r.h0, 1, bytes);
  std::memset(r.h1, 2, bytes);
  HIP_TRY(r.d0.alloc(bytes));
  HIP_TRY(r.d1.alloc(bytes));
  HIP_TRY(hipStreamCreateWithFlags(&r.s0, hipStreamNonBlocking));
  HIP_TRY(hipStreamCreateWithFlags(&r.s1, hipStreamNonBlocking));
  for (auto& x : r.e) HIP_TRY(hipEventCreate(&x));
  double best[3] = {1e30, 1e30, 1e30};
  for (int mode = 0; mode < 3; ++mode)
    for (int i = 0; i < iters + 1; ++i) {  // (the first pass of a mode is a warm-up)
      HIP_TRY(hipDeviceSynchronize());
      const auto t0 = std::chrono::steady_clock::now();
      if (mode != 1) HIP_TRY(hipMemcpyAsync(r.d0.p, r.h0, bytes, hipMemcpyHostToDevice, r.s0));
      if (mode != 0) HIP_TRY(hipMemcpyAsync(r.h1, r.d1.p, bytes, hipMemcpyDeviceToHost, r.s1));
      HIP_TRY(hipStreamSynchronize(r.s0));
      HIP_TRY(hipStreamSynchronize(r.s1));
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (i > 0) best[mode] = std::min(best[mode], ms);
    }
  if (h2d_ms) *h2d_ms = best[0];
  if (d2h_ms) *d2h_ms = best[1];
  if (duplex_ms) *duplex_ms = best[2];
  return RPSF_OK;
}

extern "C" int rpsf_apply_device_timed(rpsf_plan* p, const void* image_dev, void* out_dev, const rpsf_geometry* geom,
                                       int iters, float* total_ms, float* kernel_ms) {
  if (!p || !image_dev || !out_dev || iters <= 0) return fail(RPSF_E_BADARG, "bad argument");
  if (!p->have_k) return fail(RPSF_E_STATE, "no transfer kernel installed (call rpsf_plan_set_transfer first)");
  int rc = check_geometry(p, geom);
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  return timed_loop(p, iters, total_ms, kernel_ms, [&](hipEvent_t k0, hipEvent_t k1) {
    return launch_apply(p, reinterpret_cast<const float*>(image_dev), reinterpret_cast<float*>(out_dev), *geom, p->stream, k0, k1);
  });
}

// `iters` applies back to back between ONE pair of events on the plan's stream: the average apply as the device sees it, with nothing
// between two launches that a caller's loop would not put there (per-apply event pairs cost a marker packet each: ~8 us of the 184 here).
// Nothing at all, since launch_apply records its end-of-apply event only for plans that have been applied on more than one stream: that
// record - no timing, nobody waiting - alone kept consecutive launches 5.8 us apart (kernel trace, profiles/head_kprefetch_ab.log: end of
// launch i to start of launch i + 1, 5.80 -> 0.00 us; start to start 187.2 -> 182.7 us).
extern "C" int rpsf_apply_device_loop_ms(rpsf_plan* p, const void* image_dev, void* out_dev, const rpsf_geometry* geom, int iters,
                                         double* ms_per_apply) {
  if (!p || !image_dev || !out_dev || iters <= 0 || !ms_per_apply) return fail(RPSF_E_BADARG, "bad argument");
  if (!p->have_k) return fail(RPSF_E_STATE, "no transfer kernel installed (call rpsf_plan_set_transfer first)");
  int rc = check_geometry(p, geom);
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  HIP_TRY(hipEventRecord(p->ev[0], p->stream));
  for (int i = 0; i < iters; ++i) {
    rc = launch_apply(p, reinterpret_cast<const float*>(image_dev), reinterpret_cast<float*>(out_dev), *geom, p->stream, nullptr);
    if (rc != RPSF_OK) return rc;
  }
  HIP_TRY(hipEventRecord(p->ev[3], p->stream));
  HIP_TRY(hipEventSynchronize(p->ev[3]));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, p->ev[0], p->ev[3]));
  *ms_per_apply = (double)ms / iters;
  return sweep_check(p);
}

// ------------------------------------------------------------------------------------------------
// K2 entry points
// ------------------------------------------------------------------------------------------------
extern "C" int rpsf_build_transfer_device(int device, size_t count, const void* s_dev, const void* t_dev, int is_f64,
                                          double alpha, double epsilon, void* k_dev, void* stream) {
  if (!s_dev || !t_dev || !k_dev) return fail(RPSF_E_BADARG, "null argument");
  if (count == 0) return RPSF_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int block = 256;
  size_t grid = (count + block - 1) / block;
  if (is_f64)
    build_transfer_kernel<double><<<dim3((unsigned)grid), dim3(block), 0, st>>>(
        (const double*)s_dev, (const double*)t_dev, (double*)k_dev, count, alpha, epsilon);
  else
    build_transfer_kernel<float><<<dim3((unsigned)grid), dim3(block), 0, st>>>(
        (const float*)s_dev, (const float*)t_dev, (float*)k_dev, count, (float)alpha, (float)epsilon);
  HIP_TRY(hipGetLastError());
  return RPSF_OK;
}

extern "C" int rpsf_build_transfer(int device, size_t count, const void* s_host, const void* t_host, int is_f64,
                                   double alpha, double epsilon, void* k_host) {
  if (!s_host || !t_host || !k_host) return fail(RPSF_E_BADARG, "null argument");
  if (count == 0) return RPSF_OK;
  HIP_TRY(hipSetDevice(device));
  const size_t esz = is_f64 ? 16 : 8;
  const size_t chunk = std::min<size_t>(count, (size_t)8 << 20);  // 8 Mi elements per round
  DevBuf<char> ds, dt, dk;
  HIP_TRY(ds.alloc(chunk * esz));
  HIP_TRY(dt.alloc(chunk * esz));
  HIP_TRY(dk.alloc(chunk * esz));
  int rc = RPSF_OK;
  for (size_t first = 0; first < count && rc == RPSF_OK; first += chunk) {
    size_t cnt = std::min(chunk, count - first);
    hipError_t e = hipMemcpy(ds, (const char*)s_host + first * esz, cnt * esz, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dt, (const char*)t_host + first * esz, cnt * esz, hipMemcpyHostToDevice);
    if (e != hipSuccess) { rc = fail(RPSF_E_HIP, hipGetErrorString(e)); break; }
    rc = rpsf_build_transfer_device(device, cnt, ds, dt, is_f64, alpha, epsilon, dk, nullptr);
    if (rc != RPSF_OK) break;
    e = hipMemcpy((char*)k_host + first * esz, dk, cnt * esz, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(RPSF_E_HIP, hipGetErrorString(e));
  }
  return rc;
}

// ------------------------------------------------------------------------------------------------
// K3 entry point
// ------------------------------------------------------------------------------------------------
// fft_host / fft_dev: exactly one is non-null - where the spectra go
// model < 0: the samples come from values_host; otherwise they are rasterised on the device from params_host
// (count x RPSF_MODEL_PARAMS doubles) and, if values_dev is given, kept there as float32 as well
static int psf_fft_impl(int device, int patch_size, int count, const float* values_host, float* fft_host, void* fft_dev,
                        int model = -1, const double* params_host = nullptr, int normalize = 0, void* values_dev = nullptr) {
  if ((model < 0 ? !values_host : !params_host) || (!fft_host && !fft_dev)) return fail(RPSF_E_BADARG, "null argument");
  if (model > MODEL_MOFFAT) return fail(RPSF_E_BADARG, "unknown PSF model");
  if (count <= 0) return count == 0 ? RPSF_OK : fail(RPSF_E_BADARG, "negative count");
  return dispatch_n(patch_size, [&]<class C>() -> int {
    HIP_TRY(hipSetDevice(device));
    DevBuf<uint16_t> d_tab;
    DevBuf<cf> d_tw;
    int rc = upload_tables<PatchPlan<C, false>>(device, d_tab, d_tw);
    if (rc != RPSF_OK) return rc;
    DevBuf<float> b_in;
    DevBuf<cf> b_out;
    DevBuf<double> b_par;
    const size_t per = (size_t)C::N * C::N;
    int chunk = (int)std::max<size_t>(1, (size_t)(64u << 20) / (per * sizeof(cf)));
    if (chunk > count) chunk = count;
    if (!(model >= 0 && values_dev)) HIP_TRY(b_in.alloc(per * chunk));  // (rasterised straight into values_dev otherwise)
    if (!fft_dev) HIP_TRY(b_out.alloc(per * chunk));
    if (model >= 0) HIP_TRY(b_par.upload(params_host, RPSF_MODEL_PARAMS_DEV * (size_t)count));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&psf_fft_kernel<C>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)Launch<C>::LDS_BYTES));
    for (int first = 0; first < count && rc == RPSF_OK; first += chunk) {
      int cnt = std::min(chunk, count - first);
      cf* d_out = fft_dev ? static_cast<cf*>(fft_dev) + (size_t)first * per : b_out;
      float* d_in = model >= 0 && values_dev ? static_cast<float*>(values_dev) + (size_t)first * per : b_in;
      hipError_t e = hipSuccess;
      if (model < 0) {
        e = hipMemcpy(d_in, values_host + (size_t)first * per, per * sizeof(float) * cnt, hipMemcpyHostToDevice);
      } else {
        rasterize_kernel<<<dim3((unsigned)cnt), dim3(256), 0, nullptr>>>(model, C::N, b_par + (size_t)first * RPSF_MODEL_PARAMS_DEV,
                                                                      normalize, d_in);
        e = hipGetLastError();
      }
      if (e != hipSuccess) { rc = fail(RPSF_E_HIP, hipGetErrorString(e)); break; }
      constexpr int TEAMS = Launch<C>::TEAMS;
      unsigned grid = (unsigned)((cnt + TEAMS - 1) / TEAMS);
      psf_fft_kernel<C><<<dim3(grid), dim3(Launch<C>::WG), Launch<C>::LDS_BYTES, nullptr>>>(d_in, cnt, d_tab, d_tw, d_out);
      e = hipGetLastError();
      if (e == hipSuccess && fft_host)
        e = hipMemcpy(reinterpret_cast<cf*>(fft_host) + (size_t)first * per, d_out, per * sizeof(cf) * cnt, hipMemcpyDeviceToHost);
      if (e == hipSuccess && !fft_host) e = hipDeviceSynchronize();  // d_in is reused by the next chunk
      if (e != hipSuccess) rc = fail(RPSF_E_HIP, hipGetErrorString(e));
    }
    return rc;
  });
}

extern "C" int rpsf_psf_fft(int device, int patch_size, int count, const float* values_host, float* fft_host) {
  return psf_fft_impl(device, patch_size, count, values_host, fft_host, nullptr);
}
extern "C" int rpsf_psf_fft_device(int device, int patch_size, int count, const float* values_host, void* fft_c64_dev) {
  return psf_fft_impl(device, patch_size, count, values_host, nullptr, fft_c64_dev);
}
static_assert(RPSF_MODEL_PARAMS == RPSF_MODEL_PARAMS_DEV && RPSF_MODEL_ELLIPTICAL_GAUSSIAN == MODEL_ELLIPTICAL_GAUSSIAN &&
              RPSF_MODEL_MOFFAT == MODEL_MOFFAT, "rpsf.h and the kernel agree on the model table");
extern "C" int rpsf_psf_model_fft_device(int device, int model, int patch_size, int count, const double* params_host,
                                         int normalize, void* values_f32_dev, void* fft_c64_dev) {
  if (model < 0) return fail(RPSF_E_BADARG, "unknown PSF model");
  return psf_fft_impl(device, patch_size, count, nullptr, nullptr, fft_c64_dev, model, params_host, normalize, values_f32_dev);
}

// ------------------------------------------------------------------------------------------------
// Host-side saturation fill (regularizepsf/transform.py:135-138).  Sequential by definition: masked pixels
// are visited in row-major order and each is replaced by the NaN-ignoring mean of the window
// [i - w/2, i + w/2) x [j - w/2, j + w/2), so later pixels see earlier fills.  Window bounds follow Python
// slice semantics (a negative start wraps once; an empty window gives NaN), as in the reference.
// ------------------------------------------------------------------------------------------------

extern "C" int rpsf_saturation_fill(double* padded, int rows, int cols, const uint8_t* mask, int neighborhood_width) {
  if (!padded || !mask || rows <= 0 || cols <= 0) return fail(RPSF_E_BADARG, "bad argument");
  const long h = neighborhood_width / 2;  // floor division, like Python's // for the non-negative widths in use
  const double nan = std::nan("");
  for (long i = 0; i < rows; ++i)
    for (long j = 0; j < cols; ++j) {
      if (!mask[i * cols + j]) continue;
      long r0, r1, c0, c1;
      py_slice(i - h, i + h, rows, &r0, &r1);
      py_slice(j - h, j + h, cols, &c0, &c1);
      double sum = 0.0;
      long cnt = 0;
      for (long r = r0; r < r1; ++r)
        for (long c = c0; c < c1; ++c) {
          double v = padded[r * cols + c];
          if (v == v) sum += v, ++cnt;
        }
      padded[i * cols + j] = cnt ? sum / (double)cnt : nan;
    }
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------
// device memory helpers
// ------------------------------------------------------------------------------------------------
extern "C" int rpsf_dev_alloc(int device, size_t bytes, void** out) {
  if (!out) return fail(RPSF_E_BADARG, "null argument");
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
  return RPSF_OK;
}
extern "C" int rpsf_dev_free(int device, void* ptr) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipFree(ptr));
  return RPSF_OK;
}
extern "C" int rpsf_memcpy_h2d(int device, void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return RPSF_OK;
}
extern "C" int rpsf_memcpy_d2h(int device, void* dst, const void* src, size_t bytes) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return RPSF_OK;
}
extern "C" int rpsf_device_synchronize(int device) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------
// RCCL neighbour exchange (loaded lazily so that single-GPU use has no RCCL dependency)
// ------------------------------------------------------------------------------------------------
struct NcclId { char b[128]; };
typedef int (*fn_get_uid)(NcclId*);
typedef int (*fn_comm_init)(void**, int, NcclId, int);
typedef int (*fn_comm_destroy)(void*);
typedef int (*fn_sendrecv)(const void*, size_t, int, int, void*, hipStream_t);
typedef int (*fn_recv)(void*, size_t, int, int, void*, hipStream_t);
typedef int (*fn_group)(void);
typedef int (*fn_allreduce)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef const char* (*fn_errstr)(int);
typedef int (*fn_comm_count)(void*, int*);

static struct {
  void* h;
  fn_get_uid get_uid;
  fn_comm_init comm_init;
  fn_comm_destroy comm_destroy;
  fn_sendrecv send;
  fn_recv recv;
  fn_group group_start, group_end;
  fn_allreduce allreduce;
  fn_errstr errstr;
  fn_comm_count comm_count;
} g_rccl;

static int load_rccl() {
  static std::mutex guard;  // communicators may be created from several threads
  std::lock_guard<std::mutex> lock(guard);
  if (g_rccl.h) return RPSF_OK;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* h = nullptr;
  for (const char* n : names) {
    h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (h) break;
  }
  if (!h) return fail(RPSF_E_RCCL, std::string("cannot load librccl: ") + dlerror());
  g_rccl.get_uid = (fn_get_uid)dlsym(h, "ncclGetUniqueId");
  g_rccl.comm_init = (fn_comm_init)dlsym(h, "ncclCommInitRank");
  g_rccl.comm_destroy = (fn_comm_destroy)dlsym(h, "ncclCommDestroy");
  g_rccl.send = (fn_sendrecv)dlsym(h, "ncclSend");
  g_rccl.recv = (fn_recv)dlsym(h, "ncclRecv");
  g_rccl.group_start = (fn_group)dlsym(h, "ncclGroupStart");
  g_rccl.group_end = (fn_group)dlsym(h, "ncclGroupEnd");
  g_rccl.allreduce = (fn_allreduce)dlsym(h, "ncclAllReduce");
  g_rccl.errstr = (fn_errstr)dlsym(h, "ncclGetErrorString");
  g_rccl.comm_count = (fn_comm_count)dlsym(h, "ncclCommCount");
  if (!g_rccl.get_uid || !g_rccl.comm_init || !g_rccl.comm_destroy || !g_rccl.send || !g_rccl.recv ||
      !g_rccl.group_start || !g_rccl.group_end || !g_rccl.allreduce)
    return fail(RPSF_E_RCCL, "librccl is missing expected symbols");
  g_rccl.h = h;
  return RPSF_OK;
}
#define NCCL_TRY(expr)                                                                               \
  do {                                                                                               \
    int r_ = (expr);                                                                                 \
    if (r_ != 0)                                                                                     \
      return fail(RPSF_E_RCCL, std::string(#expr) + ": " + (g_rccl.errstr ? g_rccl.errstr(r_) : "rccl error")); \
  } while (0)

struct rpsf_comm {
  void* comm = nullptr;
  int device = 0, rank = 0, world = 1;
  hipStream_t stream = nullptr;
  double* d_scalar = nullptr;
};

extern "C" int rpsf_comm_unique_id(void* id128) {
  if (!id128) return fail(RPSF_E_BADARG, "null argument");
  int rc = load_rccl();
  if (rc != RPSF_OK) return rc;
  NCCL_TRY(g_rccl.get_uid(reinterpret_cast<NcclId*>(id128)));
  return RPSF_OK;
}

extern "C" int rpsf_comm_create(rpsf_comm** out, int device, int rank, int world, const void* id128) {
  if (!out || !id128 || rank < 0 || rank >= world) return fail(RPSF_E_BADARG, "bad argument");
  int rc = load_rccl();
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(device));
  auto* c = new rpsf_comm;
  c->device = device, c->rank = rank, c->world = world;
  NcclId id;
  std::memcpy(&id, id128, sizeof(id));
  int r = g_rccl.comm_init(&c->comm, world, id, rank);
  if (r != 0) {
    delete c;
    return fail(RPSF_E_RCCL, std::string("ncclCommInitRank: ") + (g_rccl.errstr ? g_rccl.errstr(r) : "error"));
  }
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc(&c->d_scalar, 2 * sizeof(double));
  if (e != hipSuccess) {
    rpsf_comm_destroy(c);
    return fail(RPSF_E_HIP, hipGetErrorString(e));
  }
  *out = c;
  return RPSF_OK;
}

extern "C" void rpsf_comm_destroy(rpsf_comm* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm && g_rccl.comm_destroy) g_rccl.comm_destroy(c->comm);
  (void)hipFree(c->d_scalar);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

extern "C" int rpsf_comm_seam_exchange_add(rpsf_comm* c, const void* send_dev, size_t send_count, void* recv_dev,
                                           size_t recv_count, void* accum_dev, void* stream) {
  if (!c) return fail(RPSF_E_BADARG, "null comm");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  const bool do_send = c->rank + 1 < c->world && send_count > 0;
  const bool do_recv = c->rank > 0 && recv_count > 0;
  if (do_send || do_recv) {
    NCCL_TRY(g_rccl.group_start());
    if (do_send) NCCL_TRY(g_rccl.send(send_dev, send_count, /*ncclFloat32*/ 7, c->rank + 1, c->comm, st));
    if (do_recv) NCCL_TRY(g_rccl.recv(recv_dev, recv_count, 7, c->rank - 1, c->comm, st));
    NCCL_TRY(g_rccl.group_end());
  }
  if (do_recv) return rpsf_add_rows(c->device, accum_dev, recv_dev, recv_count, st);
  return RPSF_OK;
}

// The exchange alone (no add): for callers that overlap it with the rest of their band's work on another stream
extern "C" int rpsf_comm_seam_exchange(rpsf_comm* c, const void* send_dev, size_t send_count, void* recv_dev, size_t recv_count,
                                       void* stream) {
  if (!c) return fail(RPSF_E_BADARG, "null comm");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
  const bool do_send = c->rank + 1 < c->world && send_count > 0;
  const bool do_recv = c->rank > 0 && recv_count > 0;
  if ((do_send && !send_dev) || (do_recv && !recv_dev)) return fail(RPSF_E_BADARG, "null buffer");
  if (do_send || do_recv) {
    NCCL_TRY(g_rccl.group_start());
    if (do_send) NCCL_TRY(g_rccl.send(send_dev, send_count, /*ncclFloat32*/ 7, c->rank + 1, c->comm, st));
    if (do_recv) NCCL_TRY(g_rccl.recv(recv_dev, recv_count, 7, c->rank - 1, c->comm, st));
    NCCL_TRY(g_rccl.group_end());
  }
  return RPSF_OK;
}
extern "C" void* rpsf_comm_stream(rpsf_comm* c) { return c ? (void*)c->stream : nullptr; }

// How many ranks RCCL itself counts in the communicator (ncclCommCount): what a harness prints next to its timings to show that the
// collective path really spans the GPUs it was launched on
extern "C" int rpsf_comm_ranks(rpsf_comm* c, int* ranks) {
  if (!c || !ranks) return fail(RPSF_E_BADARG, "null argument");
  if (!g_rccl.comm_count) return fail(RPSF_E_RCCL, "librccl has no ncclCommCount");
  NCCL_TRY(g_rccl.comm_count(c->comm, ranks));
  return RPSF_OK;
}

// Work enqueued on `waiter` after this call starts only when everything enqueued on `signaller` so far has finished
extern "C" int rpsf_stream_wait(int device, void* waiter, void* signaller) {
  HIP_TRY(hipSetDevice(device));
  hipEvent_t ev = nullptr;
  HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, reinterpret_cast<hipStream_t>(signaller));
  if (e == hipSuccess) e = hipStreamWaitEvent(reinterpret_cast<hipStream_t>(waiter), ev, 0);
  (void)hipEventDestroy(ev);  // released once the recorded work has completed
  if (e != hipSuccess) return fail(RPSF_E_HIP, hipGetErrorString(e));
  return RPSF_OK;
}

extern "C" int rpsf_stream_synchronize(int device, void* stream) {
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
  return RPSF_OK;
}

// Events for callers that order work across their streams at a distance (the sharded step: "this launch may start once the add of two
// steps ago has read the buffer it writes" - a dependency that rpsf_stream_wait, which records at the time of the call, cannot express)
extern "C" int rpsf_event_create(int device, void** event) {
  if (!event) return fail(RPSF_E_BADARG, "null argument");
  HIP_TRY(hipSetDevice(device));
  hipEvent_t ev = nullptr;
  HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  *event = ev;
  return RPSF_OK;
}
extern "C" int rpsf_event_record(void* event, void* stream) {
  if (!event) return fail(RPSF_E_BADARG, "null event");
  HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(event), reinterpret_cast<hipStream_t>(stream)));
  return RPSF_OK;
}
extern "C" int rpsf_stream_wait_event(void* stream, void* event) {
  if (!event) return fail(RPSF_E_BADARG, "null event");
  HIP_TRY(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), reinterpret_cast<hipEvent_t>(event), 0));
  return RPSF_OK;
}
extern "C" int rpsf_event_destroy(void* event) {
  if (event) HIP_TRY(hipEventDestroy(reinterpret_cast<hipEvent_t>(event)));
  return RPSF_OK;
}

// accum[0:count] += src[0:count] on `device` (kernel K4; the add of the seam exchange, exported for callers that move
// the seam rows themselves)
static int add_rows_impl(int device, void* accum_dev, const void* src_dev, size_t count, int max_workgroups, void* stream) {
  if (!accum_dev || !src_dev) return fail(RPSF_E_BADARG, "null argument");
  if (count == 0) return RPSF_OK;
  HIP_TRY(hipSetDevice(device));
  const int block = 256;
  size_t grid = ((count + 3) / 4 + block - 1) / block;
  if (max_workgroups > 0) grid = std::min<size_t>(grid, (size_t)max_workgroups);
  add_rows_kernel<<<dim3((unsigned)grid), dim3(block), 0, reinterpret_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<float*>(accum_dev), reinterpret_cast<const float*>(src_dev), count);
  HIP_TRY(hipGetLastError());
  return RPSF_OK;
}
extern "C" int rpsf_add_rows(int device, void* accum_dev, const void* src_dev, size_t count, void* stream) {
  return add_rows_impl(device, accum_dev, src_dev, count, 0, stream);
}
// The same add on at most `max_workgroups` workgroups (grid-stride): for callers that run it BESIDE a persistent patch launch (the pipelined
// seam exchange) - a patch workgroup needs a whole CU, and a thousand small workgroups dispatched a moment before it would each hold one
extern "C" int rpsf_add_rows_narrow(int device, void* accum_dev, const void* src_dev, size_t count, int max_workgroups, void* stream) {
  if (max_workgroups <= 0) return fail(RPSF_E_BADARG, "max_workgroups must be positive");
  return add_rows_impl(device, accum_dev, src_dev, count, max_workgroups, stream);
}

extern "C" int rpsf_comm_allreduce_max(rpsf_comm* c, double* value) {
  if (!c || !value) return fail(RPSF_E_BADARG, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(c->d_scalar, value, sizeof(double), hipMemcpyHostToDevice, c->stream));
  NCCL_TRY(g_rccl.allreduce(c->d_scalar, c->d_scalar + 1, 1, /*ncclFloat64*/ 8, /*ncclMax*/ 2, c->comm, c->stream));
  HIP_TRY(hipMemcpyAsync(value, c->d_scalar + 1, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RPSF_OK;
}

extern "C" int rpsf_comm_barrier(rpsf_comm* c, void* stream) {
  if (!c) return fail(RPSF_E_BADARG, "null comm");
  HIP_TRY(hipSetDevice(c->device));
  if (stream) HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
  double v = 0.0;
  return rpsf_comm_allreduce_max(c, &v);
}
