// rpsf.hip - the plan of librpsf_hip.so: its creation and destruction, the lattice setup, the transfer-kernel install, the geometry
// check, the whole launch path of an apply (decide / commit / fill / launch), the option setters, the device-resident entry points
// (rpsf_apply_device, rpsf_apply_batch_device and the timed ones) and the hipFFT loader of the fallback; the error message of the
// calling thread lives here too.  The rest of the host side: rpsf_host.hip (host-array pipelines), rpsf_saturated.hip (saturation routes and
// device-array views), rpsf_construct.hip (K2 / K3 entry points), rpsf_shard.hip (device memory, RCCL, streams and events); what they share
// with this file is rpsf_plan.hpp.  The device code is in rpsf_kernels.hpp (kernels) and rpsf_core.hpp (per-thread phases).  What follows from a corner
// list and a frame geometry alone - lattice tables, processing order, row bands, the geometry predicates of the launch forms - is plain
// C++ in rpsf_lattice.hpp (as the job lists of the sweep kernel are in rpsf_plan3.hpp): this file uploads what those return.
//
// Kernels launched here (rpsf_kernels.hpp, rpsf_kernels2.hpp, rpsf_kernels3.hpp; the plain ones of rpsf_kernels_plan.hpp are defined in this unit):
//   patch_kernel<C>        K1: fused gather+pad+window -> 2-D DFT -> x folded K -> inverse DFT -> window ->
//                          overlap-add; one workgroup per patch (or several small patches per workgroup),
//                          patch resident in registers, LDS used only for the inter-stage transposes.
//                          Stands in for regularizepsf/transform.py:151-169.
//   pack_kernel<C>         folds K to K_h = (K(k)+conj K(-k))/2 and re-orders it into the per-thread
//                          streaming layout of K1 (one-time, at set_transfer).
//   sum_planes_kernel      K5: output = sum of the four colour planes the patches of one parity class write.
//   fixup_kernel           K5': the sides of a direct overlap-add launch.
//   generic_*_kernel       gather / multiply / scatter around hipFFT for patch sizes without a plan.
// Development-only build switches (never set by regularizepsf_amd/build.py): RPSF_STAMPS / RPSF_WAVE_STAMPS (per-phase
// timestamps, scripts/stamps.py) and the RPSF2_ABL_* timing ablations of rpsf_kernels2.hpp (results are wrong, timing only).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "rpsf_plan.hpp"
#include "rpsf_kernels_plan.hpp"

// ------------------------------------------------------------------------------------------------
// error plumbing (fail / HIP_TRY: rpsf_side_unit.hpp, for every unit; the message they set is this one)
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
int rpsf_detail_fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

extern "C" const char* rpsf_last_error(void) { return g_err.c_str(); }

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

// The plan's error word: page-locked, set by a kernel whose bounded wait ran out (1: the sweep kernel's jobs, 2: the gate of the persistent 256-pixel
// kernel) and read by rpsf_detail_sweep_check.  A view's kernels report through its parent's word.
static int ensure_error_word(rpsf_plan* p) {
  SweepPath& sw = p->sweep;
  if (p->parent || sw.err) return RPSF_OK;
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&sw.err.p), 64, hipHostMallocMapped));
  std::memset(sw.err, 0, 64);
  HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&sw.d_err), sw.err, 0));
  return RPSF_OK;
}

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
  if (const int rc = ensure_error_word(p); rc != RPSF_OK) return rc;
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
    // (queue words: a set per launch lane - two launches that draw at once must not take each other's positions, rpsf_lanes.hpp)
    HIP_TRY(p->patch.d_sum_queue.alloc(2 * 32));
    HIP_TRY(hipMemset(p->patch.d_sum_queue, 0, 2 * 32 * sizeof(uint32_t)));
    HIP_TRY(p->patch.d_xq.alloc(2 * 8 * 32));
    HIP_TRY(hipMemset(p->patch.d_xq, 0, 2 * 8 * 32 * sizeof(uint32_t)));
    HIP_TRY(p->patch.d_tile_summed.alloc(t.sum_order.size()));
    HIP_TRY(hipMemset(p->patch.d_tile_summed, 0, t.sum_order.size() * sizeof(uint32_t)));
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
int rpsf_detail_plan_create_impl(rpsf_plan** out, int device, int patch_size, int n_patches, const int32_t* coords_rc, rpsf_plan* parent,
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
    if (p->patch.v2 && N == 256) {  // the gated kernel reports a wait that ran out; a plan that is not a view gets the second lane (RPSF_OPT_PIPELINE)
      rl = ensure_error_word(p);
      if (rl != RPSF_OK) return rl;
      if (!parent && p->lattice) {
        HIP_TRY(hipStreamCreateWithFlags(&p->lane1, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&p->ev_lane, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
        p->patch.lanes.enabled = true;
      }
    }
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
  return rpsf_detail_plan_create_impl(out, device, patch_size, n_patches, coords_rc, nullptr, nullptr);
}

// Join the launch lanes of the plan (of a view: its parent's): the public stream waits for what the second lane holds, and whatever is enqueued on
// the public stream next runs behind every apply so far, as it always did (rpsf_lanes.hpp).  Costs nothing while the second lane is idle.
int rpsf_detail_join_lanes(rpsf_plan* p) {
  rpsf_plan* r = p->parent ? p->parent : p;
  if (!r->patch.lanes.join()) return RPSF_OK;
  HIP_TRY(hipSetDevice(r->device));
  HIP_TRY(hipEventRecord(r->ev_lane, r->lane1));
  HIP_TRY(hipStreamWaitEvent(r->stream, r->ev_lane, 0));
  return RPSF_OK;
}

// The host-array, saturation and mask entry points start with a clean error word: an error a caller of the device entry points never collected
// is not theirs, and is dropped here.  Called behind the join of the lanes; device applies the caller left in flight are waited for first (the
// public stream covers both lanes then), so that a wait of theirs that runs out is neither blamed on this call nor wiped half-way.
void rpsf_detail_clear_error(rpsf_plan* p) {
  rpsf_plan* r = p->parent ? p->parent : p;
  volatile uint32_t* word = r->sweep.err;
  if (!word) return;
  if (r->busy_valid && r->stream) (void)hipStreamSynchronize(r->stream);
  *word = 0;
}

// The handle of the public stream.  What the caller enqueues there is unknown to the plan, so from here on its applies stay on that one stream.
extern "C" void* rpsf_plan_stream(rpsf_plan* p) {
  if (!p) return nullptr;
  (void)rpsf_detail_join_lanes(p);
  (p->parent ? p->parent : p)->patch.lanes.exposed = true;
  return (void*)p->stream;
}

extern "C" void rpsf_plan_destroy(rpsf_plan* p) { delete p; }

void rpsf_detail_drop_bands(rpsf_plan* p) {
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
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;  // (rpsf_lanes.hpp: everything but a pipelined apply joins first)
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
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;  // (rpsf_lanes.hpp: everything but a pipelined apply joins first)
  return install_transfer(p, KSource{reinterpret_cast<const cf*>(k_dev)}, 0, p->n_patches);
}

// construct -> pack in one pass: complex64 spectra of the plan's patches on its device
extern "C" int rpsf_plan_set_transfer_spectra_device(rpsf_plan* p, const void* s_c64_dev, const void* t_c64_dev, double alpha, double epsilon) {
  if (!p || !s_c64_dev || !t_c64_dev) return fail(RPSF_E_BADARG, "null argument");
  HIP_TRY(hipSetDevice(p->device));
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;  // (rpsf_lanes.hpp: everything but a pipelined apply joins first)
  return install_transfer(p, KSource{nullptr, hipMemcpyDeviceToDevice, reinterpret_cast<const cf*>(s_c64_dev), reinterpret_cast<const cf*>(t_c64_dev),
                                     alpha, epsilon}, 0, p->n_patches);
}

extern "C" int rpsf_plan_transfer_bytes(const rpsf_plan* p, size_t* bytes) {
  if (!p || !bytes) return fail(RPSF_E_BADARG, "null argument");
  // (the representation the plan's applies read: the third generation's when the sweep kernel runs them)
  if (p->generic) *bytes = (size_t)p->N * p->N * p->n_patches * sizeof(cf);
  else if (p->sweep.ok && rpsf_detail_overlap_kind(p) == OV_SWEEP) *bytes = p->sweep.k3_floats * sizeof(float);
  else *bytes = (p->patch.g_elems + p->patch.gs_elems) * sizeof(cf);
  return RPSF_OK;
}

int rpsf_detail_check_geometry(const rpsf_plan* p, const rpsf_geometry* g) {
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

// Whether the plan's lattice tiles cover the resident output window (rpsf_lattice.hpp): where they do not, the window is cleared first
bool rpsf_detail_lattice_covers_window(const rpsf_plan* p, const rpsf_geometry& g) {
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

// What the persistent kernels are compiled for (hot_geometry, rpsf_lattice.hpp), for this plan, image and frame stride
static bool hot_geometry(const rpsf_plan* p, const float* d_img, const rpsf_geometry& g, size_t im_stride) {
  const bool aligned16 = im_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(d_img) & 15) == 0 && p->patch.planes_floats % 4 == 0;
  return hot_geometry(g, p->lattice, p->lat_c0, aligned16);
}

// What the patch launch of one apply is: decided by patch_launch_for from the plan as it stands, committed by launch_apply (the queue positions the
// launch takes) and turned into PatchParams and a kernel by launch_patches.
struct PatchLaunch : LaunchDecision {  // (rpsf_launch.hpp: the form, the grid, the workgroups of each role and the draws from every queue word)
  uint32_t xq_base[8];      // persistent: where this launch's draws from the slot queue of each XCD start
  uint32_t sum_queue_base;  // fused and persistent: the same for the tile queue
  // the launch lane (rpsf_lanes.hpp, committed by launch_apply): whose queue words the launch draws from, what its tile sums publish and whether its
  // patches wait for the previous apply's
  int lane;
  bool gate;
  uint32_t seq;
};

// The plan and the apply as launch_decide (rpsf_launch.hpp) sees them; the arithmetic - and the FORWARD PROGRESS argument of the persistent form - is there.
// fused: the plane sum runs in this launch (see PatchPath::d_tile_done)
template <class T>
static PatchLaunch patch_launch_for(const rpsf_plan* p, const float* d_img, const rpsf_geometry& g, Batch b, bool fused) {
  constexpr bool N256 = T::V2 && T::Cfg::N == 256;
  LaunchInput in;
  in.N = p->N, in.gen2 = T::V2, in.wg_threads = T::WG;
  in.n_patches = p->n_patches, in.tiles = p->nti * p->ntj, in.frames = b.frames;
  in.cu_count = p->cu_count, in.round_capacity = p->patch.round_capacity;
  in.wgs_per_cu = std::max(1, p->patch.round_capacity / (std::max(1, p->cu_count) * T::TEAMS));  // (rpsf_plan_create: the occupancy of the patch kernel)
  in.reserved_cus = p->patch.reserved_cus, in.sum_first = p->patch.sum_first, in.head_patches = p->patch.head_patches;
  in.persist = p->patch.persist, in.fused = fused;
  in.hot_geometry = fused && hot_geometry(p, d_img, g, b.im_stride);
  // (the gated kernel - the persistent 256-pixel one - stores the output through one 32-bit buffer offset, as every fused launch does its planes)
  in.out_span_ok = !N256 || (size_t)g.out_rows * g.ld_out * sizeof(float) < ((size_t)1 << 32);
  in.planes_floats = p->patch.planes_floats, in.k_cached = p->patch.k_cached, in.plane_nt_opt = p->patch.plane_nt_opt;
  if (const char* e = dev_env("RPSF_FRAME_MAJOR")) in.frame_major_opt = std::atoi(e) == 2 ? 2 : std::atoi(e) != 0 ? 1 : 0;  // development sweeps: 0 = never, 2 = any persistent batch
  in.stagger_us = p->patch.stagger_us;
  in.prefetch = p->patch.prefetch && p->patch.d_prefetch_tiles, in.k_prefetch = p->patch.k_prefetch;
  PatchLaunch L{};
  static_cast<LaunchDecision&>(L) = launch_decide(in);
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
  ts.done = p->patch.d_tile_done, ts.epoch = p->patch.lanes.done_epoch;
  ts.n_frames = b.frames, ts.n_tiles = (uint32_t)n_tiles, ts.n_tiles_listed = (uint32_t)n_tiles, ts.frame_major = L.frame_major;
  ts.queue = p->patch.d_sum_queue + L.lane * 32, ts.queue_base = L.sum_queue_base;
  ts.summed = p->patch.d_tile_summed, ts.seq = L.seq;  // (read by the gated kernel alone, like the next three)
  ts.gate_on = L.gate ? 1u : 0u, ts.gate_want = L.seq - 1, ts.err = o->sweep.d_err;
  if (L.form != PatchLaunch::PERSISTENT) return pp;
  pp.persist = L.rows, pp.xq = p->patch.d_xq + L.lane * 8 * 32;
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

OverlapKind rpsf_detail_overlap_kind(const rpsf_plan* p) {
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
      if (p->fft.d_colour && rpsf_detail_overlap_kind(p) != OV_ATOMIC) {
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
  if (const int rc = rpsf_detail_lattice_covers_window(p, g) ? RPSF_OK : clear_window(d_out, g, b, st); rc != RPSF_OK) return rc;
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
// may_pipeline: the caller is an entry point that leaves the stream to the plan and enqueues nothing behind the apply itself (rpsf_apply_device,
// rpsf_apply_device_loop_ms) - such an apply may take the plan's second lane (rpsf_lanes.hpp); every other apply joins the lanes first.
int rpsf_detail_launch_apply(rpsf_plan* p, const float* d_img, float* d_out, const rpsf_geometry& g, hipStream_t st,
                             hipEvent_t ev_k0, hipEvent_t ev_k1, Batch b, bool may_pipeline) {
  // (a view joins its parent's lanes - it runs on the parent's stream - and has none of its own; for the applies that may be pipelined the lane
  // book decides below, once the form of the launch is known)
  if (!may_pipeline || p->parent || !p->patch.lanes.enabled)
    if (const int rc = rpsf_detail_join_lanes(p); rc != RPSF_OK) return rc;
  if (p->generic) return launch_apply_generic(p, d_img, d_out, g, st, ev_k0, ev_k1, b);
  const OverlapKind kind = rpsf_detail_overlap_kind(p);
  if (kind == OV_SWEEP) {
    if (!p->sweep.ok) return fail(RPSF_E_STATE, "the sweep kernel needs a 16-, 32- or 64-pixel patch on a complete lattice of at least 2 x 2 patches");
    return launch_sweep(p, d_img, d_out, g, st, ev_k0, ev_k1, b);
  }
  if (kind != OV_ATOMIC && !p->lattice) return fail(RPSF_E_STATE, "colour planes need a regular half-overlap lattice of patch corners");
  if (kind == OV_DIRECT && !p->patch.direct_ok) return fail(RPSF_E_STATE, "direct overlap-add needs a lattice and a 128- or 256-pixel patch");
  if (kind == OV_DIRECT && (size_t)g.out_rows * g.ld_out * sizeof(float) >= ((size_t)1 << 32))
    return fail(RPSF_E_UNSUPPORTED, "direct overlap-add addresses the output through a 32-bit buffer offset: frame too large");
  if (patch_launch_too_large(p->N, p->n_patches, b.frames)) return fail(RPSF_E_BADARG, "batch too large for one launch");
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
  // atomics accumulate into the output; the tile sums and the direct mode's fix-up write lattice tiles only
  const bool clear = kind == OV_ATOMIC || ((kind == OV_DIRECT || fused) && !rpsf_detail_lattice_covers_window(p, g));
  // ---- nothing refuses the launch from here on: the plan's lanes, epochs, counters and queue positions advance ----
  // The lane (rpsf_lanes.hpp).  Two applies of the plan may be in flight only when both run the gated kernel - the persistent 256-pixel one, whose
  // tile sums and patches order every tile between them - on a single frame, on the plan's own stream, with nothing else enqueued around the
  // launch: no clear of the output, no restart of the tile counters, no timing events, no other stream to serialise against.
  const bool gated_kernel = L.form == PatchLaunch::PERSISTENT && p->patch.v2 && p->N == 256;
  const bool hot = may_pipeline && gated_kernel && !p->parent && b.frames == 1 && st == p->stream && !p->multi_stream && !clear && !ev_k0 && !ev_k1 &&
                   !p->patch.lanes.epoch_restarts(b.frames);
  const LaneRange img_range{reinterpret_cast<uintptr_t>(d_img),
                            reinterpret_cast<uintptr_t>(d_img + (size_t)std::max(0, g.image_rows - 1) * g.ld_image + g.width)};
  const LaneRange out_range{reinterpret_cast<uintptr_t>(d_out), reinterpret_cast<uintptr_t>(d_out + (size_t)std::max(0, g.out_rows - 1) * g.ld_out + g.width)};
  LaneLayout layout;
  layout.v[0] = g.width, layout.v[1] = g.out_row0, layout.v[2] = g.out_rows, layout.v[3] = g.origin_row, layout.v[4] = g.origin_col;
  layout.v[5] = (int64_t)p->patch.planes_floats;
  const LaneBook book_before = p->patch.lanes;
  const LanePick pick = p->patch.lanes.begin(hot, gated_kernel, img_range, out_range, layout);
  {  // (a stream operation that fails leaves no launch behind: the book goes back to where it was, or the next gate would wait for nobody)
    hipError_t e = hipSuccess;
    if (pick.join) {  // (only a plan with a second lane can have it busy)
      e = hipEventRecord(p->ev_lane, p->lane1);
      if (e == hipSuccess) e = hipStreamWaitEvent(p->stream, p->ev_lane, 0);
    }
    if (e == hipSuccess && pick.fork) e = hipEventRecord(p->ev_fork, p->stream);
    if (e == hipSuccess && pick.wait_fork) e = hipStreamWaitEvent(p->lane1, p->ev_fork, 0);
    if (e != hipSuccess) {
      p->patch.lanes = book_before;
      (void)hipDeviceSynchronize();  // (whatever the lanes hold is over before anything else runs: the restored book may say "joined" or not)
      p->patch.lanes.join();
      return fail(RPSF_E_HIP, std::string("launch lanes: ") + hipGetErrorString(e));
    }
  }
  hipStream_t run = pick.lane == 1 ? p->lane1 : st;  // (everything below but the patch launch of a pipelined apply is enqueued on st == run)
  L.lane = pick.lane, L.gate = pick.gate, L.seq = pick.seq, L.sum_queue_base = pick.sum_queue_base;
  for (int x = 0; x < 8; ++x) L.xq_base[x] = pick.xq_base[x];
  LaneDraws draws;
  for (int x = 0; x < 8; ++x) draws.xq[x] = L.xq_draws[x];
  draws.sum = L.sum_queue_draws;
  p->patch.lanes.commit(pick, draws);
  if (kind == OV_DIRECT && ++p->patch.epoch >= (1u << 24) - 1) {  // the epoch field of the flag words is 24 bits wide
    HIP_TRY(hipMemsetAsync(p->patch.d_flags, 0, n_tiles * p->patch.flag_frames * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(p->patch.d_chunk_xcc, 0, 8 * sizeof(uint32_t), st));
    p->patch.epoch = 1;
  }
  if (fused) {
    // A launch advances the counters of frames [0, b.frames) only, and a tile is complete at epoch x contributors: when the frame
    // count differs from the previous fused launch's (batch -> single apply -> batch, or the short last group of a batch) the
    // counters of the higher frames would lag behind the epoch for ever - and the summing workgroups would wait for ever.
    // Start a new count whenever the frame count changes (and when the epoch would overflow the counters): LaneBook::next_epoch.
    // (such a launch is never pipelined: the lanes are joined, the clear runs behind every earlier apply)
    if (p->patch.lanes.next_epoch(b.frames).restart)
      HIP_TRY(hipMemsetAsync(p->patch.d_tile_done, 0, n_tiles * p->patch.done_frames * sizeof(uint32_t), st));
  }
  if (const int rc = clear ? clear_window(d_out, g, b, st) : RPSF_OK; rc != RPSF_OK) return rc;
  if (ev_k0) HIP_TRY(hipEventRecord(ev_k0, st));
  int rc = launch_patches(p, L, d_img, d_out, g, kind, run, b);
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
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;
  p->overlap_mode = mode;
  rpsf_detail_drop_bands(p);
  return RPSF_OK;
}

extern "C" int rpsf_plan_set_option(rpsf_plan* p, int option, int value) {
  if (!p) return fail(RPSF_E_BADARG, "null plan");
  if (const int rc = rpsf_detail_join_lanes(p); rc != RPSF_OK) return rc;
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
    case RPSF_OPT_PIPELINE:
      if (value != 0 && value != 1) return fail(RPSF_E_BADARG, "RPSF_OPT_PIPELINE takes 0 or 1");
      if (p->parent) return fail(RPSF_E_STATE, "a view runs on its parent's stream");
      p->patch.lanes.enabled = value != 0 && p->lane1 != nullptr;  // (plans without the gated kernel have one lane whatever the option says)
      // (setting it to 1 is the caller's word that nothing of theirs is enqueued on the plan's stream any more: a plan that went to one lane
      // because its stream handle was taken - rpsf_plan_stream - is armed again; a CU mask keeps it on one lane, see rpsf_plan_set_cu_mask)
      if (value != 0) p->patch.lanes.exposed = false;
      break;
    case RPSF_OPT_DEBUG_ORPHAN:
      if (value < 0) return fail(RPSF_E_BADARG, "RPSF_OPT_DEBUG_ORPHAN takes 0 (off) or a positive modulus");
      p->patch.orphan_mod = value;
      break;
    default: return fail(RPSF_E_BADARG, "unknown plan option");
  }
  rpsf_detail_drop_bands(p);  // (views inherit nothing: they are rebuilt with the parent's settings at the next host frame)
  return RPSF_OK;
}

extern "C" int rpsf_plan_set_sweep_regions(rpsf_plan* p, int target_regions) {
  if (!p || target_regions < 1 || target_regions > (1 << 20)) return fail(RPSF_E_BADARG, "target_regions must be 1..2^20");
  if (!p->sweep.ok) return fail(RPSF_E_STATE, "the sweep kernel needs a 16-, 32- or 64-pixel patch on a complete lattice of at least 2 x 2 patches");
  HIP_TRY(hipSetDevice(p->device));
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;  // (rpsf_lanes.hpp: everything but a pipelined apply joins first)
  HIP_TRY(hipStreamSynchronize(p->stream));
  HIP_TRY(hipDeviceSynchronize());  // (applies on other streams may still read the old lists)
  rpsf_detail_drop_bands(p);
  return build_sweep_lists(p, target_regions);
}
extern "C" int rpsf_plan_host_bands(const rpsf_plan* p, int* bands) {
  if (!p || !bands) return fail(RPSF_E_BADARG, "null argument");
  *bands = p->last_host_bands;
  return RPSF_OK;
}
// The lane report: what the lane book (rpsf_lanes.hpp) has decided so far.  Reads host fields only - no stream operation, no join.
extern "C" int rpsf_plan_lane_info(const rpsf_plan* p, long info[6]) {
  if (!p || !info) return fail(RPSF_E_BADARG, "null argument");
  (p->parent ? p->parent : p)->patch.lanes.info(info);
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
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;  // (rpsf_lanes.hpp: everything but a pipelined apply joins first)
  HIP_TRY(hipStreamSynchronize(p->stream));
  rpsf_detail_drop_bands(p);
  hipStream_t masked = nullptr;
  HIP_TRY(hipExtStreamCreateWithCUMask(&masked, (uint32_t)words, mask));
  if (p->generic && g_hipfft.set_stream(p->fft.plan.get(), masked) != 0) {
    (void)hipStreamDestroy(masked);
    return fail(RPSF_E_HIP, "hipfftSetStream failed");
  }
  (void)hipStreamDestroy(p->stream);
  p->stream = masked;
  p->busy_valid = false;
  // Every launch of the plan stays inside the mask: the second launch lane is an unmasked stream, so a masked plan keeps to one lane, for good
  // (the lanes were joined above; RPSF_OPT_PIPELINE cannot switch them back on without the stream).
  p->patch.lanes.enabled = false;
  if (p->lane1) {
    (void)hipStreamSynchronize(p->lane1);
    (void)hipStreamDestroy(p->lane1);
    p->lane1 = nullptr;
  }
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
  rpsf_detail_drop_bands(p);
  return RPSF_OK;
}


extern "C" int rpsf_apply_device(rpsf_plan* p, const void* image_dev, void* out_dev, const rpsf_geometry* geom,
                                 void* stream) {
  if (!p || !image_dev || !out_dev) return fail(RPSF_E_BADARG, "null argument");
  if (!p->have_k) return fail(RPSF_E_STATE, "no transfer kernel installed (call rpsf_plan_set_transfer first)");
  int rc = rpsf_detail_check_geometry(p, geom);
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : p->stream;
  // (stream == NULL leaves the stream to the plan: back-to-back applies of a 256-pixel plan may then overlap head under tail, rpsf_lanes.hpp)
  return rpsf_detail_launch_apply(p, reinterpret_cast<const float*>(image_dev), reinterpret_cast<float*>(out_dev), *geom, st, nullptr, nullptr, Batch(),
                                  /*may_pipeline*/ stream == nullptr);
}


// Frames per launch group: the colour planes take 16 bytes per output pixel per frame in flight; keep
// them under a quarter of the device memory.  (One frame is one group: nothing is asked of the device.)
static int batch_group_frames(const rpsf_plan* p, const rpsf_geometry& g, int n_frames) {
  if (n_frames == 1 || p->generic || rpsf_detail_overlap_kind(p) == OV_ATOMIC || rpsf_detail_overlap_kind(p) == OV_SWEEP) return n_frames;
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
  int rc = rpsf_detail_check_geometry(p, geom);
  if (rc != RPSF_OK) return rc;
  if (n_frames > 1 && (im_stride < (size_t)(geom->image_rows - 1) * geom->ld_image + geom->width ||
                       out_stride < (size_t)(geom->out_rows - 1) * geom->ld_out + geom->width))
    return fail(RPSF_E_BADARG, "frame stride smaller than one frame");
  return RPSF_OK;
}

int rpsf_detail_launch_batch(rpsf_plan* p, const float* d_imgs, float* d_outs, int n_frames, size_t im_stride, size_t out_stride,
                             const rpsf_geometry& g, hipStream_t st, hipEvent_t ev_k0, hipEvent_t ev_k1) {
  const int group = batch_group_frames(p, g, n_frames);
  for (int f0 = 0; f0 < n_frames; f0 += group) {
    Batch b;
    b.frames = std::min(group, n_frames - f0), b.im_stride = im_stride, b.out_stride = out_stride;
    const bool first = f0 == 0, last = f0 + group >= n_frames;
    // (with several groups the kernel-time bracket covers everything between the first group's patch launch
    //  and the last group's, plane sums of the earlier groups included)
    int rc = rpsf_detail_launch_apply(p, d_imgs + (size_t)f0 * im_stride, d_outs + (size_t)f0 * out_stride, g, st,
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
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;  // (rpsf_lanes.hpp: everything but a pipelined apply joins first)
  hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : p->stream;
  return rpsf_detail_launch_batch(p, reinterpret_cast<const float*>(images_dev), reinterpret_cast<float*>(outs_dev), n_frames,
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
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;  // (rpsf_lanes.hpp: everything but a pipelined apply joins first)
  return timed_loop(p, iters, total_ms, kernel_ms, [&](hipEvent_t k0, hipEvent_t k1) {
    return rpsf_detail_launch_batch(p, reinterpret_cast<const float*>(images_dev), reinterpret_cast<float*>(outs_dev), n_frames, image_stride,
                        out_stride, *geom, p->stream, k0, k1);
  });
}

// The sweep kernel bounds every wait of a job for its predecessors (a protocol error must not hang the GPU) and reports a wait that ran out through a
// page-locked word; every entry point that has just waited for the plan's work looks at it, so such an apply fails instead of returning a wrong image.
int rpsf_detail_sweep_check(rpsf_plan* p) {
  volatile uint32_t* word = owner(p)->sweep.err;
  if (!word || *word == 0) return RPSF_OK;
  const uint32_t what = *word;
  *word = 0;
  if (what == 2)
    return fail(RPSF_E_HIP, "patch kernel: an apply waited for the tile sums of the plan's previous apply beyond the bound (internal protocol error; the output of this apply is not valid)");
  return fail(RPSF_E_HIP, "sweep kernel: a job waited for the jobs it follows beyond the bound (internal protocol error; the output of this apply is not valid)");
}

// The way out of a host-array entry point (rpsf_host.hip, rpsf_saturated.hip) after a failed copy or launch; here because it reads the message
int rpsf_detail_drain_after_error(rpsf_plan* p, hipError_t err, const char* where) {
  (void)hipStreamSynchronize(p->pipe->st_in);
  (void)hipStreamSynchronize(p->stream);
  (void)hipStreamSynchronize(p->pipe->st_out);
  if (err == hipErrorUnknown && !g_err.empty()) return RPSF_E_HIP;  // launch_apply already set the message
  return fail(RPSF_E_HIP, std::string(where) + ": " + hipGetErrorString(err));
}

extern "C" int rpsf_apply_device_timed(rpsf_plan* p, const void* image_dev, void* out_dev, const rpsf_geometry* geom,
                                       int iters, float* total_ms, float* kernel_ms) {
  if (!p || !image_dev || !out_dev || iters <= 0) return fail(RPSF_E_BADARG, "bad argument");
  if (!p->have_k) return fail(RPSF_E_STATE, "no transfer kernel installed (call rpsf_plan_set_transfer first)");
  int rc = rpsf_detail_check_geometry(p, geom);
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;  // (rpsf_lanes.hpp: everything but a pipelined apply joins first)
  return timed_loop(p, iters, total_ms, kernel_ms, [&](hipEvent_t k0, hipEvent_t k1) {
    return rpsf_detail_launch_apply(p, reinterpret_cast<const float*>(image_dev), reinterpret_cast<float*>(out_dev), *geom, p->stream, k0, k1);
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
  int rc = rpsf_detail_check_geometry(p, geom);
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  // (the event pair brackets both launch lanes: the start is recorded behind a join, and the lanes are joined again in front of the stop; the
  // applies in between are the ones rpsf_apply_device makes)
  rc = rpsf_detail_join_lanes(p);
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipEventRecord(p->ev[0], p->stream));
  for (int i = 0; i < iters; ++i) {
    rc = rpsf_detail_launch_apply(p, reinterpret_cast<const float*>(image_dev), reinterpret_cast<float*>(out_dev), *geom, p->stream, nullptr, nullptr,
                                  Batch(), /*may_pipeline*/ true);
    if (rc != RPSF_OK) return rc;
  }
  rc = rpsf_detail_join_lanes(p);
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipEventRecord(p->ev[3], p->stream));
  HIP_TRY(hipEventSynchronize(p->ev[3]));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, p->ev[0], p->ev[3]));
  *ms_per_apply = (double)ms / iters;
  return rpsf_detail_sweep_check(p);
}
