// stars.hip - find_stars: star positions for the PSF builder.  The detector is this project's own definition,
// modelled on sep.Background + sep.extract without deblending; it is NOT sep.
//
//   S1  stars_mesh_kernel      one workgroup per background box: sigma-clipped level and rms (exact median, fixed-order sums)
//   S1b stars_mesh_filter_kernel   the mesh filled and 3 x 3 median filtered on the device, global rms and T with it (the drivers of
//                              rpsf_core_stars_mesh.hpp): one workgroup, or above rpsfm::MANY_NODES nodes the stars_mesh_many_* launches
//   S2  stars_detect_kernel    one workgroup per 32 x 32 tile: residual against the bilinear background surface (mesh window and
//                              the tile with a one-pixel halo in LDS), 3 x 3 filter, test against T -> one mask byte per pixel
//   S3  stars_label_*          union-find per tile in LDS, integer atomicMin across tile seams, flatten:
//                              every detected pixel ends with the smallest linear index of its component, the rest with -1
//   S4  stars_count/scan/roots the roots in index order; stars_init/accumulate: area and bounding box by integer atomics;
//       stars_walk_kernel      one wave per component of an accepted area: float64 moments over its bounding box, fixed tree
//
//   D1 - D4 deblend_*         the deblend option (rpsf_stars_set_deblend; off by default, and then none of this runs): S2 also stores
//                              the filtered residual; ascent to the peaks, basins, significance, ownership, moments per object
//                              (the drivers of rpsf_core_stars_deblend.hpp)
//
//   S5  stars_shape_kernel     rpsf_stars_measure, and only then: one wave per row of the last detect, a second walk around the finished
//                              centroid for central second moments, sum |d| and the peak (the driver of rpsf_core_stars_shape.hpp)
//
//   S6  stars_photometry_kernel   rpsf_stars_photometry, and only then: one wave per position the caller supplies, circular apertures with
//                              sub-pixel coverage on the frame and the filtered mesh of the fused route (the driver of
//                              rpsf_core_stars_photometry.hpp); it writes its own rows and nothing the other kernels read
//
//   S7  stars_refine_kernel    rpsf_stars_refine, and only then: one wave per position the caller supplies, the Gaussian-windowed
//                              position iterated to convergence and the windowed moments there (the driver of
//                              rpsf_core_stars_refine.hpp); it writes its own rows and nothing the other kernels read
//
//   S8  stars_fit_kernel       rpsf_stars_fit, and only then: one wave per position the caller supplies, the least-squares fit of a cell of
//                              a PSF model cube (rpsf_stars_model) and its residual (the driver of rpsf_core_stars_fit.hpp); it writes
//                              its own rows and nothing the other kernels read
//
//   S9  stars_fitpos_kernel    rpsf_stars_fit_positions, and only then: one wave per position the caller supplies, (y, x) iterated with
//                              the star's cell of the model until the Gauss-Newton step is below eps (the driver of
//                              rpsf_core_stars_fitpos.hpp), then stars_fit_kernel at the positions it ends at; both write rows of
//                              their own and nothing the other kernels read
//
//   S10 stars_render_kernel    rpsf_stars_render, and only then: one workgroup per tile of output pixels, the fitted stars on the tile's
//                              list drawn with their cells of the model in ascending star index, a gather (the driver of
//                              rpsf_core_stars_render.hpp); it writes the output frame and nothing the other kernels read
//   S11 stars_fit_group_kernel rpsf_stars_fit_groups, and only then: the host links the stars whose fit discs overlap into groups
//                              (rpsf_core_stars_group.hpp), one wave per group fits its members together (the driver of
//                              rpsf_core_stars_fit_group.hpp), and stars_fit_kernel fits every star that is alone; both write rows of
//                              their own and nothing the other kernels read
//   S12 stars_fit_weighted_kernel  rpsf_stars_fit_weighted, and only then: S8 with one weight per pixel, 1 / v with v from the finder's
//                              variance frame (rpsf_stars_variance_host / _view) or from sky_variance + max(pixel, 0) / gain, and the
//                              formal variances of flux and background (the driver of rpsf_core_stars_fit_weighted.hpp); it writes rows
//                              of its own and nothing the other kernels read
//
// The phases are the drivers of rpsf_core_stars.hpp.  Launches follow one another on the null stream; no workgroup ever waits for
// another one, and the only atomics are integer min / max / add - labels and moments are the same on every run.
#include <hip/hip_runtime.h>

#include <climits>
#include <string>
#include <vector>

#include "rpsf_convert.hpp"
#include "rpsf_core_convert.hpp"
#include "rpsf_core_stars.hpp"
#include "rpsf_core_stars_deblend.hpp"
#include "rpsf_core_stars_fit.hpp"
#include "rpsf_core_stars_fit_group.hpp"
#include "rpsf_core_stars_fit_weighted.hpp"
#include "rpsf_core_stars_fitpos.hpp"
#include "rpsf_core_stars_group.hpp"
#include "rpsf_core_stars_mesh.hpp"
#include "rpsf_core_stars_photometry.hpp"
#include "rpsf_core_stars_refine.hpp"
#include "rpsf_core_stars_render.hpp"
#include "rpsf_core_stars_shape.hpp"
#include "rpsf_scale.hpp"
#include "rpsf_side_unit.hpp"

using namespace rpsfs;
static_assert(rpsfh::SHAPE_COLUMNS == RPSF_STARS_SHAPE_COLUMNS, "the shape columns of rpsf_core_stars_shape.hpp and include/rpsf.h");
static_assert(rpsfp::photometry_columns(3) == RPSF_STARS_PHOTOMETRY_COLUMNS(3), "the photometry columns of rpsf_core_stars_photometry.hpp and include/rpsf.h");
static_assert(rpsfp::s6_lds_bytes(rpsfp::MAX_RADII) <= 64 * 1024, "S6's records fit the LDS a launch gets without asking");
static_assert(rpsfr::REFINE_COLUMNS == RPSF_STARS_REFINE_COLUMNS, "the refine columns of rpsf_core_stars_refine.hpp and include/rpsf.h");
static_assert(rpsfr::s7_lds_bytes() <= 64 * 1024 && rpsfr::s7_lds_bytes() % 16 == 0, "S7's records fit the LDS a launch gets without asking");
static_assert(rpsff::FIT_COLUMNS == RPSF_STARS_FIT_COLUMNS, "the fit columns of rpsf_core_stars_fit.hpp and include/rpsf.h");
static_assert(rpsff::FLAG_NO_MESH == RPSF_STARS_FIT_NO_MESH && rpsff::FLAG_TOO_FEW == RPSF_STARS_FIT_TOO_FEW &&
                  rpsff::FLAG_DEGENERATE == RPSF_STARS_FIT_DEGENERATE && rpsff::FLAG_BAD_CELL == RPSF_STARS_FIT_BAD_CELL,
              "the fit flags of rpsf_core_stars_fit.hpp and include/rpsf.h");
static_assert(rpsff::s8_lds_bytes() <= 64 * 1024 && rpsff::s8_lds_bytes() % 16 == 0, "S8's records fit the LDS a launch gets without asking");

static_assert(rpsfg::FITPOS_COLUMNS == RPSF_STARS_FITPOS_COLUMNS, "the iteration columns of rpsf_core_stars_fitpos.hpp and include/rpsf.h");
static_assert(rpsfg::POS_RAN_AWAY == RPSF_STARS_FITPOS_RAN_AWAY && rpsfg::POS_NOT_CONVERGED == RPSF_STARS_FITPOS_NOT_CONVERGED &&
                  rpsfg::POS_SINGULAR == RPSF_STARS_FITPOS_SINGULAR && rpsfg::POS_SKIPPED == RPSF_STARS_FITPOS_SKIPPED,
              "the iteration flags of rpsf_core_stars_fitpos.hpp and include/rpsf.h");
static_assert(rpsfg::s9_lds_bytes() <= 64 * 1024 && rpsfg::s9_lds_bytes() % 16 == 0, "S9's records fit the LDS a launch gets without asking");

static_assert(rpsfj::GROUP_COLUMNS == RPSF_STARS_FIT_GROUPS_COLUMNS && rpsfq::MAX_GROUP == RPSF_STARS_MAX_GROUP &&
                  rpsfq::FLAG_CROWDED == RPSF_STARS_FIT_CROWDED,
              "the group columns, the largest group and the crowded flag of rpsf_core_stars_fit_group.hpp and include/rpsf.h");
static_assert(rpsfj::s11_lds_bytes() <= 64 * 1024 && rpsfj::s11_lds_bytes() % 16 == 0, "S11's records fit the LDS a launch gets without asking");
static_assert(rpsfw::FITW_COLUMNS == RPSF_STARS_FIT_WEIGHTED_COLUMNS && rpsfw::VARIANCE_MAP == RPSF_STARS_VARIANCE_MAP &&
                  rpsfw::VARIANCE_MODEL == RPSF_STARS_VARIANCE_MODEL,
              "the weighted fit's columns and variance modes of rpsf_core_stars_fit_weighted.hpp and include/rpsf.h");
static_assert(rpsfw::s12_lds_bytes() <= 64 * 1024 && rpsfw::s12_lds_bytes() % 16 == 0, "S12's records fit the LDS a launch gets without asking");

static_assert(rpsfn::MODE_MODEL == RPSF_STARS_RENDER_MODEL && rpsfn::MODE_RESIDUAL == RPSF_STARS_RENDER_RESIDUAL &&
                  rpsfn::MODE_RESIDUAL_MESH == RPSF_STARS_RENDER_RESIDUAL_MESH,
              "the render modes of rpsf_core_stars_render.hpp and include/rpsf.h");

extern __shared__ __attribute__((aligned(16))) char stars_lds[];

__global__ __launch_bounds__(S1_THREADS) void stars_mesh_kernel(Frame fr, double* level, double* rms) {
  GpuCtx ctx;
  s1_box(ctx, fr, (int)blockIdx.y, (int)blockIdx.x, stars_lds, level, rms);
}
__global__ __launch_bounds__(TILE_THREADS) void stars_detect_kernel(Frame fr, const double* L, double T, uint8_t* det) {
  GpuCtx ctx;
  s2_tile(ctx, fr, L, T, (int)blockIdx.y, (int)blockIdx.x, stars_lds, det);
}
// S2 with T read from device memory, where S1b left it
__global__ __launch_bounds__(TILE_THREADS) void stars_detect_device_kernel(Frame fr, const double* L, const double* T, uint8_t* det) {
  GpuCtx ctx;
  s2_tile(ctx, fr, L, T[0], (int)blockIdx.y, (int)blockIdx.x, stars_lds, det);
}
__global__ __launch_bounds__(rpsfm::S1B_THREADS) void stars_mesh_filter_kernel(int nby, int nbx, double* level, double* rms, double* level_f,
                                                                               double* rms_f, double* out, int* none) {
  GpuCtx ctx;
  rpsfm::s1b_mesh(ctx, nby, nbx, level, rms, level_f, rms_f, out, none, stars_lds);
}
__global__ __launch_bounds__(rpsfm::S1B_THREADS) void stars_mesh_many_count_kernel(rpsfm::Source src, const rpsfm::Sel* state, int step,
                                                                                   rpsfm::Total* acc) {
  GpuCtx ctx;
  rpsfm::many_count(ctx, (int)blockIdx.x, (int)gridDim.x, src, state, step, acc, stars_lds);
}
__global__ __launch_bounds__(64) void stars_mesh_many_step_kernel(rpsfm::Sel* state, rpsfm::Total* acc, int step) {
  if (global_id() == 0) rpsfm::many_step(state, acc, step);
}
__global__ __launch_bounds__(256) void stars_mesh_many_fill_kernel(long n, double* level, double* rms, const rpsfm::Sel* valid) {
  rpsfm::many_fill(global_id(), n, level, rms, valid);
}
__global__ __launch_bounds__(256) void stars_mesh_many_filter_kernel(int nby, int nbx, const double* level, const double* rms, double* level_f,
                                                                     double* rms_f) {
  rpsfm::many_filter(global_id(), nby, nbx, level, rms, level_f, rms_f);
}
__global__ __launch_bounds__(64) void stars_mesh_many_finish_kernel(const rpsfm::Sel* valid, const rpsfm::Sel* all, double* out, int* none) {
  if (global_id() == 0) rpsfm::many_finish(valid, all, out, none);
}
// T = threshold * global_rms: one float64 multiply, one plain store
__global__ __launch_bounds__(64) void stars_threshold_kernel(double threshold, const int* none, double* out) {
  if (global_id() == 0) out[rpsfm::OUT_T] = rpsfm::threshold_of(threshold, out[rpsfm::OUT_GLOBAL_RMS], none[0]);
}

__global__ __launch_bounds__(TILE_THREADS) void stars_label_tile_kernel(const uint8_t* det, int H, int W, int32_t* labels) {
  GpuCtx ctx;
  s3_tile(ctx, det, H, W, (int)blockIdx.y, (int)blockIdx.x, reinterpret_cast<int*>(stars_lds), labels);
}
__global__ __launch_bounds__(256) void stars_label_seam_kernel(int H, int W, int32_t* labels) { s3_seam(global_id(), H, W, labels); }
__global__ __launch_bounds__(256) void stars_label_flatten_kernel(long npix, int32_t* labels) { s3_flatten(global_id(), npix, labels); }
__global__ __launch_bounds__(256) void stars_count_kernel(int H, int W, const int32_t* labels, int* segcnt) {
  s4_count(global_id(), H, W, labels, segcnt);
}
__global__ __launch_bounds__(SCAN_THREADS) void stars_scan_kernel(long nseg, const int* segcnt, int* segoff, int* total) {
  GpuCtx ctx;
  s4_scan(ctx, nseg, segcnt, segoff, total, reinterpret_cast<int*>(stars_lds));
}
__global__ __launch_bounds__(256) void stars_roots_kernel(int H, int W, const int32_t* labels, const int* segoff, int* roots) {
  s4_roots(global_id(), H, W, labels, segoff, roots);
}
__global__ __launch_bounds__(256) void stars_init_kernel(long count, int W, const int* roots, int* stats) {
  s4_init(global_id(), count, W, roots, stats);
}
__global__ __launch_bounds__(256) void stars_accumulate_kernel(long npix, int W, const int32_t* labels, const int* roots, long count,
                                                               int* stats) {
  s4_accumulate(global_id(), npix, W, labels, roots, count, stats);
}
__global__ __launch_bounds__(WALK_THREADS) void stars_walk_kernel(Frame fr, const double* L, const int32_t* labels, const int* roots,
                                                                  const int* stats, long count, long min_area, long max_area,
                                                                  double* moments) {
  GpuCtx ctx;
  s4_walk(ctx, fr, L, labels, roots, stats, count, min_area, max_area, (long)blockIdx.x * WALK_WAVES, reinterpret_cast<double*>(stars_lds),
          moments);
}

__global__ __launch_bounds__(WALK_THREADS) void stars_shape_kernel(Frame fr, const double* L, const int32_t* labels, const int32_t* owner,
                                                                   const rpsfh::ShapeRow* rows, long count, double* out) {
  GpuCtx ctx;
  rpsfh::s5_walk(ctx, fr, L, labels, owner, rows, count, (long)blockIdx.x * WALK_WAVES, reinterpret_cast<rpsfh::Seen*>(stars_lds), out);
}

__global__ __launch_bounds__(WALK_THREADS) void stars_photometry_kernel(Frame fr, const double* L, const int* none, int use_mesh,
                                                                        rpsfp::Apertures ap, const double* pos, long count, double* out) {
  GpuCtx ctx;
  rpsfp::s6_apertures(ctx, fr, L, none, use_mesh, ap, pos, count, (long)blockIdx.x * WALK_WAVES, stars_lds, out);
}

__global__ __launch_bounds__(WALK_THREADS) void stars_refine_kernel(Frame fr, const double* L, const int* none, int use_mesh, rpsfr::Refine rf,
                                                                    const double* pos, const double* sigma, long count, double* out) {
  GpuCtx ctx;
  rpsfr::s7_refine(ctx, fr, L, none, use_mesh, rf, pos, sigma, count, (long)blockIdx.x * WALK_WAVES, stars_lds, out);
}

__global__ __launch_bounds__(WALK_THREADS) void stars_fit_kernel(Frame fr, const double* L, const int* none, int use_mesh, rpsff::Model model,
                                                                 rpsff::Fit fit, const double* pos, const int* cell, long count, double* out) {
  GpuCtx ctx;
  rpsff::s8_fit(ctx, fr, L, none, use_mesh, model, fit, pos, cell, count, (long)blockIdx.x * WALK_WAVES, stars_lds, out);
}

__global__ __launch_bounds__(WALK_THREADS) void stars_fitpos_kernel(Frame fr, const double* L, const int* none, int use_mesh, rpsff::Model model,
                                                                    rpsff::Fit fit, rpsfg::FitPos fp, const double* pos, const int* cell,
                                                                    long count, double* out, double* final_pos) {
  GpuCtx ctx;
  rpsfg::s9_fit_positions(ctx, fr, L, none, use_mesh, model, fit, fp, pos, cell, count, (long)blockIdx.x * WALK_WAVES, stars_lds, out, final_pos);
}

// S11's context: the sums a lane carries from one each() to the next are registers of that thread
struct GroupCtx : GpuCtx {
  rpsfj::Lane lane;
  __device__ __forceinline__ rpsfj::Lane& regs(int) { return lane; }
};
__global__ __launch_bounds__(WALK_THREADS) void stars_fit_group_kernel(Frame fr, const double* L, int use_mesh, rpsff::Model model, rpsff::Fit fit,
                                                                       const double* pos, const int* cell, rpsfj::GroupList groups,
                                                                       double* out) {
  GroupCtx ctx;
  rpsfj::s11_fit_group(ctx, fr, L, use_mesh, model, fit, pos, cell, groups, (long)blockIdx.x * WALK_WAVES, stars_lds, out);
}

__global__ __launch_bounds__(WALK_THREADS) void stars_fit_weighted_kernel(Frame fr, const double* L, const int* none, int use_mesh,
                                                                          rpsff::Model model, rpsff::Fit fit, rpsfw::Variance var,
                                                                          const double* pos, const int* cell, long count, double* out) {
  GpuCtx ctx;
  rpsfw::s12_fit_weighted(ctx, fr, L, none, use_mesh, model, fit, var, pos, cell, count, (long)blockIdx.x * WALK_WAVES, stars_lds, out);
}

// S10's context: the accumulator of a thread's pixel is a register of that thread
struct RenderCtx : GpuCtx {
  double s;
  __device__ __forceinline__ double& reg(int) { return s; }
};
__global__ __launch_bounds__(WALK_THREADS) void stars_render_kernel(Frame fr, const double* L, rpsff::Model model, rpsfn::Render rd,
                                                                    rpsfn::Stars st, void* out) {
  RenderCtx ctx;
  rpsfn::s10_render(ctx, fr, L, model, rd, st, (int)blockIdx.y, (int)blockIdx.x, stars_lds, out);
}

// ------------------------------------------------------------------------------------------------ the deblend option
// S2 that also stores the filtered residual; T from device memory when T_dev is given
__global__ __launch_bounds__(TILE_THREADS) void stars_detect_f_kernel(Frame fr, const double* L, const double* T_dev, double T, uint8_t* det,
                                                                      double* f) {
  GpuCtx ctx;
  s2_tile(ctx, fr, L, T_dev ? T_dev[0] : T, (int)blockIdx.y, (int)blockIdx.x, stars_lds, det, f);
}
__global__ __launch_bounds__(256) void deblend_up_kernel(int H, int W, const double* f, const uint8_t* det, int32_t* up) {
  rpsfd::d1_up(global_id(), H, W, f, det, up);
}
__global__ __launch_bounds__(256) void deblend_peak_kernel(long npix, const int32_t* up, int32_t* peak) {
  rpsfd::d1_peak(global_id(), npix, up, peak);
}
__global__ __launch_bounds__(256) void deblend_init_kernel(long nb, int W, const int* peaks, int* bstats, uint64_t* saddle) {
  rpsfd::d2_init(global_id(), nb, W, peaks, bstats, saddle);
}
__global__ __launch_bounds__(256) void deblend_accumulate_kernel(int H, int W, const double* f, const int32_t* peak, const int* peaks, long nb,
                                                                 int* bstats, uint64_t* saddle) {
  rpsfd::d2_accumulate(global_id(), H, W, f, peak, peaks, nb, bstats, saddle);
}
__global__ __launch_bounds__(256) void deblend_want_kernel(long nb, const uint64_t* saddle, uint8_t* want) {
  rpsfd::d2_want(global_id(), nb, saddle, want);
}
__global__ __launch_bounds__(WALK_THREADS) void deblend_walk_kernel(Frame fr, const double* L, const int32_t* labels, rpsfd::Objects o,
                                                                    double* out) {
  GpuCtx ctx;
  rpsfd::d_walk(ctx, fr, L, labels, o, (long)blockIdx.x * WALK_WAVES, reinterpret_cast<double*>(stars_lds), out);
}
__global__ __launch_bounds__(256) void deblend_significant_kernel(long nb, int W, const double* f, const int32_t* labels, const int* roots,
                                                                  long count, const double* moments, const int* peaks, const int* bstats,
                                                                  const uint64_t* saddle, const double* bflux, rpsfd::Significance s,
                                                                  const double* T_dev, int* bcomp, uint8_t* sig, int* nsig, int* ostats) {
  if (T_dev) s.T = T_dev[0];
  rpsfd::d3_significant(global_id(), nb, W, f, labels, roots, count, moments, peaks, bstats, saddle, bflux, s, bcomp, sig, nsig, ostats);
}
__global__ __launch_bounds__(rpsfd::OWN_THREADS) void deblend_own_kernel(int W, const int32_t* labels, const int* roots, const int* stats,
                                                                         const int32_t* peak, const int* peaks, long nb, const int* bcomp,
                                                                         const uint8_t* sig, const int* nsig, int32_t* owner, int* ostats) {
  GpuCtx ctx;
  rpsfd::d4_own(ctx, W, labels, roots, stats, (long)blockIdx.x, peak, peaks, nb, bcomp, sig, nsig, stars_lds, owner, ostats);
}
__global__ __launch_bounds__(256) void deblend_objects_kernel(long nb, const int* bcomp, const uint8_t* sig, const int* nsig, const int* ostats,
                                                              long min_area, long max_area, uint8_t* want) {
  rpsfd::d4_want(global_id(), nb, bcomp, sig, nsig, ostats, min_area, max_area, want);
}

struct rpsf_stars {
  int device = 0, H = 0, W = 0, box = 0, nby = 0, nbx = 0;
  bool have_frame = false;
  bool have_mesh = false;  // S1b ran on the frame: level_f, mesh_out and none hold its results
  Buf<float> frame;
  Buf<double> level_f, rms_f, mesh_out;  // S1b: the filtered meshes; mesh_out[0] = global rms, [1] = T
  Buf<int> none;                         // S1b: 1 when no box of the frame has a usable pixel
  Buf<rpsfm::Sel> mesh_state;            // S1b on many workgroups: the two selections
  Buf<rpsfm::Total> mesh_acc;
  rpsf_scale_scratch* upscale = nullptr;  // rpsf_stars_background_scaled
  double mesh_ms = 0;
  Buf<uint8_t> mask, det;
  Buf<int32_t> labels;
  Buf<double> level, rms, moments;
  Buf<int> segcnt, segoff, total, roots, stats;
  std::vector<double> found;  // rows (row, col, flux, area) of the last detect
  // S5 (rpsf_stars_measure): where each row of `found` came from, and whether what the detect left on the device is still there
  std::vector<rpsfh::Source> sources;
  unsigned long generation = 0, detected_at = 0;  // every call that replaces the frame, a mesh or the labels moves `generation` on
  const double* detected_mesh = nullptr;          // the filtered mesh of the last detect, on the device
  Buf<rpsfh::ShapeRow> shape_rows;
  Buf<double> shapes_dev;
  std::vector<double> shapes;  // rows of RPSF_STARS_SHAPE_COLUMNS of the last measure
  double shape_ms = 0;
  // S6 (rpsf_stars_photometry): its own positions and rows, nothing of the above
  Buf<double> phot_pos, phot_out;
  double photometry_ms = 0;
  // S7 (rpsf_stars_refine): likewise its own
  Buf<double> refine_pos, refine_sigma, refine_out;
  double refine_ms = 0;
  // S8 (rpsf_stars_fit): likewise its own
  Buf<double> fit_pos, fit_out;
  Buf<int> fit_cell;
  double fit_ms = 0;
  // S9 (rpsf_stars_fit_positions): likewise its own, S8's rows at the fitted positions among them
  Buf<double> fitpos_pos, fitpos_final, fitpos_iter, fitpos_fit;
  Buf<int> fitpos_cell;
  double fitpos_ms = 0;
  // S10 (rpsf_stars_render): likewise its own - the star records, the tile lists and the frame a host caller gets
  Buf<double> render_pos, render_flux, render_out;
  Buf<int> render_cell, render_index;
  Buf<long long> render_offsets;
  double render_ms = 0;
  // S11 (rpsf_stars_fit_groups): likewise its own - every star's position and cell, the groups, S11's rows by member and S8's by lone star
  Buf<double> group_pos, group_out, group_lone_pos, group_lone_out;
  Buf<int> group_cell, group_members, group_lone_cell;
  Buf<long long> group_starts;
  double group_ms = 0;
  // S12 (rpsf_stars_fit_weighted): likewise its own, and the variance frame of rpsf_stars_variance_host / _view (allocated by the first)
  Buf<float> variance;
  bool have_variance = false;
  Buf<double> fitw_pos, fitw_out;
  Buf<int> fitw_cell;
  double fitw_ms = 0;
  // the deblend option: everything below is allocated by the first call that needs it
  bool deblend = false;
  double contrast = 0.005, prominence = 1.0;
  Buf<double> f, bflux, omoments;  // the filtered residual per pixel; (sum d, .., .., area) per basin and per object
  Buf<int32_t> up, peak, owner;
  Buf<int> peaks, bstats, ostats, bcomp, nsig;
  Buf<uint64_t> saddle;
  Buf<uint8_t> sig, want;
  size_t n_components = 0, n_basins = 0, n_split = 0;  // of the last detect
  double deblend_ms = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
  double ms[4] = {0, 0, 0, 0};
  long npix() const { return (long)H * W; }
  long nseg() const { return (long)H * segs_per_row(W); }
  Frame view() const { return Frame{frame.p, mask.p, H, W, box, nby, nbx}; }
  ~rpsf_stars() {
    rpsf_detail_scale_scratch_free(upscale);
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// device time of what `launches` enqueues, added to *ms
template <class F>
static int timed(rpsf_stars* s, double* ms, F&& launches) {
  HIP_TRY(hipEventRecord(s->ev[0], nullptr));
  launches();
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(s->ev[1], nullptr));
  HIP_TRY(hipEventSynchronize(s->ev[1]));
  float t = 0;
  HIP_TRY(hipEventElapsedTime(&t, s->ev[0], s->ev[1]));
  *ms += t;
  return RPSF_OK;
}

// a PSF model on the device (rpsf_stars_model_create, S8)
struct rpsf_stars_model {
  int device = 0, n_cells = 0, N = 0;
  Buf<double> values;
  std::vector<uint8_t> finite;  // per cell: every value is finite (rpsf_stars_fit_groups fits only stars of such cells together)
};

// ------------------------------------------------------------------------------------------------ a call over n positions
// What rpsf_stars_fit, _fit_positions, _fit_weighted and _fit_groups check of their model, with the function's `name` in every message.
static int check_model(const std::string& name, const rpsf_stars* s, const rpsf_stars_model* model, double radius) {
  if (!(radius <= rpsff::max_fit_radius(model->N)))
    return fail(RPSF_E_BADARG,
                name + ": radius " + std::to_string(radius) + " is above min(64, N / 2 - 1) of the model's N = " + std::to_string(model->N));
  if (model->device != s->device) return fail(RPSF_E_BADARG, name + ": the model is on another device than the finder");
  return RPSF_OK;
}

// What S6 - S9, S11 and S12 check alike before they launch, in this order and with the function's `name` in every message: the pointers
// (`pointers`: none that the call needs is null), the call's own arguments (`why`: what is wrong with them, or null), the 2^30 limit,
// every position - and after position i what `item(i)` says of the call's other array (RPSF_OK, or it has failed) -, the model (null: the
// call takes none) and that the frame has its mesh.
template <class Item>
static int check_positions_call(const std::string& name, const rpsf_stars* s, bool pointers, const char* why, size_t n, const double* positions_host,
                                const rpsf_stars_model* model, double radius, Item&& item) {
  if (!pointers) return fail(RPSF_E_BADARG, "null argument");
  if (why) return fail(RPSF_E_BADARG, name + ": " + why);
  if (n > ((size_t)1 << 30)) return fail(RPSF_E_UNSUPPORTED, name + ": more than 2^30 positions in one call");
  for (size_t i = 0; i < n; ++i) {
    if (!rpsfp::position_ok(positions_host[2 * i], positions_host[2 * i + 1]))
      return fail(RPSF_E_BADARG, name + ": position " + std::to_string(i) + " is not finite or not inside |y|, |x| < 2^20");
    if (const int rc = item(i)) return rc;
  }
  if (model)
    if (const int rc = check_model(name, s, model, radius)) return rc;
  if (!s->have_mesh) return fail(RPSF_E_STATE, name + " before a rpsf_stars_background_view / _host / _scaled of the frame");
  return RPSF_OK;
}
static int check_positions_call(const std::string& name, const rpsf_stars* s, bool pointers, const char* why, size_t n, const double* positions_host,
                                const rpsf_stars_model* model = nullptr, double radius = 0.0) {
  return check_positions_call(name, s, pointers, why, n, positions_host, model, radius, [](size_t) { return RPSF_OK; });
}
// one wave per position (or group): the grid of S6 - S9, S11 and S12
static dim3 walk_grid(size_t n) { return dim3((unsigned)((n + WALK_WAVES - 1) / WALK_WAVES)); }

static void launch_label(rpsf_stars* s) {
  const dim3 tiles((s->W + TILE_C - 1) / TILE_C, (s->H + TILE_R - 1) / TILE_R);
  hipLaunchKernelGGL(stars_label_tile_kernel, tiles, dim3(TILE_THREADS), TILE_R * TILE_C * sizeof(int), nullptr, s->det.p, s->H, s->W,
                     s->labels.p);
  hipLaunchKernelGGL(stars_label_seam_kernel, dim3(blocks_for((long)tiles.x * tiles.y * SEAM_SLOTS)), dim3(256), 0, nullptr, s->H, s->W,
                     s->labels.p);
  hipLaunchKernelGGL(stars_label_flatten_kernel, dim3(blocks_for(s->npix())), dim3(256), 0, nullptr, s->npix(), s->labels.p);
}

extern "C" int rpsf_stars_create(rpsf_stars** out, int device, int height, int width, int box) {
  if (!out) return fail(RPSF_E_BADARG, "null argument");
  if (height <= 0 || width <= 0) return fail(RPSF_E_BADARG, "a frame needs positive height and width");
  if (box < MIN_BOX || box > MAX_BOX)
    return fail(RPSF_E_UNSUPPORTED, "background box " + std::to_string(box) + " is outside 8..128");
  if ((long)height * width > INT_MAX) return fail(RPSF_E_UNSUPPORTED, "frames of more than 2^31 - 1 pixels are not supported");
  HIP_TRY(hipSetDevice(device));
  rpsf_stars* s = new rpsf_stars;
  s->device = device, s->H = height, s->W = width, s->box = box;
  s->nby = (height + box - 1) / box, s->nbx = (width + box - 1) / box;
  auto made = [&]() -> int {
    for (auto& e : s->ev) HIP_TRY(hipEventCreate(&e));
    const size_t npix = (size_t)s->npix(), nmesh = (size_t)s->nby * s->nbx;
    HIP_TRY(s->frame.reserve(npix));
    HIP_TRY(s->mask.reserve(npix));
    HIP_TRY(s->det.reserve(npix));
    HIP_TRY(s->labels.reserve(npix));
    HIP_TRY(s->level.reserve(nmesh));
    HIP_TRY(s->rms.reserve(nmesh));
    HIP_TRY(s->segcnt.reserve((size_t)s->nseg()));
    HIP_TRY(s->segoff.reserve((size_t)s->nseg()));
    HIP_TRY(s->total.reserve(1));
    HIP_TRY(s->level_f.reserve(nmesh));
    HIP_TRY(s->rms_f.reserve(nmesh));
    HIP_TRY(s->mesh_out.reserve(2));
    HIP_TRY(s->none.reserve(1));
    if ((long)nmesh > rpsfm::MANY_NODES) {
      HIP_TRY(s->mesh_state.reserve(2));
      HIP_TRY(s->mesh_acc.reserve(1));
    }
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&stars_mesh_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)s1_lds_bytes(MAX_BOX)));  // 70 KiB at box = 128
    return RPSF_OK;
  }();
  if (made != RPSF_OK) {
    delete s;
    return made;
  }
  *out = s;
  return RPSF_OK;
}

extern "C" void rpsf_stars_destroy(rpsf_stars* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  delete s;
}

static int upload_mask(rpsf_stars* s, const uint8_t* mask_host_or_null) {
  const size_t npix = (size_t)s->npix();
  if (mask_host_or_null) {
    std::vector<uint8_t> flags(npix);
    for (size_t i = 0; i < npix; ++i) flags[i] = mask_host_or_null[i] != 0;
    HIP_TRY(hipMemcpy(s->mask.p, flags.data(), npix, hipMemcpyHostToDevice));
  } else {
    HIP_TRY(hipMemset(s->mask.p, 0, npix));
  }
  return RPSF_OK;
}

// S1 on the finder's frame and mask into s->level / s->rms
static int mesh_on_device(rpsf_stars* s) {
  s->ms[0] = 0;
  return timed(s, &s->ms[0], [&] {
    hipLaunchKernelGGL(stars_mesh_kernel, dim3(s->nbx, s->nby), dim3(S1_THREADS), s1_lds_bytes(s->box), nullptr, s->view(), s->level.p,
                       s->rms.p);
  });
}

extern "C" int rpsf_stars_background(rpsf_stars* s, const void* image_host, int image_is_f64, const uint8_t* mask_host_or_null,
                                     double* level_host, double* rms_host) {
  if (!s || !image_host || !level_host || !rms_host) return fail(RPSF_E_BADARG, "null argument");
  const size_t nmesh = (size_t)s->nby * s->nbx;
  HIP_TRY(hipSetDevice(s->device));
  s->have_frame = s->have_mesh = false;
  ++s->generation;
  if (const int rc = upload_frame_f32(s->frame.p, image_host, image_is_f64, (size_t)s->npix())) return rc;
  if (const int rc = upload_mask(s, mask_host_or_null)) return rc;
  if (const int rc = mesh_on_device(s)) return rc;
  HIP_TRY(hipMemcpy(level_host, s->level.p, nmesh * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rms_host, s->rms.p, nmesh * sizeof(double), hipMemcpyDeviceToHost));
  s->have_frame = true;
  return RPSF_OK;
}

static int detect_on_device(rpsf_stars* s, const double* L, const double* T_dev, double T, long min_area, long max_area, size_t* count);
static int deblend_on_device(rpsf_stars* s, const double* L, const double* T_dev, double T, long min_area, long max_area, long n);

extern "C" int rpsf_stars_detect(rpsf_stars* s, const double* level_host, double threshold_abs, long min_area, long max_area,
                                 size_t* count) {
  if (!s || !level_host || !count) return fail(RPSF_E_BADARG, "null argument");
  if (!s->have_frame) return fail(RPSF_E_STATE, "rpsf_stars_detect before rpsf_stars_background uploaded a frame");
  const size_t nmesh = (size_t)s->nby * s->nbx;
  for (size_t i = 0; i < nmesh; ++i)
    if (!std::isfinite(level_host[i])) return fail(RPSF_E_BADARG, "the background mesh has a non-finite node");
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipMemcpy(s->level.p, level_host, nmesh * sizeof(double), hipMemcpyHostToDevice));
  s->have_mesh = false;  // S1b's filled mesh is gone
  ++s->generation;
  return detect_on_device(s, s->level.p, nullptr, threshold_abs, min_area, max_area, count);
}

// S2 - S4 on the finder's frame with the filtered mesh L (on the device) and the threshold T_dev[0] (on the device) or, T_dev null, T
static int detect_on_device(rpsf_stars* s, const double* L, const double* T_dev, double T, long min_area, long max_area, size_t* count) {
  s->found.clear();
  s->sources.clear();
  s->shapes.clear();
  s->detected_at = 0, s->detected_mesh = L;
  *count = 0;
  s->ms[1] = s->ms[2] = s->ms[3] = s->deblend_ms = 0;
  s->n_components = s->n_basins = s->n_split = 0;
  const dim3 tiles((s->W + TILE_C - 1) / TILE_C, (s->H + TILE_R - 1) / TILE_R);
  if (s->deblend) HIP_TRY(s->f.reserve((size_t)s->npix()));
  if (const int rc = timed(s, &s->ms[1], [&] {
        if (s->deblend) {
          hipLaunchKernelGGL(stars_detect_f_kernel, tiles, dim3(TILE_THREADS), s2_lds_bytes(), nullptr, s->view(), L, T_dev, T, s->det.p,
                             s->f.p);
        } else if (T_dev) {
          hipLaunchKernelGGL(stars_detect_device_kernel, tiles, dim3(TILE_THREADS), s2_lds_bytes(), nullptr, s->view(), L, T_dev, s->det.p);
        } else {
          hipLaunchKernelGGL(stars_detect_kernel, tiles, dim3(TILE_THREADS), s2_lds_bytes(), nullptr, s->view(), L, T, s->det.p);
        }
      }))
    return rc;
  if (const int rc = timed(s, &s->ms[2], [&] { launch_label(s); })) return rc;
  if (const int rc = timed(s, &s->ms[3], [&] {
        hipLaunchKernelGGL(stars_count_kernel, dim3(blocks_for(s->nseg())), dim3(256), 0, nullptr, s->H, s->W, s->labels.p, s->segcnt.p);
        hipLaunchKernelGGL(stars_scan_kernel, dim3(1), dim3(SCAN_THREADS), (SCAN_THREADS + 32) * sizeof(int), nullptr, s->nseg(),
                           s->segcnt.p, s->segoff.p, s->total.p);
      }))
    return rc;
  int total = 0;
  HIP_TRY(hipMemcpy(&total, s->total.p, sizeof(int), hipMemcpyDeviceToHost));
  if (total <= 0) {
    s->detected_at = ++s->generation;
    return RPSF_OK;
  }
  const long n = total;
  s->n_components = (size_t)n;
  const long walk_max = s->deblend ? -1 : max_area;  // D3 needs every component's sum; the area limits are applied to the rows below
  HIP_TRY(s->roots.reserve((size_t)n));
  HIP_TRY(s->stats.reserve(4 * (size_t)n));
  HIP_TRY(s->moments.reserve(4 * (size_t)n));
  if (const int rc = timed(s, &s->ms[3], [&] {
        hipLaunchKernelGGL(stars_roots_kernel, dim3(blocks_for(s->nseg())), dim3(256), 0, nullptr, s->H, s->W, s->labels.p, s->segoff.p,
                           s->roots.p);
        hipLaunchKernelGGL(stars_init_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, n, s->W, s->roots.p, s->stats.p);
        hipLaunchKernelGGL(stars_accumulate_kernel, dim3(blocks_for(s->npix())), dim3(256), 0, nullptr, s->npix(), s->W, s->labels.p,
                           s->roots.p, n, s->stats.p);
        hipLaunchKernelGGL(stars_walk_kernel, dim3((unsigned)((n + WALK_WAVES - 1) / WALK_WAVES)), dim3(WALK_THREADS), s4_walk_lds_bytes(),
                           nullptr, s->view(), L, s->labels.p, s->roots.p, s->stats.p, n, min_area, walk_max, s->moments.p);
      }))
    return rc;
  if (s->deblend) {
    if (const int rc = deblend_on_device(s, L, T_dev, T, min_area, max_area, n)) return rc;
    *count = s->found.size() / 4;
    s->detected_at = ++s->generation;
    return RPSF_OK;
  }
  std::vector<double> m(4 * (size_t)n);
  HIP_TRY(hipMemcpy(m.data(), s->moments.p, m.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (long k = 0; k < n; ++k) {  // roots ascend: this is the raster order of each component's first pixel
    const double flux = m[4 * k], area = m[4 * k + 3];
    if (area < (double)min_area || (max_area >= 0 && area > (double)max_area) || !(flux > 0.0)) continue;
    s->found.insert(s->found.end(), {m[4 * k + 1] / flux, m[4 * k + 2] / flux, flux, area});
    s->sources.emplace_back(k, -1);
  }
  *count = s->found.size() / 4;
  s->detected_at = ++s->generation;
  return RPSF_OK;
}

static void launch_ascent(rpsf_stars* s) {
  hipLaunchKernelGGL(deblend_up_kernel, dim3(blocks_for(s->npix())), dim3(256), 0, nullptr, s->H, s->W, s->f.p, s->det.p, s->up.p);
  hipLaunchKernelGGL(deblend_peak_kernel, dim3(blocks_for(s->npix())), dim3(256), 0, nullptr, s->npix(), s->up.p, s->peak.p);
}

// D1 - D4 after S2 (with f) - S4 (every component of at least min_area walked) of the same frame: the rows into s->found
static int deblend_on_device(rpsf_stars* s, const double* L, const double* T_dev, double T, long min_area, long max_area, long n) {
  const size_t npix = (size_t)s->npix();
  HIP_TRY(s->up.reserve(npix));
  HIP_TRY(s->peak.reserve(npix));
  HIP_TRY(s->owner.reserve(npix));
  if (const int rc = timed(s, &s->deblend_ms, [&] {
        launch_ascent(s);
        hipLaunchKernelGGL(stars_count_kernel, dim3(blocks_for(s->nseg())), dim3(256), 0, nullptr, s->H, s->W, s->peak.p, s->segcnt.p);
        hipLaunchKernelGGL(stars_scan_kernel, dim3(1), dim3(SCAN_THREADS), (SCAN_THREADS + 32) * sizeof(int), nullptr, s->nseg(),
                           s->segcnt.p, s->segoff.p, s->total.p);
      }))
    return rc;
  int total = 0;
  HIP_TRY(hipMemcpy(&total, s->total.p, sizeof(int), hipMemcpyDeviceToHost));
  if (total < 1) return fail(RPSF_E_HIP, "deblend: components without a peak");  // every component has its highest pixel
  const long nb = total;
  s->n_basins = (size_t)nb;
  HIP_TRY(s->peaks.reserve((size_t)nb));
  HIP_TRY(s->bstats.reserve(rpsfd::BOX * (size_t)nb));
  HIP_TRY(s->ostats.reserve(rpsfd::BOX * (size_t)nb));
  HIP_TRY(s->bcomp.reserve((size_t)nb));
  HIP_TRY(s->saddle.reserve((size_t)nb));
  HIP_TRY(s->sig.reserve((size_t)nb));
  HIP_TRY(s->want.reserve((size_t)nb));
  HIP_TRY(s->bflux.reserve(4 * (size_t)nb));
  HIP_TRY(s->omoments.reserve(4 * (size_t)nb));
  HIP_TRY(s->nsig.reserve((size_t)n));
  const rpsfd::Significance test{min_area, s->contrast, s->prominence, T};
  const unsigned per_basin = blocks_for(nb), walks = (unsigned)((nb + WALK_WAVES - 1) / WALK_WAVES);
  if (const int rc = timed(s, &s->deblend_ms, [&] {
        hipLaunchKernelGGL(stars_roots_kernel, dim3(blocks_for(s->nseg())), dim3(256), 0, nullptr, s->H, s->W, s->peak.p, s->segoff.p,
                           s->peaks.p);
        hipLaunchKernelGGL(deblend_init_kernel, dim3(per_basin), dim3(256), 0, nullptr, nb, s->W, s->peaks.p, s->bstats.p, s->saddle.p);
        hipLaunchKernelGGL(deblend_accumulate_kernel, dim3(blocks_for(s->npix())), dim3(256), 0, nullptr, s->H, s->W, s->f.p, s->peak.p,
                           s->peaks.p, nb, s->bstats.p, s->saddle.p);
        hipLaunchKernelGGL(deblend_want_kernel, dim3(per_basin), dim3(256), 0, nullptr, nb, s->saddle.p, s->want.p);
        hipLaunchKernelGGL(deblend_walk_kernel, dim3(walks), dim3(WALK_THREADS), s4_walk_lds_bytes(), nullptr, s->view(), L, s->labels.p,
                           rpsfd::Objects{s->peak.p, s->peaks.p, s->bstats.p, s->want.p, nb}, s->bflux.p);
        (void)hipMemsetAsync(s->nsig.p, 0, (size_t)n * sizeof(int), nullptr);
        hipLaunchKernelGGL(deblend_significant_kernel, dim3(per_basin), dim3(256), 0, nullptr, nb, s->W, s->f.p, s->labels.p, s->roots.p, n,
                           s->moments.p, s->peaks.p, s->bstats.p, s->saddle.p, s->bflux.p, test, T_dev, s->bcomp.p, s->sig.p, s->nsig.p,
                           s->ostats.p);
        hipLaunchKernelGGL(deblend_own_kernel, dim3((unsigned)n), dim3(rpsfd::OWN_THREADS), rpsfd::d4_own_lds_bytes(), nullptr, s->W,
                           s->labels.p, s->roots.p, s->stats.p, s->peak.p, s->peaks.p, nb, s->bcomp.p, s->sig.p, s->nsig.p, s->owner.p,
                           s->ostats.p);
        hipLaunchKernelGGL(deblend_objects_kernel, dim3(per_basin), dim3(256), 0, nullptr, nb, s->bcomp.p, s->sig.p, s->nsig.p, s->ostats.p,
                           min_area, max_area, s->want.p);
        hipLaunchKernelGGL(deblend_walk_kernel, dim3(walks), dim3(WALK_THREADS), s4_walk_lds_bytes(), nullptr, s->view(), L, s->labels.p,
                           rpsfd::Objects{s->owner.p, s->peaks.p, s->ostats.p, s->want.p, nb}, s->omoments.p);
      }))
    return rc;
  std::vector<double> moments(4 * (size_t)n), omoments(4 * (size_t)nb);
  std::vector<int> roots((size_t)n), nsig((size_t)n), bcomp((size_t)nb), ostats(rpsfd::BOX * (size_t)nb);
  std::vector<uint8_t> sig((size_t)nb);
  HIP_TRY(hipMemcpy(moments.data(), s->moments.p, moments.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(omoments.data(), s->omoments.p, omoments.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(roots.data(), s->roots.p, roots.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(nsig.data(), s->nsig.p, nsig.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(bcomp.data(), s->bcomp.p, bcomp.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ostats.data(), s->ostats.p, ostats.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(sig.data(), s->sig.p, sig.size(), hipMemcpyDeviceToHost));
  s->found = rpsfd::deblend_rows(n, roots.data(), moments.data(), nsig.data(), nb, bcomp.data(), sig.data(), ostats.data(), omoments.data(),
                                 min_area, max_area, &s->n_split, &s->sources);
  return RPSF_OK;
}

extern "C" int rpsf_stars_set_deblend(rpsf_stars* s, int on, double contrast, double prominence) {
  if (!s) return fail(RPSF_E_BADARG, "null argument");
  if (!(contrast >= 0.0 && contrast <= 1.0)) return fail(RPSF_E_BADARG, "deblend contrast must lie in 0 ... 1");
  if (!(prominence >= 0.0) || !std::isfinite(prominence)) return fail(RPSF_E_BADARG, "deblend prominence must be finite and not negative");
  s->deblend = on != 0, s->contrast = contrast, s->prominence = prominence;
  return RPSF_OK;
}

extern "C" int rpsf_stars_basins(rpsf_stars* s, const double* f_host, const uint8_t* detected_host, int32_t* peak_host) {
  if (!s || !f_host || !detected_host || !peak_host) return fail(RPSF_E_BADARG, "null argument");
  const size_t npix = (size_t)s->npix();
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(s->f.reserve(npix));
  HIP_TRY(s->up.reserve(npix));
  HIP_TRY(s->peak.reserve(npix));
  std::vector<uint8_t> flags(npix);
  for (size_t i = 0; i < npix; ++i) flags[i] = detected_host[i] != 0;
  ++s->generation;
  HIP_TRY(hipMemcpy(s->det.p, flags.data(), npix, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->f.p, f_host, npix * sizeof(double), hipMemcpyHostToDevice));
  s->deblend_ms = 0;
  if (const int rc = timed(s, &s->deblend_ms, [&] { launch_ascent(s); })) return rc;
  HIP_TRY(hipMemcpy(peak_host, s->peak.p, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
  return RPSF_OK;
}

extern "C" int rpsf_stars_deblend_info(const rpsf_stars* s, size_t* components, size_t* basins, size_t* split_components) {
  if (!s) return fail(RPSF_E_BADARG, "null argument");
  if (components) *components = s->n_components;
  if (basins) *basins = s->n_basins;
  if (split_components) *split_components = s->n_split;
  return RPSF_OK;
}

extern "C" int rpsf_stars_deblend_ms(const rpsf_stars* s, double* ms) {
  if (!s || !ms) return fail(RPSF_E_BADARG, "null argument");
  *ms = s->deblend_ms;
  return RPSF_OK;
}

extern "C" int rpsf_stars_positions(rpsf_stars* s, size_t first, size_t count, double* out) {
  if (!s || (!out && count)) return fail(RPSF_E_BADARG, "null argument");
  const size_t have = s->found.size() / 4;
  if (first > have || count > have - first) return fail(RPSF_E_BADARG, "range outside the detections of the last rpsf_stars_detect");
  for (size_t i = 0; i < 4 * count; ++i) out[i] = s->found[4 * first + i];
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------ S5
extern "C" int rpsf_stars_measure(rpsf_stars* s, size_t* count) {
  if (!s || !count) return fail(RPSF_E_BADARG, "null argument");
  if (!s->detected_at)
    return fail(RPSF_E_BADARG, "rpsf_stars_measure before a rpsf_stars_detect / rpsf_stars_detect_device gave the rows to measure");
  if (s->detected_at != s->generation)
    return fail(RPSF_E_BADARG, "rpsf_stars_measure: the frame, the mesh or the labels of the last detect have been replaced since");
  const size_t k = s->found.size() / 4;
  s->shapes.clear();
  s->shape_ms = 0;
  *count = k;
  if (k == 0) return RPSF_OK;  // nothing to launch
  HIP_TRY(hipSetDevice(s->device));
  const size_t n = s->n_components, nb = s->n_basins;
  std::vector<int> roots(n), stats(4 * n), peaks(nb), ostats(rpsfd::BOX * nb);
  HIP_TRY(hipMemcpy(roots.data(), s->roots.p, roots.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(stats.data(), s->stats.p, stats.size() * sizeof(int), hipMemcpyDeviceToHost));
  if (nb) {
    HIP_TRY(hipMemcpy(peaks.data(), s->peaks.p, peaks.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ostats.data(), s->ostats.p, ostats.size() * sizeof(int), hipMemcpyDeviceToHost));
  }
  const std::vector<rpsfh::ShapeRow> rows = rpsfh::describe(s->found, s->sources, s->W, roots.data(), stats.data(), peaks.data(), ostats.data());
  for (const rpsfh::ShapeRow& row : rows)  // the walk reads the whole box: it lies inside the frame, or nothing is launched
    if (row.r0 < 0 || row.r1 < row.r0 || row.r1 >= s->H || row.c0 < 0 || row.c1 < row.c0 || row.c1 >= s->W)
      return fail(RPSF_E_HIP, "rpsf_stars_measure: a bounding box outside the frame");
  HIP_TRY(s->shape_rows.reserve(k));
  HIP_TRY(s->shapes_dev.reserve(RPSF_STARS_SHAPE_COLUMNS * k));
  HIP_TRY(hipMemcpy(s->shape_rows.p, rows.data(), k * sizeof(rpsfh::ShapeRow), hipMemcpyHostToDevice));
  if (const int rc = timed(s, &s->shape_ms, [&] {
        hipLaunchKernelGGL(stars_shape_kernel, dim3((unsigned)((k + WALK_WAVES - 1) / WALK_WAVES)), dim3(WALK_THREADS),
                           rpsfh::s5_walk_lds_bytes(), nullptr, s->view(), s->detected_mesh, s->labels.p, s->owner.p, s->shape_rows.p, (long)k,
                           s->shapes_dev.p);
      }))
    return rc;
  std::vector<double> shapes(RPSF_STARS_SHAPE_COLUMNS * k);
  HIP_TRY(hipMemcpy(shapes.data(), s->shapes_dev.p, shapes.size() * sizeof(double), hipMemcpyDeviceToHost));
  s->shapes = std::move(shapes);
  return RPSF_OK;
}

extern "C" int rpsf_stars_shapes(rpsf_stars* s, size_t first, size_t count, double* out) {
  if (!s || (!out && count)) return fail(RPSF_E_BADARG, "null argument");
  const size_t have = s->shapes.size() / RPSF_STARS_SHAPE_COLUMNS;
  if (first > have || count > have - first) return fail(RPSF_E_BADARG, "range outside the rows of the last rpsf_stars_measure");
  for (size_t i = 0; i < RPSF_STARS_SHAPE_COLUMNS * count; ++i) out[i] = s->shapes[RPSF_STARS_SHAPE_COLUMNS * first + i];
  return RPSF_OK;
}

extern "C" int rpsf_stars_shape_ms(const rpsf_stars* s, double* ms) {
  if (!s || !ms) return fail(RPSF_E_BADARG, "null argument");
  *ms = s->shape_ms;
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------ S6 (Apertures)
extern "C" int rpsf_stars_photometry(rpsf_stars* s, size_t n, const double* positions_host, int m, const double* radii, int subpix,
                                     int use_mesh, double* out_host) {
  if (const int rc = check_positions_call("rpsf_stars_photometry", s, s && (!n || (positions_host && out_host)),
                                          rpsfp::apertures_problem(m, radii, subpix), n, positions_host))
    return rc;
  s->photometry_ms = 0;
  if (n == 0) return RPSF_OK;  // nothing to launch
  HIP_TRY(hipSetDevice(s->device));
  const size_t columns = (size_t)rpsfp::photometry_columns(m);
  HIP_TRY(s->phot_pos.reserve(2 * n));
  HIP_TRY(s->phot_out.reserve(columns * n));
  HIP_TRY(hipMemcpy(s->phot_pos.p, positions_host, 2 * n * sizeof(double), hipMemcpyHostToDevice));
  const rpsfp::Apertures ap = rpsfp::make_apertures(m, radii, subpix);
  if (const int rc = timed(s, &s->photometry_ms, [&] {
        hipLaunchKernelGGL(stars_photometry_kernel, walk_grid(n), dim3(WALK_THREADS), rpsfp::s6_lds_bytes(m), nullptr, s->view(), s->level_f.p,
                           s->none.p, use_mesh != 0, ap, s->phot_pos.p, (long)n, s->phot_out.p);
      }))
    return rc;
  HIP_TRY(hipMemcpy(out_host, s->phot_out.p, columns * n * sizeof(double), hipMemcpyDeviceToHost));
  return RPSF_OK;
}

extern "C" int rpsf_stars_photometry_ms(const rpsf_stars* s, double* ms) {
  if (!s || !ms) return fail(RPSF_E_BADARG, "null argument");
  *ms = s->photometry_ms;
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------ S7 (Windowed positions)
extern "C" int rpsf_stars_refine(rpsf_stars* s, size_t n, const double* positions_host, const double* sigma_host, int max_iter, double eps,
                                 double max_shift, int use_mesh, double* out_host) {
  const auto sigma_problem = [&](size_t i) -> int {
    if (rpsfr::sigma_ok(sigma_host[i])) return RPSF_OK;
    return fail(RPSF_E_BADARG, "rpsf_stars_refine: sigma " + std::to_string(i) + " is not inside 0.5 <= sigma <= 16");
  };
  if (const int rc = check_positions_call("rpsf_stars_refine", s, s && (!n || (positions_host && sigma_host && out_host)),
                                          rpsfr::refine_problem(max_iter, eps, max_shift), n, positions_host, nullptr, 0.0, sigma_problem))
    return rc;
  s->refine_ms = 0;
  if (n == 0) return RPSF_OK;  // nothing to launch
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(s->refine_pos.reserve(2 * n));
  HIP_TRY(s->refine_sigma.reserve(n));
  HIP_TRY(s->refine_out.reserve(RPSF_STARS_REFINE_COLUMNS * n));
  HIP_TRY(hipMemcpy(s->refine_pos.p, positions_host, 2 * n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->refine_sigma.p, sigma_host, n * sizeof(double), hipMemcpyHostToDevice));
  const rpsfr::Refine rf = rpsfr::make_refine(max_iter, eps, max_shift);
  if (const int rc = timed(s, &s->refine_ms, [&] {
        hipLaunchKernelGGL(stars_refine_kernel, walk_grid(n), dim3(WALK_THREADS), rpsfr::s7_lds_bytes(), nullptr, s->view(), s->level_f.p,
                           s->none.p, use_mesh != 0, rf, s->refine_pos.p, s->refine_sigma.p, (long)n, s->refine_out.p);
      }))
    return rc;
  HIP_TRY(hipMemcpy(out_host, s->refine_out.p, RPSF_STARS_REFINE_COLUMNS * n * sizeof(double), hipMemcpyDeviceToHost));
  return RPSF_OK;
}

extern "C" int rpsf_stars_refine_ms(const rpsf_stars* s, double* ms) {
  if (!s || !ms) return fail(RPSF_E_BADARG, "null argument");
  *ms = s->refine_ms;
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------ S8 (Model fits)
extern "C" int rpsf_stars_model_create(int device, size_t n_cells, int N, const double* values_host, rpsf_stars_model** out) {
  if (!out || !values_host) return fail(RPSF_E_BADARG, "null argument");
  if (!rpsff::model_size_ok(N)) return fail(RPSF_E_BADARG, "rpsf_stars_model_create: the cells must be N x N with 4 <= N <= 256");
  if (n_cells < 1 || n_cells > ((size_t)1 << 24)) return fail(RPSF_E_BADARG, "rpsf_stars_model_create: the number of cells must lie in 1 ... 2^24");
  const size_t words = n_cells * (size_t)N * N;
  HIP_TRY(hipSetDevice(device));
  rpsf_stars_model* m = new rpsf_stars_model;
  m->device = device, m->n_cells = (int)n_cells, m->N = N;
  m->finite.assign(n_cells, 1);
  for (size_t k = 0; k < n_cells; ++k)
    for (size_t j = 0; j < (size_t)N * N && m->finite[k]; ++j) m->finite[k] = rpsfr::finite_d(values_host[k * (size_t)N * N + j]);
  auto made = [&]() -> int {
    HIP_TRY(m->values.reserve(words));
    HIP_TRY(hipMemcpy(m->values.p, values_host, words * sizeof(double), hipMemcpyHostToDevice));
    return RPSF_OK;
  };
  if (const int rc = made()) {
    delete m;
    return rc;
  }
  *out = m;
  return RPSF_OK;
}

void rpsf_detail_stars_model_view(const rpsf_stars_model* m, int* device, int* n_cells, int* N, const double** values_dev) {
  *device = m->device, *n_cells = m->n_cells, *N = m->N, *values_dev = m->values.p;
}

extern "C" void rpsf_stars_model_destroy(rpsf_stars_model* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  delete m;
}

extern "C" int rpsf_stars_fit(rpsf_stars* s, const rpsf_stars_model* model, size_t n, const double* positions_host, const int32_t* cells_host,
                              double radius, int fit_background, int use_mesh, double* out_host) {
  if (const int rc = check_positions_call("rpsf_stars_fit", s, s && model && (!n || (positions_host && cells_host && out_host)),
                                          rpsff::fit_problem(radius, fit_background), n, positions_host, model, radius))
    return rc;
  s->fit_ms = 0;
  if (n == 0) return RPSF_OK;  // nothing to launch
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(s->fit_pos.reserve(2 * n));
  HIP_TRY(s->fit_cell.reserve(n));
  HIP_TRY(s->fit_out.reserve(RPSF_STARS_FIT_COLUMNS * n));
  HIP_TRY(hipMemcpy(s->fit_pos.p, positions_host, 2 * n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->fit_cell.p, cells_host, n * sizeof(int32_t), hipMemcpyHostToDevice));
  const rpsff::Model cube{model->values.p, model->n_cells, model->N};
  const rpsff::Fit fit = rpsff::make_fit(radius, fit_background, model->N);
  if (const int rc = timed(s, &s->fit_ms, [&] {
        hipLaunchKernelGGL(stars_fit_kernel, walk_grid(n), dim3(WALK_THREADS), rpsff::s8_lds_bytes(), nullptr, s->view(), s->level_f.p, s->none.p,
                           use_mesh != 0, cube, fit, s->fit_pos.p, s->fit_cell.p, (long)n, s->fit_out.p);
      }))
    return rc;
  HIP_TRY(hipMemcpy(out_host, s->fit_out.p, RPSF_STARS_FIT_COLUMNS * n * sizeof(double), hipMemcpyDeviceToHost));
  return RPSF_OK;
}

extern "C" int rpsf_stars_fit_ms(const rpsf_stars* s, double* ms) {
  if (!s || !ms) return fail(RPSF_E_BADARG, "null argument");
  *ms = s->fit_ms;
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------ S9 (Fitted positions)
extern "C" int rpsf_stars_fit_positions(rpsf_stars* s, const rpsf_stars_model* model, size_t n, const double* positions_host,
                                        const int32_t* cells_host, double radius, int fit_background, int max_iter, double eps,
                                        double max_shift, double max_step, int use_mesh, double* iter_out_host, double* fit_out_host) {
  const char* why = rpsff::fit_problem(radius, fit_background);
  if (!why) why = rpsfg::fitpos_problem(max_iter, eps, max_shift, max_step);
  if (const int rc = check_positions_call("rpsf_stars_fit_positions", s,
                                          s && model && (!n || (positions_host && cells_host && iter_out_host && fit_out_host)), why, n,
                                          positions_host, model, radius))
    return rc;
  s->fitpos_ms = 0;
  if (n == 0) return RPSF_OK;  // nothing to launch
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(s->fitpos_pos.reserve(2 * n));
  HIP_TRY(s->fitpos_final.reserve(2 * n));
  HIP_TRY(s->fitpos_cell.reserve(n));
  HIP_TRY(s->fitpos_iter.reserve(RPSF_STARS_FITPOS_COLUMNS * n));
  HIP_TRY(s->fitpos_fit.reserve(RPSF_STARS_FIT_COLUMNS * n));
  HIP_TRY(hipMemcpy(s->fitpos_pos.p, positions_host, 2 * n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->fitpos_cell.p, cells_host, n * sizeof(int32_t), hipMemcpyHostToDevice));
  const rpsff::Model cube{model->values.p, model->n_cells, model->N};
  const rpsff::Fit fit = rpsff::make_fit(radius, fit_background, model->N);
  const rpsfg::FitPos fp = rpsfg::make_fitpos(max_iter, eps, max_shift, max_step);
  if (const int rc = timed(s, &s->fitpos_ms, [&] {
        const dim3 grid = walk_grid(n);
        hipLaunchKernelGGL(stars_fitpos_kernel, grid, dim3(WALK_THREADS), rpsfg::s9_lds_bytes(), nullptr, s->view(), s->level_f.p, s->none.p,
                           use_mesh != 0, cube, fit, fp, s->fitpos_pos.p, s->fitpos_cell.p, (long)n, s->fitpos_iter.p, s->fitpos_final.p);
        // S8 itself at the positions S9 ended at (the null stream orders the two)
        hipLaunchKernelGGL(stars_fit_kernel, grid, dim3(WALK_THREADS), rpsff::s8_lds_bytes(), nullptr, s->view(), s->level_f.p, s->none.p,
                           use_mesh != 0, cube, fit, s->fitpos_final.p, s->fitpos_cell.p, (long)n, s->fitpos_fit.p);
      }))
    return rc;
  HIP_TRY(hipMemcpy(iter_out_host, s->fitpos_iter.p, RPSF_STARS_FITPOS_COLUMNS * n * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(fit_out_host, s->fitpos_fit.p, RPSF_STARS_FIT_COLUMNS * n * sizeof(double), hipMemcpyDeviceToHost));
  return RPSF_OK;
}

extern "C" int rpsf_stars_fit_positions_ms(const rpsf_stars* s, double* ms) {
  if (!s || !ms) return fail(RPSF_E_BADARG, "null argument");
  *ms = s->fitpos_ms;
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------ S10 (Model and residual frames)
extern "C" int rpsf_stars_render(rpsf_stars* s, const rpsf_stars_model* model, size_t n, const double* positions_host, const double* flux_host,
                                 const int32_t* cells_host, double radius, int mode, int out_float64, int out_on_device, void* out,
                                 size_t* n_rendered) {
  if (!s || !model || !out || (n && (!positions_host || !flux_host || !cells_host))) return fail(RPSF_E_BADARG, "null argument");
  if (const char* why = rpsfn::render_problem(radius, mode)) return fail(RPSF_E_BADARG, std::string("rpsf_stars_render: ") + why);
  if (n > ((size_t)1 << 30)) return fail(RPSF_E_UNSUPPORTED, "rpsf_stars_render: more than 2^30 stars in one call");
  for (size_t i = 0; i < n; ++i)
    if (!rpsfp::position_ok(positions_host[2 * i], positions_host[2 * i + 1]))
      return fail(RPSF_E_BADARG, "rpsf_stars_render: position " + std::to_string(i) + " is not finite or not inside |y|, |x| < 2^20");
  if (!(radius <= rpsff::max_fit_radius(model->N)))
    return fail(RPSF_E_BADARG, "rpsf_stars_render: radius " + std::to_string(radius) + " is above min(64, N / 2 - 1) of the model's N = " +
                                   std::to_string(model->N));
  if (model->device != s->device) return fail(RPSF_E_BADARG, "rpsf_stars_render: the model is on another device than the finder");
  if (mode != rpsfn::MODE_MODEL && !s->have_mesh)
    return fail(RPSF_E_STATE, "rpsf_stars_render of a residual before a rpsf_stars_background_view / _host / _scaled of the frame");
  HIP_TRY(hipSetDevice(s->device));
  if (mode == rpsfn::MODE_RESIDUAL_MESH) {
    int none = 0;
    HIP_TRY(hipMemcpy(&none, s->none.p, sizeof(int), hipMemcpyDeviceToHost));
    if (none) return fail(RPSF_E_STATE, "rpsf_stars_render: the frame has no usable pixel, so there is no mesh to subtract");
  }
  s->render_ms = 0;
  std::vector<long long> offsets;
  std::vector<int> index;
  const size_t drawn = rpsfn::tile_lists(s->H, s->W, n, positions_host, flux_host, cells_host, model->n_cells, radius, offsets, index);
  const size_t npix = (size_t)s->npix(), item = out_float64 ? sizeof(double) : sizeof(float);
  HIP_TRY(s->render_pos.reserve(2 * n));
  HIP_TRY(s->render_flux.reserve(n));
  HIP_TRY(s->render_cell.reserve(n));
  HIP_TRY(s->render_offsets.reserve(offsets.size()));
  HIP_TRY(s->render_index.reserve(index.size()));
  if (!out_on_device) HIP_TRY(s->render_out.reserve(npix));
  if (n) {
    HIP_TRY(hipMemcpy(s->render_pos.p, positions_host, 2 * n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->render_flux.p, flux_host, n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->render_cell.p, cells_host, n * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  HIP_TRY(hipMemcpy(s->render_offsets.p, offsets.data(), offsets.size() * sizeof(long long), hipMemcpyHostToDevice));
  if (!index.empty()) HIP_TRY(hipMemcpy(s->render_index.p, index.data(), index.size() * sizeof(int), hipMemcpyHostToDevice));
  const rpsff::Model cube{model->values.p, model->n_cells, model->N};
  const rpsfn::Render rd = rpsfn::make_render(radius, mode, out_float64, model->N);
  const rpsfn::Stars st{s->render_pos.p, s->render_flux.p, s->render_cell.p, s->render_offsets.p, s->render_index.p};
  void* out_dev = out_on_device ? out : static_cast<void*>(s->render_out.p);
  if (const int rc = timed(s, &s->render_ms, [&] {
        const dim3 grid((unsigned)rpsfn::tiles_across(s->W), (unsigned)rpsfn::tiles_down(s->H));
        hipLaunchKernelGGL(stars_render_kernel, grid, dim3(WALK_THREADS), rpsfn::s10_lds_bytes(), nullptr, s->view(), s->level_f.p, cube, rd, st,
                           out_dev);
      }))
    return rc;
  if (!out_on_device) HIP_TRY(hipMemcpy(out, out_dev, npix * item, hipMemcpyDeviceToHost));
  if (n_rendered) *n_rendered = drawn;
  return RPSF_OK;
}

extern "C" int rpsf_stars_render_ms(const rpsf_stars* s, double* ms) {
  if (!s || !ms) return fail(RPSF_E_BADARG, "null argument");
  *ms = s->render_ms;
  return RPSF_OK;
}

extern "C" int rpsf_stars_render_info(int* tile_rows, int* tile_cols, int* chunk) {
  if (tile_rows) *tile_rows = rpsfn::RENDER_TILE_R;
  if (tile_cols) *tile_cols = rpsfn::RENDER_TILE_C;
  if (chunk) *chunk = rpsfn::RENDER_CHUNK;
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------ S11 (Group fits)
extern "C" int rpsf_stars_link_groups(size_t n, const double* positions_host, const uint8_t* eligible_host, double link, int max_group,
                                      int32_t* labels_host, int32_t* sizes_host, uint8_t* crowded_host) {
  if (n && (!positions_host || !labels_host || !sizes_host || !crowded_host)) return fail(RPSF_E_BADARG, "null argument");
  if (const char* why = rpsfq::link_problem(link, max_group)) return fail(RPSF_E_BADARG, std::string("rpsf_stars_link_groups: ") + why);
  if (n > ((size_t)1 << 30)) return fail(RPSF_E_UNSUPPORTED, "rpsf_stars_link_groups: more than 2^30 positions in one call");
  for (size_t i = 0; i < n; ++i)
    if (!rpsfp::position_ok(positions_host[2 * i], positions_host[2 * i + 1]))
      return fail(RPSF_E_BADARG, "rpsf_stars_link_groups: position " + std::to_string(i) + " is not finite or not inside |y|, |x| < 2^20");
  rpsfq::Groups groups;
  rpsfq::link_groups(n, positions_host, eligible_host, link, max_group, groups);
  for (size_t i = 0; i < n; ++i)
    labels_host[i] = groups.label[i], sizes_host[i] = groups.size[i], crowded_host[i] = groups.crowded[i] ? RPSF_STARS_FIT_CROWDED : 0;
  return RPSF_OK;
}

extern "C" int rpsf_stars_fit_groups(rpsf_stars* s, const rpsf_stars_model* model, size_t n, const double* positions_host,
                                     const int32_t* cells_host, double radius, int fit_background, int use_mesh, double link, int max_group,
                                     double* out_host) {
  const char* why = rpsff::fit_problem(radius, fit_background);
  if (!why) why = rpsfq::group_problem(link, max_group, radius);
  if (const int rc = check_positions_call("rpsf_stars_fit_groups", s, s && model && (!n || (positions_host && cells_host && out_host)), why, n,
                                          positions_host, model, radius))
    return rc;
  s->group_ms = 0;
  if (n == 0) return RPSF_OK;  // nothing to launch
  HIP_TRY(hipSetDevice(s->device));
  int none = 0;
  if (use_mesh) HIP_TRY(hipMemcpy(&none, s->none.p, sizeof(int), hipMemcpyDeviceToHost));
  // a star is fitted with others only when its cell is one of the model's and all finite, and the frame has the mesh it asks for
  std::vector<uint8_t> eligible(n);
  for (size_t i = 0; i < n; ++i) eligible[i] = !none && cells_host[i] >= 0 && cells_host[i] < model->n_cells && model->finite[(size_t)cells_host[i]];
  rpsfq::Groups groups;
  rpsfq::link_groups(n, positions_host, eligible.data(), link, max_group, groups);
  const size_t n_groups = groups.count(), n_members = groups.members.size(), n_lone = n - n_members;
  std::vector<uint8_t> grouped(n, 0);
  for (const int32_t i : groups.members) grouped[(size_t)i] = 1;
  std::vector<double> lone_pos(2 * n_lone);
  std::vector<int32_t> lone_cell(n_lone), lone(n_lone);
  for (size_t i = 0, k = 0; i < n; ++i)
    if (!grouped[i]) lone[k] = (int32_t)i, lone_pos[2 * k] = positions_host[2 * i], lone_pos[2 * k + 1] = positions_host[2 * i + 1], lone_cell[k++] = cells_host[i];
  const rpsff::Model cube{model->values.p, model->n_cells, model->N};
  const rpsff::Fit fit = rpsff::make_fit(radius, fit_background, model->N);
  if (n_lone) {
    HIP_TRY(s->group_lone_pos.reserve(2 * n_lone));
    HIP_TRY(s->group_lone_cell.reserve(n_lone));
    HIP_TRY(s->group_lone_out.reserve(RPSF_STARS_FIT_COLUMNS * n_lone));
    HIP_TRY(hipMemcpy(s->group_lone_pos.p, lone_pos.data(), 2 * n_lone * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->group_lone_cell.p, lone_cell.data(), n_lone * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  if (n_groups) {
    HIP_TRY(s->group_pos.reserve(2 * n));
    HIP_TRY(s->group_cell.reserve(n));
    HIP_TRY(s->group_starts.reserve(n_groups + 1));
    HIP_TRY(s->group_members.reserve(n_members));
    HIP_TRY(s->group_out.reserve(RPSF_STARS_FIT_GROUPS_COLUMNS * n_members));
    HIP_TRY(hipMemcpy(s->group_pos.p, positions_host, 2 * n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->group_cell.p, cells_host, n * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->group_starts.p, groups.starts.data(), (n_groups + 1) * sizeof(long long), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->group_members.p, groups.members.data(), n_members * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  if (const int rc = timed(s, &s->group_ms, [&] {
        // S8's own launch for every star that is alone: its rows are rpsf_stars_fit's
        if (n_lone)
          hipLaunchKernelGGL(stars_fit_kernel, walk_grid(n_lone), dim3(WALK_THREADS), rpsff::s8_lds_bytes(), nullptr, s->view(), s->level_f.p,
                             s->none.p, use_mesh != 0, cube, fit, s->group_lone_pos.p, s->group_lone_cell.p, (long)n_lone, s->group_lone_out.p);
        if (n_groups) {
          const rpsfj::GroupList list{s->group_starts.p, s->group_members.p, (long)n_groups};
          hipLaunchKernelGGL(stars_fit_group_kernel, walk_grid(n_groups), dim3(WALK_THREADS), rpsfj::s11_lds_bytes(), nullptr, s->view(),
                             s->level_f.p, use_mesh != 0, cube, fit, s->group_pos.p, s->group_cell.p, list, s->group_out.p);
        }
      }))
    return rc;
  std::vector<double> rows8(RPSF_STARS_FIT_COLUMNS * n_lone), rows11(RPSF_STARS_FIT_GROUPS_COLUMNS * n_members);
  if (n_lone) HIP_TRY(hipMemcpy(rows8.data(), s->group_lone_out.p, rows8.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (n_groups) HIP_TRY(hipMemcpy(rows11.data(), s->group_out.p, rows11.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t k = 0; k < n_lone; ++k) {  // a star alone: S8's row, and it is its own group
    const size_t i = (size_t)lone[k];
    const double* from = rows8.data() + RPSF_STARS_FIT_COLUMNS * k;
    double* o = out_host + RPSF_STARS_FIT_GROUPS_COLUMNS * i;
    for (int c = 0; c < RPSF_STARS_FIT_COLUMNS; ++c) o[c] = from[c];
    o[rpsfj::COL_GROUP] = (double)groups.label[i], o[rpsfj::COL_GROUP_SIZE] = (double)groups.size[i];
    o[rpsfj::COL_GROUP_N] = from[rpsff::COL_N], o[rpsfj::COL_GROUP_CHI2] = from[rpsff::COL_CHI2], o[rpsfj::COL_GROUP_ABS] = from[rpsff::COL_ABS_RES];
  }
  for (size_t k = 0; k < n_members; ++k) {
    const double* from = rows11.data() + RPSF_STARS_FIT_GROUPS_COLUMNS * k;
    double* o = out_host + RPSF_STARS_FIT_GROUPS_COLUMNS * (size_t)groups.members[k];
    for (int c = 0; c < RPSF_STARS_FIT_GROUPS_COLUMNS; ++c) o[c] = from[c];
  }
  return RPSF_OK;
}

extern "C" int rpsf_stars_fit_groups_ms(const rpsf_stars* s, double* ms) {
  if (!s || !ms) return fail(RPSF_E_BADARG, "null argument");
  *ms = s->group_ms;
  return RPSF_OK;
}

extern "C" int rpsf_stars_fit_groups_info(int* columns, int* max_group, int* groups_per_workgroup) {
  if (columns) *columns = rpsfj::GROUP_COLUMNS;
  if (max_group) *max_group = rpsfq::MAX_GROUP;
  if (groups_per_workgroup) *groups_per_workgroup = WALK_WAVES;
  return RPSF_OK;
}

extern "C" int rpsf_stars_label(rpsf_stars* s, const uint8_t* detected_host, int32_t* labels_host) {
  if (!s || !detected_host || !labels_host) return fail(RPSF_E_BADARG, "null argument");
  const size_t npix = (size_t)s->npix();
  HIP_TRY(hipSetDevice(s->device));
  std::vector<uint8_t> flags(npix);
  for (size_t i = 0; i < npix; ++i) flags[i] = detected_host[i] != 0;
  ++s->generation;
  HIP_TRY(hipMemcpy(s->det.p, flags.data(), npix, hipMemcpyHostToDevice));
  s->ms[2] = 0;
  if (const int rc = timed(s, &s->ms[2], [&] { launch_label(s); })) return rc;
  HIP_TRY(hipMemcpy(labels_host, s->labels.p, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
  return RPSF_OK;
}

extern "C" int rpsf_stars_info(const rpsf_stars* s, int* tile_rows, int* tile_cols) {
  if (!s) return fail(RPSF_E_BADARG, "null argument");
  if (tile_rows) *tile_rows = TILE_R;
  if (tile_cols) *tile_cols = TILE_C;
  return RPSF_OK;
}

extern "C" int rpsf_stars_kernel_ms(const rpsf_stars* s, double ms[4]) {
  if (!s || !ms) return fail(RPSF_E_BADARG, "null argument");
  for (int i = 0; i < 4; ++i) ms[i] = s->ms[i];
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------ the fused route
// one exact selection on many workgroups: a counting launch and a one-thread step launch per pass
static void launch_select_many(rpsf_stars* s, const rpsfm::Source& src, rpsfm::Sel* state) {
  const dim3 grid(rpsfm::many_workgroups(src.n));
  hipLaunchKernelGGL(stars_mesh_many_step_kernel, dim3(1), dim3(64), 0, nullptr, state, s->mesh_acc.p, -1);
  for (int step = 0; step < rpsfm::STEPS; ++step) {
    hipLaunchKernelGGL(stars_mesh_many_count_kernel, grid, dim3(rpsfm::S1B_THREADS), rpsfm::s1b_lds_bytes(), nullptr, src, state, step,
                       s->mesh_acc.p);
    hipLaunchKernelGGL(stars_mesh_many_step_kernel, dim3(1), dim3(64), 0, nullptr, state, s->mesh_acc.p, step);
  }
}

// S1b on s->level / s->rms (filled in place) into s->level_f / s->rms_f, s->mesh_out[0] and s->none; nothing comes back to the host
static int filter_mesh_on_device(rpsf_stars* s) {
  const long n = (long)s->nby * s->nbx;
  s->mesh_ms = 0;
  return timed(s, &s->mesh_ms, [&] {
    if (n <= rpsfm::MANY_NODES) {
      hipLaunchKernelGGL(stars_mesh_filter_kernel, dim3(1), dim3(rpsfm::S1B_THREADS), rpsfm::s1b_lds_bytes(), nullptr, s->nby, s->nbx,
                         s->level.p, s->rms.p, s->level_f.p, s->rms_f.p, s->mesh_out.p, s->none.p);
      return;
    }
    launch_select_many(s, rpsfm::Source{s->level.p, s->rms.p, n, 1}, s->mesh_state.p);
    hipLaunchKernelGGL(stars_mesh_many_fill_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, n, s->level.p, s->rms.p, s->mesh_state.p);
    hipLaunchKernelGGL(stars_mesh_many_filter_kernel, dim3(blocks_for(n)), dim3(256), 0, nullptr, s->nby, s->nbx, s->level.p, s->rms.p,
                       s->level_f.p, s->rms_f.p);
    launch_select_many(s, rpsfm::Source{s->rms_f.p, s->rms_f.p, n, 0}, s->mesh_state.p + 1);
    hipLaunchKernelGGL(stars_mesh_many_finish_kernel, dim3(1), dim3(64), 0, nullptr, s->mesh_state.p, s->mesh_state.p + 1, s->mesh_out.p,
                       s->none.p);
  });
}

// the tail every fused background entry shares: the frame is in s->frame (enqueued on the null stream); mask, S1, S1b
static int background_on_device(rpsf_stars* s, const uint8_t* mask_host_or_null) {
  if (const int rc = upload_mask(s, mask_host_or_null)) return rc;
  if (const int rc = mesh_on_device(s)) return rc;
  if (const int rc = filter_mesh_on_device(s)) return rc;
  s->have_frame = s->have_mesh = true;
  return RPSF_OK;
}

extern "C" int rpsf_stars_background_view(rpsf_stars* s, const rpsf_view* image, const uint8_t* mask_host_or_null) {
  if (!s || !image) return fail(RPSF_E_BADARG, "null argument");
  bool empty = false;
  if (const char* why = rpsfconv::view_problem(image, false, &empty)) return fail(RPSF_E_BADARG, std::string("image: ") + why);
  if (image->rows != s->H || image->cols != s->W)
    return fail(RPSF_E_BADARG, "the view is " + std::to_string(image->rows) + " x " + std::to_string(image->cols) + ", the finder's frame " +
                                   std::to_string(s->H) + " x " + std::to_string(s->W));
  HIP_TRY(hipSetDevice(s->device));
  s->have_frame = s->have_mesh = false;
  ++s->generation;
  if (rpsfconv::dense_f32(*image)) {  // the same bits, device to device; the caller's array is only ever read
    HIP_TRY(hipMemcpyAsync(s->frame.p, image->data, (size_t)s->npix() * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
  } else if (const int rc = rpsf_conv_gather(*image, 1, 0, s->frame.p, 0, nullptr)) {  // C1
    return rc;
  }
  return background_on_device(s, mask_host_or_null);
}

extern "C" int rpsf_stars_background_host(rpsf_stars* s, const void* image_host, int image_is_f64, const uint8_t* mask_host_or_null) {
  if (!s || !image_host) return fail(RPSF_E_BADARG, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  s->have_frame = s->have_mesh = false;
  ++s->generation;
  if (const int rc = upload_frame_f32(s->frame.p, image_host, image_is_f64, (size_t)s->npix())) return rc;
  return background_on_device(s, mask_host_or_null);
}

extern "C" int rpsf_stars_background_scaled(rpsf_stars* s, const void* image_host, int image_is_f64, int height, int width, int scale,
                                            const uint8_t* mask_host_or_null) {
  if (!s || !image_host) return fail(RPSF_E_BADARG, "null argument");
  if (scale < 2) return fail(RPSF_E_BADARG, "scale must be at least 2 here (scale 1: rpsf_stars_background_host)");
  if (height < 4 || width < 4) return fail(RPSF_E_BADARG, "the spline of the upscale needs at least 4 x 4 pixels");
  const long hs = 1 + (long)(height - 1) * scale, ws = 1 + (long)(width - 1) * scale;
  if (hs != s->H || ws != s->W)
    return fail(RPSF_E_BADARG, "the scaled frame is " + std::to_string(hs) + " x " + std::to_string(ws) + ", the finder's frame " +
                                   std::to_string(s->H) + " x " + std::to_string(s->W));
  HIP_TRY(hipSetDevice(s->device));
  s->have_frame = s->have_mesh = false;
  ++s->generation;
  if (!s->upscale) s->upscale = rpsf_detail_scale_scratch_new();
  // the unscaled frame crosses PCIe once, in its own type; U1 / U2 leave the scaled one, rounded to float32 once, where S1 reads it
  if (const int rc = rpsf_detail_scale_upload(s->upscale, image_host, image_is_f64, height, width)) return rc;
  if (const int rc = rpsf_detail_scale_run(s->upscale, image_is_f64, height, width, scale, s->frame.p, 1)) return rc;
  return background_on_device(s, mask_host_or_null);
}

extern "C" int rpsf_stars_filter_mesh(rpsf_stars* s, const double* level_host, const double* rms_host, double threshold, double* level_out,
                                      double* rms_out, double* global_rms, double* T, int* none) {
  if (!s || !level_host || !rms_host || !level_out || !rms_out || !global_rms || !T || !none) return fail(RPSF_E_BADARG, "null argument");
  const size_t nmesh = (size_t)s->nby * s->nbx;
  HIP_TRY(hipSetDevice(s->device));
  s->have_mesh = false;  // the meshes are the caller's, not the frame's
  ++s->generation;
  HIP_TRY(hipMemcpy(s->level.p, level_host, nmesh * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->rms.p, rms_host, nmesh * sizeof(double), hipMemcpyHostToDevice));
  if (const int rc = filter_mesh_on_device(s)) return rc;
  hipLaunchKernelGGL(stars_threshold_kernel, dim3(1), dim3(64), 0, nullptr, threshold, s->none.p, s->mesh_out.p);
  HIP_TRY(hipGetLastError());
  double out[2] = {0, 0};
  HIP_TRY(hipMemcpy(none, s->none.p, sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(out, s->mesh_out.p, sizeof out, hipMemcpyDeviceToHost));
  *T = out[rpsfm::OUT_T];
  if (*none) return RPSF_OK;  // no usable box: nothing else was written
  *global_rms = out[rpsfm::OUT_GLOBAL_RMS];
  HIP_TRY(hipMemcpy(level_out, s->level_f.p, nmesh * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(rms_out, s->rms_f.p, nmesh * sizeof(double), hipMemcpyDeviceToHost));
  return RPSF_OK;
}

extern "C" int rpsf_stars_detect_device(rpsf_stars* s, double threshold, long min_area, long max_area, size_t* count) {
  if (!s || !count) return fail(RPSF_E_BADARG, "null argument");
  if (!s->have_mesh) return fail(RPSF_E_STATE, "rpsf_stars_detect_device before a rpsf_stars_background_view / _host / _scaled of the frame");
  HIP_TRY(hipSetDevice(s->device));
  hipLaunchKernelGGL(stars_threshold_kernel, dim3(1), dim3(64), 0, nullptr, threshold, s->none.p, s->mesh_out.p);
  HIP_TRY(hipGetLastError());
  // no usable box: T = +inf, nothing is detected, *count stays 0
  return detect_on_device(s, s->level_f.p, s->mesh_out.p + rpsfm::OUT_T, 0.0, min_area, max_area, count);
}

extern "C" int rpsf_stars_frame(rpsf_stars* s, const float** frame_dev, int* height, int* width) {
  if (!s || !frame_dev) return fail(RPSF_E_BADARG, "null argument");
  if (!s->have_frame) return fail(RPSF_E_STATE, "rpsf_stars_frame before a frame was uploaded");
  *frame_dev = s->frame.p;
  if (height) *height = s->H;
  if (width) *width = s->W;
  return RPSF_OK;
}

extern "C" int rpsf_stars_mesh_ms(const rpsf_stars* s, double* ms) {
  if (!s || !ms) return fail(RPSF_E_BADARG, "null argument");
  *ms = s->mesh_ms;
  return RPSF_OK;
}

// ------------------------------------------------------------------------------------------------ S12 (Weighted fits)
// The variance frame takes the frame's own route into a float32 buffer of its own: no S1, no mask, and the frame, the meshes, the
// detections and `generation` stay what they were.
extern "C" int rpsf_stars_variance_view(rpsf_stars* s, const rpsf_view* variance) {
  if (!s || !variance) return fail(RPSF_E_BADARG, "null argument");
  bool empty = false;
  if (const char* why = rpsfconv::view_problem(variance, false, &empty)) return fail(RPSF_E_BADARG, std::string("variance: ") + why);
  if (variance->rows != s->H || variance->cols != s->W)
    return fail(RPSF_E_BADARG, "the view is " + std::to_string(variance->rows) + " x " + std::to_string(variance->cols) + ", the finder's frame " +
                                   std::to_string(s->H) + " x " + std::to_string(s->W));
  HIP_TRY(hipSetDevice(s->device));
  s->have_variance = false;
  HIP_TRY(s->variance.reserve((size_t)s->npix()));
  if (rpsfconv::dense_f32(*variance)) {  // the same bits, device to device; the caller's array is only ever read
    HIP_TRY(hipMemcpyAsync(s->variance.p, variance->data, (size_t)s->npix() * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
  } else if (const int rc = rpsf_conv_gather(*variance, 1, 0, s->variance.p, 0, nullptr)) {  // C1
    return rc;
  }
  s->have_variance = true;
  return RPSF_OK;
}

extern "C" int rpsf_stars_variance_host(rpsf_stars* s, const void* variance_host, int variance_is_f64) {
  if (!s || !variance_host) return fail(RPSF_E_BADARG, "null argument");
  HIP_TRY(hipSetDevice(s->device));
  s->have_variance = false;
  HIP_TRY(s->variance.reserve((size_t)s->npix()));
  if (const int rc = upload_frame_f32(s->variance.p, variance_host, variance_is_f64, (size_t)s->npix())) return rc;
  s->have_variance = true;
  return RPSF_OK;
}

extern "C" int rpsf_stars_fit_weighted(rpsf_stars* s, const rpsf_stars_model* model, size_t n, const double* positions_host,
                                       const int32_t* cells_host, double radius, int fit_background, int use_mesh, int variance_mode,
                                       double sky_variance, double gain, double* out_host) {
  const char* why = rpsff::fit_problem(radius, fit_background);
  if (!why) why = rpsfw::variance_problem(variance_mode, sky_variance, gain);
  if (const int rc = check_positions_call("rpsf_stars_fit_weighted", s, s && model && (!n || (positions_host && cells_host && out_host)), why, n,
                                          positions_host, model, radius))
    return rc;
  if (variance_mode == RPSF_STARS_VARIANCE_MAP && !s->have_variance)
    return fail(RPSF_E_STATE, "rpsf_stars_fit_weighted with RPSF_STARS_VARIANCE_MAP before a rpsf_stars_variance_view / _host");
  s->fitw_ms = 0;
  if (n == 0) return RPSF_OK;  // nothing to launch
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(s->fitw_pos.reserve(2 * n));
  HIP_TRY(s->fitw_cell.reserve(n));
  HIP_TRY(s->fitw_out.reserve(RPSF_STARS_FIT_WEIGHTED_COLUMNS * n));
  HIP_TRY(hipMemcpy(s->fitw_pos.p, positions_host, 2 * n * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(s->fitw_cell.p, cells_host, n * sizeof(int32_t), hipMemcpyHostToDevice));
  const rpsff::Model cube{model->values.p, model->n_cells, model->N};
  const rpsff::Fit fit = rpsff::make_fit(radius, fit_background, model->N);
  const rpsfw::Variance var{variance_mode == RPSF_STARS_VARIANCE_MAP ? s->variance.p : nullptr, variance_mode, sky_variance, gain};
  if (const int rc = timed(s, &s->fitw_ms, [&] {
        hipLaunchKernelGGL(stars_fit_weighted_kernel, walk_grid(n), dim3(WALK_THREADS), rpsfw::s12_lds_bytes(), nullptr, s->view(), s->level_f.p,
                           s->none.p, use_mesh != 0, cube, fit, var, s->fitw_pos.p, s->fitw_cell.p, (long)n, s->fitw_out.p);
      }))
    return rc;
  HIP_TRY(hipMemcpy(out_host, s->fitw_out.p, RPSF_STARS_FIT_WEIGHTED_COLUMNS * n * sizeof(double), hipMemcpyDeviceToHost));
  return RPSF_OK;
}

extern "C" int rpsf_stars_fit_weighted_ms(const rpsf_stars* s, double* ms) {
  if (!s || !ms) return fail(RPSF_E_BADARG, "null argument");
  *ms = s->fitw_ms;
  return RPSF_OK;
}
