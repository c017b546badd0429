/* rpsf.h - C ABI of the MI355X patch-wise PSF-correction library (librpsf_hip.so).
 *
 * The reference (punch-mission/regularizepsf 1.2.0) is pure Python and has no FFI seam of its
 * own; the boundary it offers is the class API.  Each entry point below states which reference
 * lines it stands in for, so that a reference maintainer can bind it with ctypes (see
 * INTEGRATION.md for the stub).  Conventions:
 *   - plain pointers and sizes only; no C++ / torch types cross the boundary;
 *   - every function returns 0 on success or a negative RPSF_E_* code; rpsf_last_error() returns a
 *     thread-local human-readable message for the last failure on the calling thread;
 *   - host pointers are borrowed for the duration of the call only; a plan owns all of its device
 *     memory; nothing returned by the library is freed by the caller except through *_destroy/_free;
 *   - a plan is bound to one device and is not re-entrant; distinct plans may be used from
 *     distinct threads;
 *   - applies of distinct plans on distinct streams may run on the device at the same time.  The launches of the
 *     128- and 256-pixel plans are persistent (workgroups that stay resident and draw patches from queues) and contain
 *     workgroups that wait for others of the same launch; they need no particular number of resident workgroups to
 *     finish - every patch is drawn from a queue by whichever workgroups are resident - as long as the few (<= 160)
 *     summing workgroups at the head of all concurrent launches together leave one compute unit free on every XCD
 *     (csrc/rpsf_launch.hpp, launch_decide, "FORWARD PROGRESS"; rpsf_plan_set_cu_mask below for plans on a part of the chip).
 */
#ifndef RPSF_H
#define RPSF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPSF_OK 0
#define RPSF_E_BADARG (-1)      /* null pointer, negative size, coordinate outside the padded image ... */
#define RPSF_E_UNSUPPORTED (-2) /* patch size outside 2..4096; or a size without a compiled plan (compiled: 16, 32, 64,
                                   128, 256) when libhipfft.so, which the fallback needs, cannot be loaded */
#define RPSF_E_HIP (-3)         /* HIP runtime error (message has the hipError string) */
#define RPSF_E_NOMEM (-4)       /* device allocation failed */
#define RPSF_E_RCCL (-5)        /* RCCL missing or failed */
#define RPSF_E_STATE (-6)       /* call order: e.g. apply before a transfer kernel was set */

/* np.pad modes evaluated inside the kernel (regularizepsf/transform.py:119-123 passes pad_mode to
 * np.pad).  Any other np.pad mode is handled by the Python layer, which pads on the host and calls
 * the library on the padded image with RPSF_PAD_CONSTANT. */
#define RPSF_PAD_CONSTANT 0
#define RPSF_PAD_SYMMETRIC 1
#define RPSF_PAD_REFLECT 2
#define RPSF_PAD_EDGE 3
#define RPSF_PAD_WRAP 4

typedef struct rpsf_plan rpsf_plan;

const char* rpsf_last_error(void);
int rpsf_device_count(int* count);
/* Compute-unit count and name of a device (for reporting). */
int rpsf_device_info(int device, int* compute_units, char* name, size_t name_len);

/* A plan is the device-side form of one ArrayPSFTransform: patch size N (psf_shape, square,
 * regularizepsf/transform.py:37-40), the patch corner list (transform.coordinates, (row, col) pairs,
 * transform.py:141-149) and, once installed, the transfer kernel.  N = 16, 32, 64, 128, 256 use the
 * hand-written kernels; any other N in 2..4096 (the reference takes every size) a hipFFT-based fallback with
 * the same results and tolerance (whole-image geometry only). */
int rpsf_plan_create(rpsf_plan** out, int device, int patch_size, int n_patches, const int32_t* coords_rc);
void rpsf_plan_destroy(rpsf_plan* plan);

/* Install the transfer kernel K (IndexedCube values of ArrayPSFTransform, complex64 interleaved,
 * shape (n_patches, N, N), transform.py:164).  The library folds it to its Hermitian part and
 * re-orders it into the layout the patch kernel streams.  host: pageable host memory. */
int rpsf_plan_set_transfer(rpsf_plan* plan, const float* k_c64_host);
/* Same, from a device-resident full K (e.g. produced by rpsf_build_transfer_device). */
int rpsf_plan_set_transfer_device(rpsf_plan* plan, const void* k_c64_device);
/* The same from the two PSF spectra K is built from (ArrayPSFTransform.construct, transform.py:78-82; complex64 (n_patches, N, N) each, on
 * the plan's device, e.g. left there by rpsf_psf_fft_device): the formula is evaluated where the packer reads K, so the full K is never
 * written or read back - 2 x n N^2 x 8 B in, the packed n N (N/2 + 1) x 8 B out, bit-identical to rpsf_build_transfer_device followed by
 * rpsf_plan_set_transfer_device. */
int rpsf_plan_set_transfer_spectra_device(rpsf_plan* plan, const void* s_c64_dev, const void* t_c64_dev, double alpha, double epsilon);
/* Overlap-add strategy (transform.py:167-169).  0 = automatic: on a regular half-overlap lattice of
 * corners (calculate_covering output) patches of equal lattice parity never overlap, so each patch
 * stores into one of four colour planes with plain coalesced stores and the planes are summed in a
 * fixed order (deterministic) - inside the same launch for 256-pixel patches, by a small kernel
 * otherwise; any other corner list falls back to float atomics.
 * 1 = force atomics, 2 = force planes (error if the corners are not a lattice), 3 = direct: every
 * lattice tile is accumulated in the output image itself, through the L2 of the XCD that runs most of
 * its patches, in processing order (deterministic; 128- and 256-pixel patches on a lattice only;
 * measured slower than the planes, kept for comparison).
 * 4 = sweep (what 0 selects for 16-, 32- and 64-pixel patches on a complete lattice of at least 2 x 2 patches):
 * a workgroup owns a region of OUTPUT pixels, walks every patch that touches it and adds the four
 * contributions of a pixel in LDS, in a fixed order (lattice rows top-down, even patch columns before odd
 * ones: bit-reproducible and independent of how the lattice is cut); every output pixel is written once,
 * by the one launch that is the whole apply.  Patches on region borders are computed by both neighbours. */
int rpsf_plan_set_overlap_mode(rpsf_plan* plan, int mode);
/* Sweep kernel (mode 4): cut the lattice into about `target_regions` regions of output pixels (one workgroup each; default: the device's
 * number of compute units).  More regions: shorter regions and a better balance over the CUs, more patches computed twice on region
 * borders.  The result does not depend on the cut, bit for bit.  rpsf_plan_sweep_info reports the cut in use: regions, jobs (slabs of
 * 128 / N patches), patch slots computed (/ the number of patches = the recompute factor), slabs per column parity and lattice row
 * of a region.  (The reference has no counterpart: transform.py:157-169 is one NumPy expression per step.) */
int rpsf_plan_set_sweep_regions(rpsf_plan* plan, int target_regions);
/* Launch options of a plan that tests and callers may pin (everything else is decided by the library; none changes a result beyond the
 * round-off of a different addition order, and the persistent / fused forms are bit-identical to their plain counterparts).
 * ENVIRONMENT: the shipped library reads exactly two variables, both for the host-side thread pool of the host-array entry points:
 *   RPSF_HOST_THREADS  (threads of the pool, default: the cores of the device's NUMA node, at most 16)
 *   RPSF_HOST_AFFINITY (0: do not bind the pool's threads to the device's NUMA node).
 * The development knobs of earlier rounds (RPSF_STRIPS, RPSF_SUM_FIRST, RPSF_V1, ...) are compiled in only with -DRPSF_DEV_ENV. */
enum {
  RPSF_OPT_PERSIST = 1,       /* 0 / 1: persistent patch workgroups for 128- and 256-pixel plans (default 1) */
  RPSF_OPT_FUSE = 2,          /* 0 / 1: colour-plane sum inside the patch launch where the geometry allows (default 1) */
  RPSF_OPT_K_CACHED = 3,      /* 0 / 1: transfer kernel by plain instead of streaming loads (default: by its size) */
  RPSF_OPT_PLANE_NT = 4,      /* -1 automatic, 0 / 1: streaming hint on the colour-plane stores of 128-pixel batches */
  RPSF_OPT_HOST_BANDS = 5,    /* -1 automatic, else the row bands a single host frame is cut into (0 or 1: none) */
  RPSF_OPT_STREAM_GROUP = 6,  /* 0 automatic, else frames per group of the streamed host path */
  RPSF_OPT_STREAM_DEPTH = 7,  /* 0 automatic, else groups in flight of the streamed host path */
  RPSF_OPT_DEBUG_ORPHAN = 8,  /* testing aid of the direct overlap-add: every value-th workgroup behaves as if placed on a foreign XCD */
  RPSF_OPT_HEAD_KPREFETCH = 9, /* 0 / 1: persistent launches of a 256-pixel plan - the head summing workgroups touch the transfer kernel of the
                                 first round's patches before they sum (default 0: measured a loss; ignored by other plans).
                                 Changes no value of the result. */
  RPSF_OPT_SAT_GROUP = 10,    /* 0 automatic (scratch under 1 GiB), else 1..65535 frames per frame-group of the batched device
                                 saturation route.  Changes no value of the result. */
  RPSF_OPT_PIPELINE = 11      /* 0 / 1: back-to-back rpsf_apply_device calls of a 256-pixel plan with stream == NULL alternate between two streams
                                 of the plan, so that the head of one apply runs under the tail of the last (default 1 for 256-pixel plans, ignored
                                 by the others).  Applies still complete in call order per pixel; everything else
                                 the plan does joins the two streams first.  A plan whose stream handle was taken (rpsf_plan_stream) keeps
                                 to one stream until the option is set to 1 again; a plan with a CU mask keeps to one for good.  Changes no
                                 value of the result. */
};
int rpsf_plan_set_option(rpsf_plan* plan, int option, int value);
/* The launch lanes of the plan (of a view: its parent's), read-only and host-side: info[0], info[1] the pipelined applies begun so far on the
 * plan's public stream and on its second stream, info[2] those of them that were begun while the previous apply might still run (they wait
 * for its tile sums), info[3] the times an operation that is not a pipelined apply found the second stream busy and made the public stream
 * wait for it, info[4] whether RPSF_OPT_PIPELINE is in force (0 / 1), info[5] whether the plan keeps to one stream because its stream handle
 * was taken (0 / 1).  Enqueues nothing and waits for nothing. */
int rpsf_plan_lane_info(const rpsf_plan* plan, long info[6]);
int rpsf_plan_sweep_info(const rpsf_plan* plan, int* regions, long* jobs, long* patch_slots, int* slabs_per_phase);
/* Row bands the last single host frame (rpsf_apply_host / rpsf_apply, one frame) was cut into: 0 = it went as a whole.  A frame of B bands
 * cannot take less than PCIe's duplex time x (1 + 1/B) (bench.py's e2e.pcie_floor_ms). */
int rpsf_plan_host_bands(const rpsf_plan* plan, int* bands);
/* Start-up stagger of the patch kernel's first resident workgroups (microseconds, 0 = off): spreads
 * the gather / K-stream / store phases of different CUs in time so that HBM traffic overlaps compute.
 * Without this call the library decides: 12 us for the persistent launches of the 256-pixel plan from
 * 256 patches on (24 us from 2048 on), none otherwise. */
int rpsf_plan_set_stagger(rpsf_plan* plan, int microseconds);
/* The persistent launch of the 256-pixel plan keeps one workgroup on every CU until its patches are done, so a kernel
 * enqueued beside it on another stream - RCCL's send/recv of the seam rows (rpsf_comm_seam_exchange) - would wait for the
 * first of them to finish.  `cus` CUs (0..128; 8 is what the sharded apply asks for) are left without a patch workgroup. */
int rpsf_plan_set_reserved_cus(rpsf_plan* plan, int cus);
/* Partition the chip between the plan and a caller's own stream: the plan's stream (and every launch on it) is confined to the compute
 * units set in `mask` (bit i of word i / 32, hipExtStreamCreateWithCUMask's numbering; `words` uint32), its persistent launches are
 * sized for them; rpsf_stream_create makes a stream masked to whatever the caller passes (NULL: unmasked).  The pipelined seam exchange
 * gives RCCL's kernels and K4 a handful of CUs of their own this way (rpsf_plan_set_reserved_cus only leaves CUs unclaimed - a kernel
 * dispatched a moment before the persistent launch still lands on CUs that launch is waiting for).  A masked plan gives up its second
 * launch lane, which is not masked: RPSF_OPT_PIPELINE has no effect on it from then on.  A mask of fewer than 8 CUs is refused (RPSF_E_BADARG), but a mask is
 * meant to take a FEW CUs off the chip (the sharded step: 8 of 256).  The fused launches put up to 32 (256-pixel plan) or 160 (128-pixel
 * plan, four to a CU) head summing workgroups in front of the patches by the amount of work alone, and need room beside them, on every
 * XCD, for a patch workgroup: on a plan masked to fewer than 40 CUs (256-pixel plan) or 42 CUs (128-pixel plan) an apply of 512
 * patch-frames or more may NEVER END, and a mask that leaves some XCD only a few CUs is no safer at a larger count
 * (csrc/rpsf_launch.hpp, FORWARD PROGRESS; tests/test_launch_host.py records where a model of the launch stalls).  An apply on a caller's
 * own masked stream is NOT sized by that stream's mask - the library cannot see it - but by the plan's own CU count (the device's, or the
 * last rpsf_plan_set_cu_mask), and the same limits apply to that stream's CUs. */
int rpsf_plan_set_cu_mask(rpsf_plan* plan, const uint32_t* mask, int words);
int rpsf_stream_create(int device, const uint32_t* mask, int words, void** stream);
int rpsf_stream_destroy(void* stream);
/* Opt-in image prefetch for streams of NEW frames (256-pixel plan, single-frame applies; ignored elsewhere): the summing workgroups at
 * the head of the persistent launch touch the image tile by tile, in the order in which the patches will gather it, as a paced side
 * job.  A frame that was not corrected a moment ago is not in the memory-side cache, and its first gathers pay the HBM latency
 * (transform.py:157-162 is the gather): -4 % per apply on a stream of different 4096^2 frames, nothing on a repeated one; frames
 * larger than the cache (8192^2) lose 8 %, which is why the library does not decide this by itself. */
int rpsf_plan_set_image_prefetch(rpsf_plan* plan, int on);
/* Development aid: in builds compiled with -DRPSF_STAMPS the patch kernel records 16 phase
 * timestamps per patch (10 ns ticks); this copies them out.  All zeros in a normal build. */
int rpsf_plan_debug_stamps(rpsf_plan* plan, unsigned long long* host, size_t count);
/* Bytes of packed transfer kernel the patch kernel reads per apply (for roofline accounting). */
int rpsf_plan_transfer_bytes(const rpsf_plan* plan, size_t* bytes);

/* Image geometry of one apply call.  The reference pads the image by 2N on every side with
 * np.pad(mode) and slices patch (r, c) at padded[r+2N : r+3N, c+2N : c+3N] (transform.py:119-123,
 * 141-149); here padding is an index map evaluated inside the kernel against the FULL image shape
 * (height, width).  origin_* is added to every patch corner (used when the caller hands over an
 * already padded image).  image_row0/image_rows and out_row0/out_rows describe which rows of the
 * full image / full output are resident at the device pointers (row-band sharding); for a whole
 * image they are 0 and height.
 * ld_image / ld_out are the row strides in floats (>= width, any value); the pointers and the frame strides of a batch need the
 * alignment of a float and no more.  The library chooses 16-byte, 8-byte or pixel-wise accesses per call from these numbers; on
 * every overlap-add mode but the atomics the result has the same bits whichever it chooses.  Of the output, columns [0, width) of
 * the resident rows are written and nothing else: not the floats between two rows, before the pointer, behind the last row or
 * between the frames of a batch (tests/test_gpu_geometry.py).  A call that is refused (RPSF_E_BADARG for a geometry outside these
 * bounds, RPSF_E_UNSUPPORTED for a row window on a plan of the hipFFT fallback) has written nothing. */
typedef struct rpsf_geometry {
  int height, width;
  int pad_mode;
  float pad_value;
  int origin_row, origin_col;
  int image_row0, image_rows, ld_image;
  int out_row0, out_rows, ld_out;
} rpsf_geometry;

/* ArrayPSFTransform.apply, transform.py:117-177 without the saturation branch (:125-138,:171-172,
 * done by the Python layer): float32 image (height, width) in, float32 corrected image out. */
int rpsf_apply(rpsf_plan* plan, const float* image_host, int height, int width, int pad_mode, float pad_value,
               float* out_host);
/* The same call for the dtypes ArrayPSFTransform.apply really sees: the image as float32 or float64
 * (image_is_f64; apply casts with astype, transform.py:117) and the result as float32 or float64
 * (out_is_f64; the reference returns float64, transform.py:174-177).  The conversions run on the library's persistent
 * worker pool (created at the first such call of the process, RPSF_HOST_THREADS wide, default min(16, cores); no
 * thread or buffer is created per call), chunk by chunk through the plan's pinned staging, overlapped with the PCIe
 * copies.  rpsf_apply above is this call with float32 on both sides. */
int rpsf_apply_host(rpsf_plan* plan, const void* image_host, int image_is_f64, int height, int width, int pad_mode,
                    float pad_value, void* out_host, int out_is_f64);
/* ArrayPSFTransform.apply with a finite saturation_threshold, whole (transform.py:117-138,171-177): float64 copy, np.pad by
 * 2N (pad_mode's index map on the host), mask = padded > threshold, binary dilation with scipy's default cross element
 * (dilation >= 1 iterations), NaN, the sequential row-major nanmean fill over [i - w/2, i + w/2) (neighborhood_width >= 0),
 * the correction of the padded frame on the GPU, the raw values restored on the mask, the crop.  The host steps are the
 * reference's, in its order, on the plan's own scratch; only the rows the patches read and the rows the caller gets cross
 * PCIe.  (dilation < 1, negative widths and np.pad modes the kernel does not know stay with the Python layer's NumPy route.) */
int rpsf_apply_host_saturated(rpsf_plan* plan, const void* image_host, int image_is_f64, int height, int width, int pad_mode,
                              double threshold, int dilation, int neighborhood_width, void* out_host, int out_is_f64);
/* The same for a sequence of frames of one shape, one pointer per frame - the reference's example corrects a list of frames this way
 * (`[transform.apply(image, saturation_threshold=...) for image in images]`, docs/source/example.ipynb cell 25): the host steps of
 * frame i + 1 run while the GPU corrects frame i (two staging slots in turn). */
int rpsf_apply_frames_host_saturated(rpsf_plan* plan, const void* const* images_host, int image_is_f64, int n_frames, int height,
                                     int width, int pad_mode, double threshold, int dilation, int neighborhood_width,
                                     void* const* outs_host, int out_is_f64);
/* The saturation branch with every step on the device (kernels F1 - F5, csrc/saturation.hip; DESIGN.md 3.8 has the definition):
 * image_dev is a float32 height x width frame on the plan's device, out_dev receives the float32 height x width result.  The frame is
 * padded by 2N with pad_mode's index map, thresholded ((double)value > threshold; NaN is not hot), the mask dilated `dilation` >= 1
 * times with the cross element, the masked pixels filled in row-major order with the float64 nan-mean of [i - w/2, i + w/2) x
 * [j - w/2, j + w/2) (Python slice rules; later pixels see earlier fills), the padded float32 frame corrected with the geometry
 * rpsf_apply_host_saturated uses, the raw values restored on the mask and the frame cropped: on a float32 frame the result has the
 * bits of rpsf_apply_host_saturated's.  Arguments as there, and neighborhood_width / 2 >= 1 (an always-empty window needs no kernel:
 * RPSF_E_BADARG, use the host route).  Asynchronous on `stream` (NULL: the plan's own) EXCEPT that the call waits for the stream once,
 * after the labelling, to read the hot, masked and group counts; with nothing hot F2 - F4 do nothing and the padded frame is corrected
 * as it is.  *n_masked_or_null: masked pixels of the padded frame.  The frame is a frame-group of one on the route of
 * rpsf_apply_batch_device_saturated (there is one driver), with F4's workgroups in the group table's own order, the ascending order of
 * the groups' first pixels: no ordering pass runs.  rpsf_saturation_batch_info is left as it was.
 * SCRATCH, owned by the plan, shared with the batch entry points, allocated at the first call, reused, grown when a larger frame arrives, freed with the plan: per pixel
 * of the padded (height + 4N) x (width + 4N) frame 4 B (float32 frame) + 3 B (hot / mask / grown mask bytes) + 4 B (labels) = 11 B,
 * plus the padded float32 output rows (4 B per pixel of height + 4N rows for a generic-size plan, of `height` rows otherwise), 8 B per
 * 64-pixel row segment, and per MASKED pixel 8 B (float64 fill) + at most 8 B (the list, device and pinned host), 24 B per group. */
int rpsf_apply_device_saturated(rpsf_plan* plan, const void* image_dev, void* out_dev, int height, int width, int pad_mode,
                                double threshold, int dilation, int neighborhood_width, void* stream, size_t* n_masked_or_null);
/* rpsf_apply_host_saturated's contract through the device route (rpsf_apply_frames_host_saturated_device's steps for one frame, in
 * the group table's own order, the batch info left as it was): the UNPADDED frame is narrowed to float32 and uploaded through the
 * plan's staging, rpsf_apply_device_saturated's route runs, `height` rows come back, and for a float64 frame the masked in-frame pixels, which
 * the device lists, receive the caller's own float64 values.  A float64 frame is thresholded and filled from its float32 rounding
 * (what every device path of the library holds): a pixel whose float64 value lies on the other side of the threshold from its float32
 * rounding is the one place where the two routes can disagree beyond the rounding of the fill's inputs. */
int rpsf_apply_host_saturated_device(rpsf_plan* plan, const void* image_host, int image_is_f64, int height, int width, int pad_mode,
                                     double threshold, int dilation, int neighborhood_width, void* out_host, int out_is_f64);
/* Device time of the last F1 ... F5 launches of the plan, milliseconds (F3's includes the host's one wait; zeros for what did not run):
 * of the LAST frame-group, all its frames together - after a single-frame call that frame, after a batch call
 * (rpsf_apply_batch_device_saturated and its kin) the batch's last frame-group. */
int rpsf_saturation_kernel_ms(rpsf_plan* plan, double ms[5]);
/* Test entry: F1 - F4 alone on a float32 host frame.  padded_host ((height + 4N) x (width + 4N) float32) receives the filled padded
 * frame, mask_host (as many bytes) the dilated mask; *n_groups_or_null: independent groups found.  rpsf_saturation_fill_batch_device
 * for one frame with order 2, and with reverse_groups != 0 order 1: F4's workgroups take the groups shortest first instead of in the
 * table's own order (the result must not depend on it).  Leaves rpsf_saturation_batch_info as it was. */
int rpsf_saturation_fill_device(rpsf_plan* plan, const float* image_host, int height, int width, int pad_mode, double threshold,
                                int dilation, int neighborhood_width, int reverse_groups, float* padded_host, uint8_t* mask_host,
                                int* n_groups_or_null);
/* rpsf_apply_device_saturated for n_frames float32 frames of one shape on the plan's device, image_stride floats apart (>= height x
 * width, any alignment); frame f of the result goes to outs_dev + f x out_stride (>= height x width), the floats between two frames
 * stay untouched.  Frame by frame the result has the bits of rpsf_apply_device_saturated's.  The batch is cut into frame-groups
 * (RPSF_OPT_SAT_GROUP; automatic: as many frames as keep the scratch below under 1 GiB).  A frame-group shares every launch of F1 - F3
 * (the frame is a grid index; labels, roots and counters stay per frame), the host waits for the stream ONCE per frame-group, not per
 * frame, F4 is one launch of one wave per group over all frames' groups, longest groups first, the correction is the shared-K batch
 * launch of rpsf_apply_batch_device on the padded frames, F5 one launch; n_frames == 1 takes the same steps, ordering pass included.
 * Argument checks as rpsf_apply_device_saturated
 * (neighborhood_width / 2 < 1: RPSF_E_BADARG), n_frames < 0: RPSF_E_BADARG, a stride below height x width with n_frames > 1:
 * RPSF_E_BADARG, n_frames == 0: RPSF_OK and nothing is done (the pointers may then be NULL).  RPSF_E_UNSUPPORTED when a frame-group
 * holds 2^31 masked pixels or more (cut it smaller).  n_masked_per_frame_or_null: n_frames entries, masked pixels of padded frame f.
 * SCRATCH per frame of a frame-group: what rpsf_apply_device_saturated lists for one frame (every per-frame array starts on a
 * multiple of 4 elements), 32 B of counters and offsets, and the batch launch's own 16 B per output pixel; 8 B more per group. */
int rpsf_apply_batch_device_saturated(rpsf_plan* plan, const void* images_dev, void* outs_dev, int n_frames, size_t image_stride,
                                      size_t out_stride, int height, int width, int pad_mode, double threshold, int dilation,
                                      int neighborhood_width, void* stream, size_t* n_masked_per_frame_or_null);
/* rpsf_apply_host_saturated_device's contract for n_frames host frames of one shape and type, per frame-group: the frames are narrowed
 * to float32 into the plan's page-locked staging and uploaded, rpsf_apply_batch_device_saturated's route runs, `height` rows per frame
 * come back, and for float64 input every frame's listed pixels receive the caller's own float64 values.  A frame-group's upload is not
 * overlapped with the previous group's kernels.  n_frames == 0: RPSF_OK. */
int rpsf_apply_frames_host_saturated_device(rpsf_plan* plan, const void* const* images_host, int image_is_f64, int n_frames, int height,
                                            int width, int pad_mode, double threshold, int dilation, int neighborhood_width,
                                            void* const* outs_host, int out_is_f64);
/* Of the last batch call of the plan (either entry above, or the test entry below; a single-frame call changes nothing): info[0] frames, info[1] frame-groups (= host waits
 * before F4), info[2] fill groups over all frames, info[3] masked pixels of the padded frames (saturating at INT_MAX).  Zeros before
 * the first.  After a batch call rpsf_saturation_kernel_ms reports F1 ... F5 of the LAST frame-group (F4 with its ordering pass). */
int rpsf_saturation_batch_info(rpsf_plan* plan, int info[4]);
/* Test entry: F1 - F4 alone on n_frames float32 host frames (contiguous, height x width each), cut into frame-groups as above.
 * padded_host (n_frames x (height + 4N) x (width + 4N) float32, dense) receives the filled padded frames, masks_host (as many bytes)
 * the dilated masks, groups_per_frame_or_null[f] the independent groups of frame f.  order: 0 F4's workgroups take the groups longest
 * first, 1 that order reversed, 2 the group table's own order (frame by frame); the result must not depend on it. */
int rpsf_saturation_fill_batch_device(rpsf_plan* plan, const float* images_host, int n_frames, int height, int width, int pad_mode,
                                      double threshold, int dilation, int neighborhood_width, int order, float* padded_host,
                                      uint8_t* masks_host, int* groups_per_frame_or_null);
/* Same with image and output already resident on the plan's device; asynchronous on `stream`
 * (a hipStream_t, or NULL for the plan's own stream).  Every pixel of the resident output rows is written
 * (uncovered ones with 0).  image_dev / out_dev must be ordinary device memory of the plan's device
 * (hipMalloc: coarse-grained) - the atomic overlap-add mode uses hardware float atomics, which
 * fine-grained or host-mapped memory does not support.  A plan serves one apply at a time: a call on a
 * different stream than the previous one waits for that one (the plan's scratch is shared).  With stream == NULL, back-to-back applies of a
 * 256-pixel plan may overlap head under tail (RPSF_OPT_PIPELINE); they complete in call order per pixel, and every other call on the plan,
 * rpsf_device_synchronize included, sees them complete as before. */
int rpsf_apply_device(rpsf_plan* plan, const void* image_dev, void* out_dev, const rpsf_geometry* geom, void* stream);
/* Run `iters` back-to-back device-resident applies on the plan's stream, each bracketed by HIP events of its own, one
 * synchronisation at the end (the launches queue up as in a caller's loop): total_ms[i] covers the whole apply
 * (output clear + patch kernel), kernel_ms[i] the patch kernel alone.  Either array may be NULL. */
int rpsf_apply_device_timed(rpsf_plan* plan, const void* image_dev, void* out_dev, const rpsf_geometry* geom,
                            int iters, float* total_ms, float* kernel_ms);
/* `iters` applies back to back between ONE pair of HIP events on the plan's stream: the average device time of an apply in
 * a caller's loop (what bench.py's roofline line divides the algorithmic bytes by). */
int rpsf_apply_device_loop_ms(rpsf_plan* plan, const void* image_dev, void* out_dev, const rpsf_geometry* geom, int iters,
                              double* ms_per_apply);
/* A batch of n_frames frames of identical geometry corrected with the plan's (shared) transfer kernel -
 * what a caller of the reference does with a Python loop over ArrayPSFTransform.apply
 * (transform.py:85-177) on a stack of exposures.  The frames of one patch are scheduled next to each other so
 * the packed transfer kernel is read from HBM once per batch, not once per frame.
 * Host variants - the STREAMED path: what a user of the reference runs is `[transform.apply(image) for image in images]`
 * (docs/source/example.ipynb over transform.py:85-177), host arrays in and out, and every frame crosses PCIe twice, which
 * costs several times the kernel.  The frames go through the plan's staging slots in groups, up to four groups in flight on
 * three streams: H2D of group i + 1 || the shared-K launch of group i (rpsf_apply_batch_device's) || D2H of group i - 1, with
 * the dtype conversions of both directions on the persistent worker pool - PCIe in both directions is kept busy and is what
 * bounds the call (bench.py --config 5 --streamed reports it against rpsf_pcie_probe's floor).  Results are bit-identical to
 * the frame-by-frame loop.
 *   rpsf_apply_batch:        (n_frames, height, width) float32 stacks, C-contiguous;
 *   rpsf_apply_batch_host:   the same with float32 or float64 on either side (as rpsf_apply_host);
 *   rpsf_apply_frames_host:  one pointer per frame (a Python list of arrays needs no np.stack). */
int rpsf_apply_batch(rpsf_plan* plan, const float* images_host, int n_frames, int height, int width, int pad_mode,
                     float pad_value, float* outs_host);
int rpsf_apply_batch_host(rpsf_plan* plan, const void* images_host, int image_is_f64, int n_frames, int height, int width,
                          int pad_mode, float pad_value, void* outs_host, int out_is_f64);
int rpsf_apply_frames_host(rpsf_plan* plan, const void* const* images_host, int image_is_f64, int n_frames, int height,
                           int width, int pad_mode, float pad_value, void* const* outs_host, int out_is_f64);
/* Page-locked host memory (hipHostMalloc).  float32 frames kept in it - acquisition buffers, result rings - are read and
 * written by the copy engines directly: the host-array entry points above detect such pointers (hipPointerGetAttributes)
 * and skip the staging copy of the pageable path for every side that needs no dtype conversion. */
int rpsf_host_alloc(int device, size_t bytes, void** out);
int rpsf_host_free(void* ptr);
/* Width of the worker pool the host-array entry points convert on (creates it if this is the first use).  The workers are
 * pinned to cores of the NUMA node the (first) device hangs off, spread over its core complexes (RPSF_HOST_AFFINITY=0: not
 * pinned; RPSF_HOST_THREADS: width). */
int rpsf_host_threads(int* threads);
/* Self-test of that pool (no GPU involved; the CPU test suite runs it): `jobs` jobs of up to `parts` parts from each of `callers`
 * threads at once, every part checked to have run exactly once; *failures = number of jobs that came out wrong. */
int rpsf_host_pool_selftest(int callers, int jobs, int parts, int* failures);
/* That node (-1: unknown): a process that feeds the GPU from host arrays should run and allocate there - staging copies
 * from the other socket run at a third of the rate (scripts/micro/host_copy.hip). */
int rpsf_device_numa_node(int device, int* node);
/* What PCIe gives `bytes` on this box, from and to pinned host memory: one direction at a time and both at once (two
 * streams), best of `iters`, milliseconds.  The floor the streamed entry points are reported against (SURVEY 8d:
 * end-to-end figures are reported separately from the device-resident ones).  Any pointer may be NULL. */
int rpsf_pcie_probe(int device, size_t bytes, int iters, double* h2d_ms, double* d2h_ms, double* duplex_ms);
/* Device variant: frame f is at images_dev + f * image_stride and outs_dev + f * out_stride (strides in
 * floats); asynchronous on `stream` (NULL: the plan's own).  The plan keeps 16 bytes of scratch per output
 * pixel per frame in flight (large batches are cut into groups internally). */
int rpsf_apply_batch_device(rpsf_plan* plan, const void* images_dev, void* outs_dev, int n_frames, size_t image_stride,
                            size_t out_stride, const rpsf_geometry* geom, void* stream);
/* Timed variant, like rpsf_apply_device_timed: total_ms[i] covers the whole batch, kernel_ms[i] its patch kernel. */
int rpsf_apply_batch_device_timed(rpsf_plan* plan, const void* images_dev, void* outs_dev, int n_frames,
                                  size_t image_stride, size_t out_stride, const rpsf_geometry* geom, int iters,
                                  float* total_ms, float* kernel_ms);
/* DEVICE-ARRAY VIEWS: what regularizepsf_amd.DeviceArray - or any object with __cuda_array_interface__ - hands to apply and apply_batch
 * (the reference takes NumPy arrays only, transform.py:85-117; this is the device-resident counterpart of its np.asarray / astype).
 * A view is rows x cols elements of `dtype` in ordinary device memory of the plan's device, element (r, c) at
 * data + r * row_stride + c * col_stride BYTES.  Strides are positive; a pointer or a stride that is no multiple of the item size is
 * served, byte by byte.  An OUTPUT view is float32, float64 or float16.  Bad arguments (null view, null data of a non-empty view, a
 * non-positive stride, rows or cols < 0, an unknown dtype, an output dtype outside the three) return RPSF_E_BADARG and write nothing; an
 * empty view (rows or cols == 0) returns RPSF_OK and does nothing. */
#define RPSF_DTYPE_FLOAT32 0
#define RPSF_DTYPE_FLOAT64 1
#define RPSF_DTYPE_FLOAT16 2
#define RPSF_DTYPE_UINT8 3
#define RPSF_DTYPE_INT16 4
#define RPSF_DTYPE_UINT16 5
#define RPSF_DTYPE_INT32 6
typedef struct rpsf_view {
  void* data;
  int dtype;
  int rows, cols;
  int64_t row_stride, col_stride; /* bytes */
} rpsf_view;
/* What an apply did with its views, a bit set: */
#define RPSF_ROUTE_C1 1        /* the input went through conversion kernel C1 (gather and convert to a dense float32 frame) */
#define RPSF_ROUTE_C2 2        /* the output went through conversion kernel C2 (convert and scatter from a dense float32 frame) */
#define RPSF_ROUTE_SATURATED 4 /* the saturation route ran (rpsf_apply_device_saturated / rpsf_apply_batch_device_saturated) */
#define RPSF_ROUTE_STAGED 8    /* a batch: the frames were gathered into the plan's staging stack */
/* ZERO COPY: a side is taken as it is - no kernel added, no byte copied, the view goes straight into rpsf_apply_device (a stack of such
 * planes with one frame stride that is a multiple of 4 bytes into rpsf_apply_batch_device) - when it is float32 with col_stride == 4, a
 * row_stride that is a positive multiple of 4, at least 4 * cols and at most INT_MAX floats, and a 4-byte aligned pointer: what
 * rpsf_geometry's ld_image / ld_out promise.  Every other side goes through C1 / C2 (csrc/convert.hip) and a dense float32 frame in
 * STAGING owned by the plan: 4 B per pixel (rounded up to 4 pixels per frame) per frame of the call for each side that needs it, allocated
 * at the first such call, grown when a larger call arrives, freed with the plan.  The saturation entry points take dense frames, so on
 * that route a pitched float32 side is staged as well.
 * rpsf_view_route: *route = the RPSF_ROUTE_C1 / _C2 bits a plain (threshold = +inf) single-frame apply of these views sets; pure, no GPU. */
int rpsf_view_route(const rpsf_view* image, const rpsf_view* out, int* route);
/* C1 or C2 alone on `device`, asynchronous on `stream` (NULL: the null stream): dst a dense float32 view (row_stride == 4 * cols) -> C1 from
 * any src; else src a dense float32 view and dst float32 / float64 / float16 -> C2; anything else, or two shapes: RPSF_E_BADARG. */
int rpsf_convert_view(int device, const rpsf_view* src, const rpsf_view* dst, void* stream);
/* ArrayPSFTransform.apply on views (whole-image geometry): threshold == +inf is rpsf_apply_device's correction (pad_value: constant mode),
 * anything else rpsf_apply_device_saturated's route with its preconditions (dilation >= 1, neighborhood_width / 2 >= 1) and its one wait.
 * Integers convert as (float)(double)v, float64 by the C cast, float16 output rounds to nearest even.  image and out have one shape.
 * Everything is enqueued on `stream` (NULL: the plan's own); a call on another stream than the last one that used the staging waits
 * for that one on the device.  *route_or_null receives the RPSF_ROUTE_* bits. */
int rpsf_apply_view(rpsf_plan* plan, const rpsf_view* image, const rpsf_view* out, int pad_mode, float pad_value, double threshold,
                    int dilation, int neighborhood_width, void* stream, int* route_or_null);
/* The same for n_frames frames of one shape, images[f] -> outs[f], with the shared-K batch launch (rpsf_apply_batch_device /
 * rpsf_apply_batch_device_saturated): frame by frame the bits of rpsf_apply_view.  A side whose views are zero copy (saturation: dense),
 * of one row stride and evenly spaced by a positive multiple of 4 bytes is taken as it is; any other side is gathered into / scattered
 * from one staging stack (RPSF_ROUTE_STAGED with RPSF_ROUTE_C1 for the input).  n_frames == 0: RPSF_OK; < 0: RPSF_E_BADARG. */
int rpsf_apply_batch_view(rpsf_plan* plan, const rpsf_view* images, const rpsf_view* outs, int n_frames, int pad_mode, float pad_value,
                          double threshold, int dilation, int neighborhood_width, void* stream, int* route_or_null);
/* BAD-PIXEL MASKS ("Bad-pixel masks"; not in the reference): the device saturation route with, besides the pixels above
 * the threshold, pixels the caller names.  On the 2N-padded frame P: M = the dilated hot mask as above; E = the caller's mask taken
 * through pad_mode's index map (0 in the pad of RPSF_PAD_CONSTANT), or-ed with "P is NaN or +-Inf" when fill_nonfinite != 0; the mask of
 * F3 - F5 is M | E.  E is NOT dilated.  Fill, correction, restore and lists are those of the entry points these stand beside, from which
 * they differ by the mask arguments only; threshold == +inf leaves E alone.  A mask is a uint8 rpsf_view of the frame's shape in device
 * memory, nonzero = masked, any positive strides; n_masks is 0 (with masks_or_null == NULL), 1 (one mask for every frame) or n_frames.
 * A view of another dtype or shape, null data, a stride that is not positive or another n_masks: RPSF_E_BADARG before anything runs.
 * masks_or_null == NULL with fill_nonfinite == 0 IS the call of the unmasked entry point (rpsf_apply_batch_device_saturated,
 * rpsf_apply_view, rpsf_apply_batch_view, rpsf_apply_frames_host_saturated_device): that code runs, nothing else.  Otherwise the route
 * runs whatever the threshold, and a frame with nothing hot and nothing in E still leaves F2 - F4 at their first instruction.
 * SCRATCH, owned by the plan, besides what rpsf_apply_device_saturated lists: per pixel of the padded frame 1 B more (the exact plane E),
 * 24 B per frame (the mask views, device and pinned host) and 4 B per frame (the count of E); rpsf_apply_frames_host_masked_device
 * uploads its host masks into uint8 scratch of 1 B per pixel of the frame-group (of one frame for a shared mask).  All of it is made
 * at the first masked call, reused, grown on demand and freed with the plan. */
int rpsf_apply_batch_device_masked(rpsf_plan* plan, const void* images_dev, void* outs_dev, int n_frames, size_t image_stride,
                                   size_t out_stride, int height, int width, int pad_mode, double threshold, int dilation,
                                   int neighborhood_width, const rpsf_view* masks_or_null, int n_masks, int fill_nonfinite, void* stream,
                                   size_t* n_masked_per_frame_or_null);
/* rpsf_apply_view / rpsf_apply_batch_view with masks; RPSF_ROUTE_SATURATED is set whenever a mask or fill_nonfinite is given */
int rpsf_apply_view_masked(rpsf_plan* plan, const rpsf_view* image, const rpsf_view* out, int pad_mode, float pad_value, double threshold,
                           int dilation, int neighborhood_width, const rpsf_view* mask_or_null, int fill_nonfinite, void* stream,
                           int* route_or_null);
int rpsf_apply_batch_view_masked(rpsf_plan* plan, const rpsf_view* images, const rpsf_view* outs, int n_frames, int pad_mode, float pad_value,
                                 double threshold, int dilation, int neighborhood_width, const rpsf_view* masks_or_null, int n_masks,
                                 int fill_nonfinite, void* stream, int* route_or_null);
/* rpsf_apply_frames_host_saturated_device with HOST masks: masks_host_or_null[f] is a dense height x width uint8 array */
int rpsf_apply_frames_host_masked_device(rpsf_plan* plan, const void* const* images_host, int image_is_f64, int n_frames, int height,
                                         int width, int pad_mode, double threshold, int dilation, int neighborhood_width,
                                         const uint8_t* const* masks_host_or_null, int n_masks, int fill_nonfinite, void* const* outs_host,
                                         int out_is_f64);
/* Test entry in the style of rpsf_saturation_fill_batch_device: F1 - F4 alone with masks.  masks_in_host_or_null: n_masks host masks
 * mask_frame_bytes apart, element (r, c) at r * mask_row_stride + c * mask_col_stride bytes; they are uploaded as they lie and read
 * through those strides.  masks_host receives M | E, masked_per_frame_or_null[f] its pixel count in padded frame f. */
int rpsf_saturation_fill_masked_device(rpsf_plan* plan, const float* images_host, int n_frames, int height, int width, int pad_mode,
                                       double threshold, int dilation, int neighborhood_width, int order, const uint8_t* masks_in_host_or_null,
                                       int n_masks, size_t mask_frame_bytes, int64_t mask_row_stride, int64_t mask_col_stride,
                                       int fill_nonfinite, float* padded_host, uint8_t* masks_host, int* groups_per_frame_or_null,
                                       int* masked_per_frame_or_null);
/* The plan's own stream (hipStream_t), for callers that enqueue follow-up work such as the seam exchange.  The plan cannot know what a caller
 * puts on it: the call joins the plan's two launch lanes (RPSF_OPT_PIPELINE) and the plan keeps to this one stream from then on. */
void* rpsf_plan_stream(rpsf_plan* plan);

/* ArrayPSFTransform.construct arithmetic, transform.py:78-82:
 *   K = conj(S) |S|^(alpha-1) / (|S|^(alpha+1) + (eps |T|)^(alpha+1)) * T
 * element-wise over `count` complex values; S, T, K are host arrays of complex64 (is_f64 = 0,
 * evaluated in float32 like NumPy does for complex64 input) or complex128 (is_f64 = 1). */
int rpsf_build_transfer(int device, size_t count, const void* s_host, const void* t_host, int is_f64, double alpha,
                        double epsilon, void* k_host);
/* Device-resident variant (pointers on `device`), asynchronous on stream. */
int rpsf_build_transfer_device(int device, size_t count, const void* s_dev, const void* t_dev, int is_f64,
                               double alpha, double epsilon, void* k_dev, void* stream);

/* Batched un-shifted 2-D FFT of real PSF cubes (ArrayPSF.__init__, psf.py:216-219), float32 in,
 * complex64 out, (count, N, N) host arrays. */
int rpsf_psf_fft(int device, int patch_size, int count, const float* values_host, float* fft_c64_host);
/* Same, leaving the spectra on the device (count * N * N complex64 at fft_c64_dev, allocated by the caller): the input
 * of rpsf_build_transfer_device, so that ArrayPSF -> construct (psf.py:216-219 -> transform.py:78-82) -> apply never
 * moves a spectrum or K over PCIe. */
int rpsf_psf_fft_device(int device, int patch_size, int count, const float* values_host, void* fft_c64_dev);
/* Built-in parametric PSF models rasterised on the device (kernel K6) and transformed there: replaces the host loop of
 * VariedFunctionalPSF.as_array_psf (regularizepsf/psf.py:159-165: one Python call of the model per patch on an N x N
 * meshgrid) followed by ArrayPSF.__init__ (psf.py:216-219) for models the library knows, so that model parameters ->
 * samples -> spectra -> K -> apply never leaves the GPU.  params_host: count x RPSF_MODEL_PARAMS doubles, per model
 *   RPSF_MODEL_ELLIPTICAL_GAUSSIAN: amplitude, row0, col0, sigma_row, sigma_col, theta, background, unused
 *   RPSF_MODEL_MOFFAT:              amplitude, row0, col0, alpha, beta, unused, background, unused
 * Element [i][j] of a patch is the model at (row = j, col = i), as the reference's meshgrid hands it over.  normalize != 0
 * scales every patch to unit sum.  values_f32_dev (optional, count * N * N floats) keeps the samples, fft_c64_dev
 * (count * N * N complex64) receives the spectra; both allocated by the caller on `device`. */
#define RPSF_MODEL_PARAMS 8
#define RPSF_MODEL_ELLIPTICAL_GAUSSIAN 0
#define RPSF_MODEL_MOFFAT 1
int rpsf_psf_model_fft_device(int device, int model, int patch_size, int count, const double* params_host, int normalize,
                              void* values_f32_dev, void* fft_c64_dev);

/* ArrayPSFBuilder.build downstream of the star list (regularizepsf/builder.py:139-265): a builder owns a device stack of float32
 * N x N star patches (background-subtracted, not normalised), filled frame by frame and then averaged per lattice cell.  Star finding
 * (sep, image_processing.py:65-74) and the cell membership (builder.py:45-51) stay with the caller; the final per-cell clean-up
 * (builder.py:231-260) is the caller's after rpsf_builder_average and the device's with rpsf_builder_model.  N from 4 to 128, odd sizes included (anything else: RPSF_E_UNSUPPORTED; 129 to 256: rpsf_builder_create_wide below); `capacity` patches are allocated at once, the
 * stack grows by itself beyond that.  INVARIANT: every patch of the stack is finite and has a non-zero centre pixel [N/2][N/2]. */
typedef struct rpsf_builder rpsf_builder;
int rpsf_builder_create(rpsf_builder** out, int device, int patch_size, size_t capacity);
void rpsf_builder_destroy(rpsf_builder* builder);
/* The per-star loop of _find_patches (image_processing.py:95-121) for one frame, kernel B1: the frame is uploaded once as float32; star i
 * has the rounded corner corners_i32[i] = (row, col) (:96) and the shift amounts frac_f64[i] (:101), both computed by the caller with the
 * reference's expressions.  Per star: the patch through np.pad's reflect map (:82-100), scipy.ndimage.shift(order 3, mode 'mirror') (:102),
 * the background plane of calculate_background (:13-46) subtracted (:110-112), the tests of :117-119.  accepted_u8_host[i] receives
 * 1: accepted and appended to the stack (in star order), 0: rejected (a pixel not below saturation_threshold, the centre not strictly
 * inside (star_minimum, star_maximum), a zero or non-finite pixel), 2: fewer than three usable border pixels (or all on one line) for the
 * plane - nothing the reference defines; the caller decides. */
int rpsf_builder_add_frame(rpsf_builder* builder, const void* image_host, int image_is_f64, int height, int width, int n_stars,
                           const int32_t* corners_i32, const double* frac_f64, double saturation_threshold, double star_minimum,
                           double star_maximum, uint8_t* accepted_u8_host);
int rpsf_builder_count(const rpsf_builder* builder, size_t* count);
/* Patches first .. first + count of the stack, count x N x N float32. */
int rpsf_builder_patches(rpsf_builder* builder, size_t first, size_t count, float* host);
/* Append patches the caller already has (count x N x N float32); RPSF_E_BADARG for a non-finite pixel or a zero centre. */
int rpsf_builder_load_patches(rpsf_builder* builder, size_t count, const float* host);
/* _average_patches (builder.py:53-125), kernel B2: cell c averages the patches members_i32[cell_offsets_i64[c] .. cell_offsets_i64[c + 1])
 * (indices into the stack, in the order the reference meets them), every sample being (double)pixel / (double)centre of its patch
 * (:61,:87).  Mean: the additions of :66 in list order, divided by the count.  Median / percentile (0..100): exact selection, NumPy's
 * rules (mean of the two middle samples; the default linear method).  A cell without members is all zeros (:119-123).
 * cells_f64_host: n_cells x N x N float64. */
#define RPSF_AVERAGE_MEAN 0
#define RPSF_AVERAGE_MEDIAN 1
#define RPSF_AVERAGE_PERCENTILE 2
int rpsf_builder_average(rpsf_builder* builder, int method, double percentile, int n_cells, const int64_t* cell_offsets_i64,
                         const int32_t* members_i32, double* cells_f64_host);
/* Device time of the last B1 and the last B2 launch, milliseconds (either pointer may be NULL). */
int rpsf_builder_kernel_ms(const rpsf_builder* builder, double* patch_ms, double* average_ms);
/* The per-cell clean-up of builder.py:238-258, kernel B3, on n_cells (> 0) cells of N x N float64 the caller supplies (every pixel
 * finite, else RPSF_E_BADARG): background plane fitted to the ring around the non-zero interior and subtracted, everything inside the
 * region below 0.5 % of the centre dropped, the 4-connected component of the centre kept and dilated by one pixel, unit sum
 * (DESIGN.md 3.6 has the definition step by step).  out_f64_host: n_cells x N x N float64; flags_u8_host[c] receives
 * 0: cleaned (an all-zero cell leaves all NaN, as from the reference), 1: the cell is not zero and its ring has fewer than three pixels or
 * all on one line - out holds the cell as it came, and the caller decides (the reference takes SciPy's minimum-norm fit there). */
int rpsf_builder_clean(rpsf_builder* builder, int n_cells, const double* cells_f64_host, double* out_f64_host, uint8_t* flags_u8_host);
/* rpsf_builder_average followed by rpsf_builder_clean with the averaged cells staying on the device: one download, of the cleaned cells
 * and the flags.  out_f64_host of a cell with flag 1 holds the AVERAGED cell. */
int rpsf_builder_model(rpsf_builder* builder, int method, double percentile, int n_cells, const int64_t* cell_offsets_i64,
                       const int32_t* members_i32, double* out_f64_host, uint8_t* flags_u8_host);
/* Device time of the last B3 launch, milliseconds. */
int rpsf_builder_clean_ms(const rpsf_builder* builder, double* ms);

/* interpolation_scale = s of the reference builder.  _scale_image (image_processing.py:49-59), kernels U1 / U2: the
 * height x width frame (float32 or float64, not narrowed before the solve; both at least 4, else RPSF_E_BADARG - the cubic spline needs
 * four points) resampled with the not-a-knot interpolating cubic spline - RectBivariateSpline's defaults on integer knots - one pass per
 * axis, float64 throughout, onto (1 + (height - 1) s) x (1 + (width - 1) s) samples; sample [i s][j s] is pixel [i][j] itself.
 * scale >= 1, scale == 1 copies.  out_f64_host: the scaled frame, float64.  Two runs of one input agree bit for bit. */
int rpsf_scale_image(int device, const void* image_host, int image_is_f64, int height, int width, int scale, double* out_f64_host);
/* Device time of the calling thread's last upscale, milliseconds (either pointer may be NULL, not both): U1, the axis-0 pass, and U2, the
 * axis-1 pass with its two transposes. */
int rpsf_scale_kernel_ms(double* u1_ms, double* u2_ms);
/* A builder for interpolation_scale = scale: its stack holds P x P patches, P = patch_size * scale (B1 and B2 run at P), its cells and
 * its model are patch_size x patch_size (B3 runs at patch_size).  patch_size or P outside 4..128: RPSF_E_UNSUPPORTED; scale < 1:
 * RPSF_E_BADARG; scale == 1 is rpsf_builder_create.  On such a builder rpsf_builder_patches and rpsf_builder_load_patches move P x P
 * patches, rpsf_builder_average delivers patch_size x patch_size cells (B2, then the block mean B4), rpsf_builder_model the same cells
 * cleaned (B2, B4, B3), and rpsf_builder_clean takes patch_size x patch_size cells. */
int rpsf_builder_create_scaled(rpsf_builder** out, int device, int patch_size, int scale, size_t capacity);
/* rpsf_builder_add_frame for the UNSCALED frame of a scaled builder (`scale` must be the builder's): the frame is uploaded as it is,
 * upscaled on the device as by rpsf_scale_image, rounded to float32 once into the buffer B1 reads, and B1 runs with the scaled height
 * and width - no scaled frame crosses PCIe.  corners_i32 and frac_f64 are in scaled-frame pixels, computed with P. */
int rpsf_builder_add_frame_scaled(rpsf_builder* builder, const void* image_host, int image_is_f64, int height, int width, int scale,
                                  int n_stars, const int32_t* corners_i32, const double* frac_f64, double saturation_threshold,
                                  double star_minimum, double star_maximum, uint8_t* accepted_u8_host);
/* downscale_local_mean (builder.py:234-235), kernel B4 alone: n_cells (> 0) cells of P x P float64 the caller supplies -> cells of
 * patch_size x patch_size, each pixel the sum of its scale x scale block in row-major order, in float64, divided by scale * scale. */
int rpsf_builder_downscale(rpsf_builder* builder, int n_cells, const double* cells_f64_host, double* out_f64_host);

/* The wide sizes, 129 <= patch_size <= 256 ("Wide sizes"): a builder whose patches and cells do not fit LDS as float64.
 * null `out`: RPSF_E_BADARG; a patch_size outside 129..256: RPSF_E_UNSUPPORTED with the size in rpsf_last_error() - both before any HIP
 * call.  rpsf_builder_create and rpsf_builder_create_scaled keep refusing these sizes.  The handle is an ordinary rpsf_builder: _add_frame,
 * _add_frame_device, _load_patches, _patches, _count, _average, _clean, _model, _kernel_ms, _clean_ms and _destroy take it unchanged and
 * give what they give at the other sizes (kernels B1w and B3w in the place of B1 and B3; B2 serves every size);
 * rpsf_builder_add_frame_scaled and rpsf_builder_downscale refuse it (RPSF_E_UNSUPPORTED).  B1w and B3w work through a fixed number of
 * slots of a workspace in device memory (at most 256 MiB: 256 slots, 255 at N = 256) that belongs to the handle: it is allocated by the first call
 * that launches either kernel and freed by rpsf_builder_destroy. */
int rpsf_builder_create_wide(rpsf_builder** out, int device, int patch_size, size_t capacity);
/* The number of workspace slots of a wide builder: a launch of B1w or B3w is min(items, slots) workgroups, workgroup b takes items
 * b, b + slots, ...  RPSF_E_UNSUPPORTED for a handle that is not wide. */
int rpsf_builder_wide_slots(const rpsf_builder* builder, int* slots);

/* find_stars: star positions for the builder, upstream of the star list.  The detector is this library's own, modelled on
 * sep.Background + sep.extract; it is not sep and its positions differ from sep's for blended or extended sources.  Deblending is an
 * option (rpsf_stars_set_deblend, off by default): one watershed level on the filtered residual with a significance test per basin - not
 * sep's multi-threshold tree.  Without it touching stars come out as one detection at their common centroid.
 * A finder is made for one frame shape and one background box (8 .. 128 pixels, anything else: RPSF_E_UNSUPPORTED; frames of up to
 * 2^31 - 1 pixels).  A pixel is usable when it is finite and not masked.  Everything is float64 on a frame rounded to float32 once;
 * two runs on one input agree bit for bit. */
typedef struct rpsf_stars rpsf_stars;
int rpsf_stars_create(rpsf_stars** out, int device, int height, int width, int box);
void rpsf_stars_destroy(rpsf_stars* finder);
/* Kernel S1: upload the frame (float32, or float64 narrowed once) and the mask (height x width bytes, non-zero = ignore; NULL: none) and
 * return the RAW background mesh, ceil(height / box) x ceil(width / box) float64 each: per box up to 16 rounds of clipping at
 * |v - median| <= 3 sd (exact median, NumPy's rule), then level = median if sd == 0 or |mean - median| >= 0.3 sd, else
 * 2.5 median - 1.5 mean, and rms = sd.  A box without a usable pixel gives NaN in both.  Filling and filtering the mesh is the caller's. */
int rpsf_stars_background(rpsf_stars* finder, const void* image_host, int image_is_f64, const uint8_t* mask_host_or_null,
                          double* level_host, double* rms_host);
/* Kernels S2 - S4 on the frame uploaded last: level_host is the caller's filled and filtered mesh (finite everywhere), threshold_abs the
 * absolute threshold T.  Residual d = pixel - bilinear surface through the mesh on usable pixels, 0 elsewhere; f = d filtered with
 * [[1,2,1],[2,4,2],[1,2,1]] / 16 (zeros outside the frame); detected: f > T on a usable pixel; 8-connected components; kept:
 * min_area <= area <= max_area (max_area < 0: no upper limit) and sum d > 0.  *count receives the number kept.
 * RPSF_E_STATE before the first rpsf_stars_background. */
int rpsf_stars_detect(rpsf_stars* finder, const double* level_host, double threshold_abs, long min_area, long max_area, size_t* count);
/* Detections first .. first + count of the last detect, in raster order of each component's first pixel: count x 4 float64
 * (row, col, flux, area) with (row, col) = (sum d row, sum d col) / sum d over the component's pixels, d unfiltered. */
int rpsf_stars_positions(rpsf_stars* finder, size_t first, size_t count, double* out);
/* Kernel S3 alone on a mask of the finder's shape (non-zero = detected): labels_host (int32) receives for every detected pixel the
 * smallest linear index row * width + col of its 8-connected component and -1 elsewhere. */
int rpsf_stars_label(rpsf_stars* finder, const uint8_t* detected_host, int32_t* labels_host);
/* The tile S2 and S3 work on (either pointer may be NULL). */
int rpsf_stars_info(const rpsf_stars* finder, int* tile_rows, int* tile_cols);
/* Device time of the last S1, S2, S3 and S4 launches, milliseconds. */
int rpsf_stars_kernel_ms(const rpsf_stars* finder, double ms[4]);

/* THE FUSED ROUTE: a frame is uploaded at most once, the stars are found and the builder's patches cut from that one
 * float32 frame on the device, and the background mesh never leaves the device.  The results are bit for bit those of
 * rpsf_stars_background, the host filter of the mesh (regularizepsf_amd.stars.filter_mesh), rpsf_stars_detect and rpsf_builder_add_frame.
 *
 * Kernel S1b, after S1 and on the device: valid = both raw meshes finite at the node; the invalid nodes take the median of the valid ones
 * (NumPy's rule), a 3 x 3 median with the indices clamped at the edges runs over both filled meshes, global_rms is the median of the
 * filtered rms.  No valid node at all sets a flag on the device and the frame has no stars.
 *
 * rpsf_stars_background_view: `image` is a device view of the finder's shape on the finder's device (any dtype and strides of rpsf_view;
 * a dense float32 view is copied device to device, anything else converted by kernel C1) and is only read; the mask is a host array as
 * for rpsf_stars_background.  Then S1 and S1b; nothing is downloaded.  _host: the same after the one upload of a host frame (float32, or
 * float64 narrowed once).  _scaled: the UNSCALED height x width host frame is uploaded in its own type, upscaled on the device as by
 * rpsf_scale_image and rounded to float32 once into the frame buffer of a finder made for the scaled shape
 * (1 + (height - 1) scale) x (1 + (width - 1) scale) (anything else: RPSF_E_BADARG; scale >= 2); the mask has the scaled shape. */
int rpsf_stars_background_view(rpsf_stars* finder, const rpsf_view* image, const uint8_t* mask_host_or_null);
int rpsf_stars_background_host(rpsf_stars* finder, const void* image_host, int image_is_f64, const uint8_t* mask_host_or_null);
int rpsf_stars_background_scaled(rpsf_stars* finder, const void* image_host, int image_is_f64, int height, int width, int scale,
                                 const uint8_t* mask_host_or_null);
/* Kernel S1b alone on raw meshes of the finder's mesh shape that the caller supplies (NaN and infinities mark invalid nodes):
 * *none = 1 when no node is valid - then *T = +inf and nothing else is written; else the filtered meshes, *global_rms and
 * *T = threshold * global_rms, the multiply done on the device. */
int rpsf_stars_filter_mesh(rpsf_stars* finder, const double* level_host, const double* rms_host, double threshold, double* level_out,
                           double* rms_out, double* global_rms, double* T, int* none);
/* Kernels S2 - S4 of rpsf_stars_detect on the frame and the filtered mesh a rpsf_stars_background_view / _host / _scaled left on the device,
 * with T = threshold * global_rms computed and read there; *count = 0 when no box had a usable pixel.  RPSF_E_STATE before such a call.
 * rpsf_stars_positions delivers the detections as after rpsf_stars_detect. */
int rpsf_stars_detect_device(rpsf_stars* finder, double threshold, long min_area, long max_area, size_t* count);
/* The finder's frame on its device: height x width dense float32, valid until the next frame is given to the finder or it is destroyed
 * (height and width may be NULL).  RPSF_E_STATE before a frame was uploaded. */
int rpsf_stars_frame(rpsf_stars* finder, const float** frame_dev, int* height, int* width);
/* Device time of the last S1b, milliseconds. */
int rpsf_stars_mesh_ms(const rpsf_stars* finder, double* ms);

/* THE DEBLEND OPTION.  rpsf_stars_set_deblend configures the finder: with on != 0 every following
 * rpsf_stars_detect / rpsf_stars_detect_device splits blended components, with on == 0 (the state of a new finder) nothing of it runs and
 * every result is bit for bit what it was.  contrast outside [0, 1], prominence < 0 or a non-finite value: RPSF_E_BADARG.
 *   D1  on detected pixels p is above q when f(p) > f(q), or f(p) == f(q) and index(p) < index(q) (index = row * width + col); up(p) is
 *       the highest of p and its detected 8-neighbours, peak(p) the fixed point of following up; equal peaks form a basin.
 *   D2  per basin: area, sum of d (fixed order), saddle = max of min(f(p), f(q)) over 8-adjacent pairs with q in another basin.
 *   D3  a basin is significant when area >= min_area, flux >= contrast * F (F: the component's sum of d as S4 computes it) and
 *       f(peak) - saddle >= prominence * T.
 *   D4  a component with at most one significant basin is one object, its row bit for bit the undeblended one; otherwise one object
 *       per significant basin, every pixel of an insignificant basin joining the significant peak of its component at the smallest
 *       (drow)^2 + (dcol)^2, ties to the smaller index.  Rows as for components, kept by the same area and flux rule, in raster order
 *       of each object's first pixel. */
int rpsf_stars_set_deblend(rpsf_stars* finder, int on, double contrast, double prominence);
/* D1 alone on the caller's f (float64) and mask (non-zero = detected) of the finder's shape: peak_host (int32) receives for every
 * detected pixel the linear index of its basin's peak and -1 elsewhere.  The counterpart of rpsf_stars_label.  f is expected to be free of
 * NaN on detected pixels (a NaN compares with nothing, so D1's order is not total there; the walks end all the same, because every step
 * needs f to rise or the index to fall). */
int rpsf_stars_basins(rpsf_stars* finder, const double* f_host, const uint8_t* detected_host, int32_t* peak_host);
/* Of the last detect: the number of components, of basins and of components that were split (any pointer may be NULL); basins and
 * split_components are 0 when the option was off. */
int rpsf_stars_deblend_info(const rpsf_stars* finder, size_t* components, size_t* basins, size_t* split_components);
/* Device time of the last D1 - D4 (or of the last rpsf_stars_basins), milliseconds; 0 when the option was off. */
int rpsf_stars_deblend_ms(const rpsf_stars* finder, double* ms);

/* SHAPES (kernel S5): second moments and the peak of every row of the last detect.  Never called, nothing of it runs and
 * no launch, allocation or download of the finder differs.  For a row (row, col, flux, area) with P the pixels of its component (or, with
 * the deblend option, of its object), d the residual of rpsf_stars_detect, dr = r - row and dc = c - col:
 *   rr = sum_P d (dr dr) / flux, cc = sum_P d (dc dc) / flux, rc = sum_P d (dr dc) / flux, abs_flux = sum_P |d|, peak = max_P d at
 *   (peak_row, peak_col), the first pixel in raster order that attains it, and the bounding box of P;
 * float64, in S4's summation order (lane-strided raster order over the bounding box, 8 groups of 8).  This is not sep: no 1 / 12 pixel
 * term, no clamp of a singular matrix, and the footprint is this detector's.  A row is RPSF_STARS_SHAPE_COLUMNS float64:
 *   row, col, flux, area (the bits of rpsf_stars_positions), peak, peak_row, peak_col, row_min, row_max, col_min, col_max, abs_flux,
 *   rr, cc, rc. */
#define RPSF_STARS_SHAPE_COLUMNS 15
/* Kernel S5 on the rows of the last rpsf_stars_detect / rpsf_stars_detect_device; *count receives their number (0: nothing is launched).
 * RPSF_E_BADARG when there is no such detect, or when a call since has replaced the finder's frame, a mesh or its labels
 * (rpsf_stars_background*, rpsf_stars_filter_mesh, rpsf_stars_label, rpsf_stars_basins). */
int rpsf_stars_measure(rpsf_stars* finder, size_t* count);
/* Rows first .. first + count of the last rpsf_stars_measure, in the order of rpsf_stars_positions: count x RPSF_STARS_SHAPE_COLUMNS
 * float64.  A range outside them: RPSF_E_BADARG.  A new detect empties them. */
int rpsf_stars_shapes(rpsf_stars* finder, size_t first, size_t count, double* out);
/* Device time of the last S5, milliseconds. */
int rpsf_stars_shape_ms(const rpsf_stars* finder, double* ms);

/* APERTURES (kernel S6): forced aperture photometry at n positions (y, x) the caller supplies (finite, |y|, |x| < 2^20;
 * they may lie off the frame), on the frame, the mask and the filtered mesh a rpsf_stars_background_view / _host / _scaled left on the
 * device (RPSF_E_STATE before such a call).  m radii (1 .. 8, strictly ascending, 0 < R <= 64) and subpix = s (1 .. 8), anything else
 * or a non-finite position: RPSF_E_BADARG.  d is the residual of rpsf_stars_detect_device (use_mesh != 0) or the pixel itself on usable
 * pixels (use_mesh == 0: a frame that is already background-subtracted).  For the pixel (r, c) of the box floor(y - R_max) - 1 ..
 * ceil(y + R_max) + 1 (likewise in x; not clipped to the frame): pr = r - y, pc = c - x, o_a = (2a + 1 - s) / (2s),
 * q_ab = (pr + o_a)(pr + o_a) + (pc + o_b)(pc + o_b), n_k = #{(a, b): q_ab <= R_k R_k}, w_k = n_k / (s s).  Per radius
 * flux_k = sum w_k d and N_use_k = sum n_k over the usable pixels of the frame, N_all_k = sum n_k over the whole box; on the outermost
 * radius, with t = w d: abs = sum w |d|, mr = sum t pr, mc = sum t pc, mrr = sum t (pr pr), mcc = sum t (pc pc), mrc = sum t (pr pc),
 * and peak = max d where n > 0 at (peak_row, peak_col), the first such pixel in raster order (NaN at (-1, -1) when there is none).
 * float64, in S4's summation order; two runs agree bit for bit.  With use_mesh != 0 and no valid mesh node every flux, sum and the peak
 * is NaN and the counts are delivered.  This is not sep's sum_circle / flux_radius: the comparison is <=, there is no error column and no
 * 1 / 12 term, and masked pixels are left out and reported through the counts, not corrected for.  A row of out_host is
 * RPSF_STARS_PHOTOMETRY_COLUMNS(m) float64:
 *   row, col, flux[m], N_use[m], N_all[m], abs, mr, mc, mrr, mcc, mrc, peak, peak_row, peak_col.
 * n == 0 launches nothing.  The call replaces nothing of the finder: a rpsf_stars_positions or rpsf_stars_measure after it gives the
 * bits it gave before. */
#define RPSF_STARS_PHOTOMETRY_COLUMNS(m) (2 + 3 * (m) + 9)
int rpsf_stars_photometry(rpsf_stars* finder, size_t n, const double* positions_host, int m, const double* radii, int subpix,
                          int use_mesh, double* out_host);
/* Device time of the last S6, milliseconds; 0 when it launched nothing. */
int rpsf_stars_photometry_ms(const rpsf_stars* finder, double* ms);

/* WINDOWED POSITIONS (kernel S7): the Gaussian-windowed position and moments at n positions (y, x) the caller supplies
 * (finite, |y|, |x| < 2^20; they may lie off the frame), on the frame, the mask and the filtered mesh a rpsf_stars_background_view /
 * _host / _scaled left on the device (RPSF_E_STATE before such a call).  sigma_host holds one window sigma per position, 0.5 <= sigma
 * <= 16; max_iter lies in 0 .. 64, eps > 0 and finite, 0 < max_shift <= 64; anything else is RPSF_E_BADARG, before anything is launched.
 * d is the residual of rpsf_stars_detect_device (use_mesh != 0) or the pixel itself on usable pixels (finite, not masked).  A WALK at
 * p = (y, x): R = 4 sigma, h = 1 / (2 sigma sigma); over the pixels (r, c) with q = (r - y)^2 + (c - x)^2 <= R R (N_all of them, N_use
 * usable and on the frame), w = g(q h) with g this library's own exp(-t) in plain float64 arithmetic, t = w d:
 *   S = sum t, A = sum w |d|, mr = sum t (r - y), mc = sum t (c - x), mrr = sum t (r - y)^2, mcc = sum t (c - x)^2, mrc = sum t (r - y)(c - x)
 * in float64, in S4's summation order.  From p_0 = the input, j = 0: (1) walk at p_j; (2) S not finite or S <= 0: stop, NO_FLUX; (3) dy =
 * mr / S, dx = mc / S, p' = p_j + 2 (dy, dx); (4) p' not finite or farther than max_shift from p_0: stop, RAN_AWAY; (5) p_(j+1) = p',
 * niter = j + 1, dy dy + dx dx < eps eps: stop, converged; (6) niter == max_iter: stop, NOT_CONVERGED; else j += 1 and (1).  max_iter = 0
 * iterates nothing and sets no flag.  The sums and counts delivered are those of one more walk at the position returned (after a stop at
 * 2 or 4: p_j and the walk just made).  With use_mesh != 0 and no valid mesh node nothing iterates: NO_FLUX, every sum NaN, the counts
 * delivered.  Two runs agree bit for bit.  This is not sep's winpos: no sub-pixel sampling of the window's rim, the comparison is <=,
 * there is no error column, and masked pixels are left out and reported through the counts, not corrected for.  A row of out_host is
 * RPSF_STARS_REFINE_COLUMNS float64:
 *   y0, x0, y, x, sigma, niter, flags, dy, dx (the last step taken or rejected, NaN if none), N_use, N_all, S, A, mr, mc, mrr, mcc, mrc.
 * n == 0 launches nothing.  The call replaces nothing of the finder: a rpsf_stars_positions, rpsf_stars_measure or rpsf_stars_photometry
 * after it gives the bits it gave before. */
#define RPSF_STARS_REFINE_COLUMNS 18
#define RPSF_STARS_REFINE_NO_FLUX 1
#define RPSF_STARS_REFINE_RAN_AWAY 2
#define RPSF_STARS_REFINE_NOT_CONVERGED 4
int rpsf_stars_refine(rpsf_stars* finder, size_t n, const double* positions_host, const double* sigma_host, int max_iter, double eps,
                      double max_shift, int use_mesh, double* out_host);
/* Device time of the last S7, milliseconds; 0 when it launched nothing. */
int rpsf_stars_refine_ms(const rpsf_stars* finder, double* ms);

/* MODEL FITS (kernel S8): the linear least-squares fit of a cell of a PSF model to each of n stars, and its residual.
 * A rpsf_stars_model is a cube of n_cells x N x N float64 values (4 <= N <= 256, 1 <= n_cells <= 2^24; anything else is RPSF_E_BADARG)
 * uploaded to `device` once and used by any number of rpsf_stars_fit calls.  The values are taken as they are: a cell of NaN, which
 * ArrayPSFBuilder leaves where it had no star, makes Smm NaN and the fit DEGENERATE.
 * rpsf_stars_fit: n positions (y, x) the caller supplies (finite, |y|, |x| < 2^20; they may lie off the frame) with one cell index each,
 * on the frame, the mask and the filtered mesh a rpsf_stars_background_view / _host / _scaled left on the device (RPSF_E_STATE before
 * such a call).  0 < radius = R <= min(64, N / 2 - 1), fit_background is 0 or 1, the model lies on the finder's device; anything else is
 * RPSF_E_BADARG, before anything is launched.  d is the residual of rpsf_stars_detect_device (use_mesh != 0) or the pixel itself, on usable
 * pixels (finite, not masked, on the frame).  The cell C holds the star as ArrayPSFBuilder cuts it: its centre at index h = N / 2.0 - 0.5
 * on both axes.  THE MODEL at pixel (r, c):  u = (r - y) + h, v = (c - x) + h, i = floor(u), j = floor(v), a = u - i, b = v - j,
 *   m = ((1 - a) * ((1 - b) * C[i, j] + b * C[i, j + 1])) + (a * ((1 - b) * C[i + 1, j] + b * C[i + 1, j + 1]))
 * in exactly this order of float64 operations, nothing fused.  PASS 1 over the pixels with (r - y)^2 + (c - x)^2 <= R R: n_all and Sm_all =
 * sum m over all of them, and over the usable ones n, Sm = sum m, Smm = sum m m, Sd = sum d, Sdm = sum d m, Sdd = sum d d, in S4's
 * summation order (lane-strided raster order over the box floor(y - R) - 1 .. ceil(y + R) + 1, 8 groups of 8).  THE SOLVE: with
 * fit_background D = n Smm - Sm Sm, f = (n Sdm - Sm Sd) / D, bg = (Sd - f Sm) / n; without, D = Smm, f = Sdm / Smm, bg = 0.  FLAGS:
 *   NO_MESH     use_mesh != 0 and no valid mesh node: every sum NaN, the counts delivered;
 *   BAD_CELL    the cell index is outside 0 .. n_cells - 1: nothing is read from the cube, every sum NaN, the counts delivered;
 *   TOO_FEW     n < 3 with fit_background, n < 1 without;   DEGENERATE (when not TOO_FEW)   D not finite or D <= 0;
 * with any flag f, bg and PASS 2's columns are NaN and the peak sits at (-1, -1).  PASS 2 over the same pixels in the same order, with
 * e = d - (f m + bg): chi2 = sum e e, abs_res = sum |e|, peak_res = max |e| with the signed e there (peak_e) at (peak_row, peak_col), the
 * first such pixel in raster order (a NaN e counts as the largest).  Two runs agree bit for bit.  This is not a PSF-photometry package's
 * fit: the weights are uniform (no error column, no variance weighting), the position is given and not fitted (rpsf_stars_refine supplies
 * positions), the interpolation is bilinear and does not conserve flux below the pixel scale, and masked pixels are left out and reported
 * through the counts, not corrected for.  A row of out_host is RPSF_STARS_FIT_COLUMNS float64:
 *   y, x, cell, flags, n, n_all, Sm, Sm_all, Smm, Sd, Sdm, Sdd, f, bg, chi2, abs_res, peak_res, peak_e, peak_row, peak_col.
 * n == 0 launches nothing and needs no pointers.  The call replaces nothing of the finder: a rpsf_stars_positions, rpsf_stars_measure,
 * rpsf_stars_photometry or rpsf_stars_refine after it gives the bits it gave before. */
#define RPSF_STARS_FIT_COLUMNS 20
#define RPSF_STARS_FIT_NO_MESH 1
#define RPSF_STARS_FIT_TOO_FEW 2
#define RPSF_STARS_FIT_DEGENERATE 4
#define RPSF_STARS_FIT_BAD_CELL 8
typedef struct rpsf_stars_model rpsf_stars_model;
int rpsf_stars_model_create(int device, size_t n_cells, int N, const double* values_host, rpsf_stars_model** out);
void rpsf_stars_model_destroy(rpsf_stars_model* model);
int rpsf_stars_fit(rpsf_stars* finder, const rpsf_stars_model* model, size_t n, const double* positions_host, const int32_t* cells_host,
                   double radius, int fit_background, int use_mesh, double* out_host);
/* Device time of the last S8, milliseconds; 0 when it launched nothing. */
int rpsf_stars_fit_ms(const rpsf_stars* finder, double* ms);

/* FITTED POSITIONS (kernel S9): the position of each of n stars fitted with its cell of a rpsf_stars_model, by a
 * Gauss-Newton iteration around S8's linear fit, and S8's own row at the position it ends at.  The inputs are rpsf_stars_fit's (the
 * positions, one int32 cell index per star that stays fixed for the whole iteration, 0 < radius = R <= min(64, N / 2 - 1), fit_background
 * 0 or 1, the model on the finder's device, RPSF_E_STATE before a rpsf_stars_background_view / _host / _scaled), and max_iter in 0 .. 64,
 * eps > 0 and finite, 0 < max_shift <= 64, 0 < max_step <= 64; anything else is RPSF_E_BADARG, before anything is launched.
 * THE MODEL AND ITS GRADIENT at pixel offset (pr, pc) = (r - y, c - x): u, v, i, j, a, b and m are exactly S8's, and
 *   g_u = ((1 - b) * (C[i + 1, j] - C[i, j])) + (b * (C[i + 1, j + 1] - C[i, j + 1]))
 *   g_v = ((1 - a) * (C[i, j + 1] - C[i, j])) + (a * (C[i + 1, j + 1] - C[i + 1, j]))
 * the exact derivatives of the bilinear interpolant inside its cell, in exactly this order of float64 operations, nothing fused.
 * A WALK at p = (y, x) covers S8's box with S8's disc test q <= R R, S8's usable-pixel rule and S8's d, in S4's summation order
 * (lane-strided raster order, 64 partials folded as 8 groups of 8).  Over the usable pixels it takes n and the thirteen sums of the
 * linearised problem d ~ f m + bg + a_u g_u + a_v g_v:
 *   Smm = sum m m, Sm = sum m, Smu = sum m g_u, Smv = sum m g_v, Su = sum g_u, Sv = sum g_v, Suu = sum g_u g_u, Suv = sum g_u g_v,
 *   Svv = sum g_v g_v, and the right-hand sides Sdm = sum d m, Sd = sum d, Sdu = sum d g_u, Sdv = sum d g_v.
 * THE SOLVE, in the wave's first lane: the symmetric system in the unknowns (f, bg, a_u, a_v)
 *   (Smm Sm Smu Smv) (f  )   (Sdm)
 *   (Sm  n  Su  Sv ) (bg ) = (Sd )         K = 4; without fit_background the row and the column of the constant drop out, K = 3
 *   (Smu Su Suu Suv) (a_u)   (Sdu)
 *   (Smv Sv Suv Svv) (a_v)   (Sdv)
 * by an LDL^T elimination on the upper triangle without pivoting and without square roots: for j = 0 .. K - 1: the pivot A[j][j] must be
 * finite and > 0; for i = j + 1 .. K - 1: l = A[j][i] / A[j][j], for c = i .. K - 1: A[i][c] = A[i][c] - l A[j][c], b[i] = b[i] - l b[j];
 * then back, for j = K - 1 .. 0: s = b[j], for c = j + 1 .. K - 1: s = s - A[j][c] x[c], x[j] = s / A[j][j].  The step is dy = -a_u / f,
 * dx = -a_v / f.  From p_0 = the input, j = 0:
 *   SKIPPED (8)        the star has S8's NO_MESH or BAD_CELL: nothing iterates;
 *   (1) walk at p_j and solve;  SINGULAR (4): n < K, a pivot not finite or <= 0, or dy or dx not finite: stop at p_j, the last step stays
 *       what it was;
 *   (2) each of dy, dx is clamped to [-max_step, max_step] and is now the last step; p' = p_j + (dy, dx);
 *   (3) RAN_AWAY (1): (p' - p_0)^2 > max_shift^2: stop at p_j;
 *   (4) p_(j+1) = p', niter = j + 1; dy dy + dx dx < eps eps: stop, converged;
 *   (5) NOT_CONVERGED (2): niter == max_iter: stop; else j += 1 and (1).
 * max_iter = 0 iterates nothing and sets no flag but SKIPPED.  A row of iter_out_host is RPSF_STARS_FITPOS_COLUMNS float64:
 *   y0, x0, y, x, niter, flags, dy, dx (the last step taken or rejected, NaN if none was computed).
 * A row of fit_out_host is rpsf_stars_fit's row (RPSF_STARS_FIT_COLUMNS float64, S8's flags) at the (y, x) returned, computed by kernel S8
 * itself on those positions: it is what rpsf_stars_fit gives there, bit for bit.  No atomics, no workgroup waits for another, two runs
 * agree bit for bit.  This is not a PSF-photometry package's fit: the weights are uniform (no error column, no variance weighting), the
 * interpolation is bilinear, the cell is fixed, one star is fitted at a time (neighbours are not fitted together), and masked pixels are
 * left out, not corrected for.  n == 0 launches nothing and needs no pointers.  The call replaces nothing of the finder: a
 * rpsf_stars_positions, rpsf_stars_measure, rpsf_stars_photometry, rpsf_stars_refine or rpsf_stars_fit after it gives the bits it gave
 * before. */
#define RPSF_STARS_FITPOS_COLUMNS 8
#define RPSF_STARS_FITPOS_RAN_AWAY 1
#define RPSF_STARS_FITPOS_NOT_CONVERGED 2
#define RPSF_STARS_FITPOS_SINGULAR 4
#define RPSF_STARS_FITPOS_SKIPPED 8
int rpsf_stars_fit_positions(rpsf_stars* finder, const rpsf_stars_model* model, size_t n, const double* positions_host,
                             const int32_t* cells_host, double radius, int fit_background, int max_iter, double eps, double max_shift,
                             double max_step, int use_mesh, double* iter_out_host, double* fit_out_host);
/* Device time of the last S9 and the S8 that follows it, milliseconds; 0 when it launched nothing. */
int rpsf_stars_fit_positions_ms(const rpsf_stars* finder, double* ms);

/* MODEL AND RESIDUAL FRAMES (kernel S10): the sum of n fitted stars drawn with their cells of a rpsf_stars_model, or the
 * finder's frame with that sum taken out.  positions_host holds (y, x) per star (finite, |y|, |x| < 2^20), flux_host one float64 flux and
 * cells_host one int32 cell index per star; 0 < radius = R <= min(64, N / 2 - 1); the model on the finder's device; anything else is
 * RPSF_E_BADARG, before anything is launched or written.  Star i is DRAWN when flux_i is finite and 0 <= cell_i < n_cells; every other
 * star is skipped (so rpsf_stars_fit's flagged rows, whose flux is NaN, drop out by themselves), and *n_rendered (may be NULL) is the
 * number of stars drawn, on the frame or off it.
 * THE SUM at pixel (r, c) of the frame: s = 0.0; for i ascending over the stars drawn: pr = r - y_i, pc = c - x_i, q = pr pr + pc pc; when
 * q <= R R: s = s + flux_i * m, with m rpsf_stars_fit's model at (pr, pc) of cell_i (h = N / 2 - 0.5, the same float64 operations in
 * the same order, nothing fused).  mode:
 *   RPSF_STARS_RENDER_MODEL (0)          out = s; the frame is not read, no state is needed beyond the finder's shape;
 *   RPSF_STARS_RENDER_RESIDUAL (1)       out = (double)frame[p] - s;
 *   RPSF_STARS_RENDER_RESIDUAL_MESH (2)  out = ((double)frame[p] - background(r, c)) - s, the d that rpsf_stars_fit fitted with use_mesh.
 * The two residual modes read the frame, and mode 2 the filtered mesh, a rpsf_stars_background_view / _host / _scaled left on the device:
 * RPSF_E_STATE before such a call, and for mode 2 on a frame without a usable pixel (rpsf_stars_fit's NO_MESH); nothing is written then.
 * Masks play no part but through the mesh; NaN and Inf propagate as the arithmetic says; in mode 1 a pixel that no star reaches comes back
 * as its own bits, in mode 0 it is + 0.0.  out takes height x width elements in dense rows, float32 (s or the difference rounded once from
 * float64) or with out_float64 float64; it is host memory, or with out_on_device a pointer on the finder's device that the kernel writes
 * directly.  n == 0 is valid and needs no star pointers: mode 0 gives zeros, mode 1 the frame.
 * One workgroup owns a tile of RENDER tile rows x tile columns output pixels (rpsf_stars_render_info), one pixel per thread.  The host
 * builds a list per tile: star i is on it when the box floor(y - R) - 1 .. ceil(y + R) + 1 (likewise in x), clipped to the frame, meets
 * the tile; indices ascend within a list.  The kernel stages a list into LDS `chunk` records at a time, so no tile has a cap on its stars.
 * A gather: no atomics, no workgroup waits for another, two runs agree bit for bit.  This is not a PSF-photometry package's subtraction:
 * the interpolation is bilinear and does not conserve flux below the pixel scale, the disc cuts the model at R, and a per-star fitted
 * background is not subtracted.  The call replaces nothing of the finder: a rpsf_stars_positions, rpsf_stars_measure,
 * rpsf_stars_photometry, rpsf_stars_refine, rpsf_stars_fit or rpsf_stars_fit_positions after it gives the bits it gave before. */
#define RPSF_STARS_RENDER_MODEL 0
#define RPSF_STARS_RENDER_RESIDUAL 1
#define RPSF_STARS_RENDER_RESIDUAL_MESH 2
int rpsf_stars_render(rpsf_stars* finder, const rpsf_stars_model* model, size_t n, const double* positions_host, const double* flux_host,
                      const int32_t* cells_host, double radius, int mode, int out_float64, int out_on_device, void* out,
                      size_t* n_rendered);
/* Device time of the last S10, milliseconds. */
int rpsf_stars_render_ms(const rpsf_stars* finder, double* ms);
/* S10's tile (rows, columns) and the records of a chunk; any pointer may be NULL. */
int rpsf_stars_render_info(int* tile_rows, int* tile_cols, int* chunk);

/* GROUP FITS (kernel S11): blended neighbours fitted together - one flux per star, one shared constant, positions fixed -
 * with rpsf_stars_fit's definitions, so that S8, S10 and S11 agree bit for bit where they meet.
 * rpsf_stars_link_groups (host only, no handle): two ELIGIBLE stars i < j (eligible_host may be NULL: all are) are LINKED when
 * dy dy + dx dx <= link link, in float64, nothing fused; the groups are the connected components.  labels_host[i] is the smallest index
 * of i's component, sizes_host[i] its size as found (an ineligible star is a component of one).  A component of more than max_group
 * (1 .. RPSF_STARS_MAX_GROUP) members is broken up: each member is fitted alone, crowded_host[i] is RPSF_STARS_FIT_CROWDED (else 0), and
 * the size stays the component's.  link > 0 and finite, positions finite with |y|, |x| < 2^20; anything else is RPSF_E_BADARG.  Expected
 * linear time (a hashed grid of cells of side link and a union-find); the result does not depend on any order of visits.
 * rpsf_stars_fit_groups: rpsf_stars_fit's arguments, state rules and return codes, and 0 < link <= 2 R (beyond 2 R two discs share no
 * pixel), max_group in 1 .. 8 (1 fits every star alone).  A star is eligible when its cell index is inside the model and that cell is
 * all finite, and - with use_mesh - the frame has a valid mesh node.  Every star that is alone (a component of one, an ineligible or a
 * crowded star) goes through kernel S8's own launch: the first RPSF_STARS_FIT_COLUMNS of its row are rpsf_stars_fit's, bit for bit, the
 * flags included, and group = label, group_size = size, group_n = n, group_chi2 = chi2, group_abs = abs_res.  The groups of g = 2 ..
 * max_group members go through S11, one wave per group, members b = 0 .. g - 1 in ascending index.  Disc b HOLDS pixel (r, c) when
 * (r - y_b)^2 + (c - x_b)^2 <= R R, spelled as rpsf_stars_fit spells it.
 *   PASS 1  for a = 0 .. g - 1 over member a's box in S8's lane-strided raster order, on the pixels that disc a holds and no disc b < a
 *           does (the union of the discs, every pixel OWNED by the first member that holds it), on the frame and usable: with d and
 *           m_b = the model of member b for the members that hold the pixel: n += 1, Sd += d, Sdd += d d, Sm[b] += m_b, Sdm[b] += d m_b,
 *           and for c >= b, both holding: A[b][c] += m_b m_c.  A lane's partial sums run on across the members; one fold, S8's.
 *   SOLVE   unknowns f_0 .. f_{g-1}, then the constant with fit_background: p = g + fit_background; the matrix is A bordered by Sm and n,
 *           the right-hand side Sdm, then Sd; TOO_FEW: n < p; else rpsf_stars_fit_positions' LDL^T elimination at order p, in its order;
 *           DEGENERATE: a pivot not finite or <= 0, or an unknown not finite.  Either flag goes to every member and leaves NaN in f, bg
 *           and the residual's columns.  Near-coincident stars give a near-singular system and huge fluxes of opposite sign: nothing
 *           guards that but DEGENERATE at a pivot that is not positive.
 *   PASS 2  for a = 0 .. g - 1 over member a's disc exactly as S8 walks that star alone: n_all, Sm_all, and on the usable pixels n, Sm,
 *           Smm, Sd, Sdm, Sdd - rpsf_stars_fit's numbers for that star, bit for bit.  With e = d - (S + bg), S = 0.0 and then S += f_b *
 *           m_b over the members b (ascending) that hold the pixel (rpsf_stars_render's sum): chi2, abs_res and the peak as S8's; on the
 *           pixels a owns also the group's chi2 and abs_res, whose lane partials run on across the members and fold once.  A member
 *           without a usable pixel has no peak (NaN at (-1, -1)).
 * A row of out_host is RPSF_STARS_FIT_GROUPS_COLUMNS float64: rpsf_stars_fit's 20 columns with their meanings (bg is the shared
 * constant, or + 0.0), then group, group_size, group_n, group_chi2, group_abs.  No atomics, no workgroup waits for another, two runs agree
 * bit for bit; nothing of the finder is replaced.  This is not a PSF-photometry package's fit: uniform weights, fixed positions, bilinear
 * interpolation, the model cut at R, the cell fixed. */
#define RPSF_STARS_FIT_GROUPS_COLUMNS 25
#define RPSF_STARS_MAX_GROUP 8
#define RPSF_STARS_FIT_CROWDED 16
int rpsf_stars_link_groups(size_t n, const double* positions_host, const uint8_t* eligible_host, double link, int max_group,
                           int32_t* labels_host, int32_t* sizes_host, uint8_t* crowded_host);
int rpsf_stars_fit_groups(rpsf_stars* finder, const rpsf_stars_model* model, size_t n, const double* positions_host,
                          const int32_t* cells_host, double radius, int fit_background, int use_mesh, double link, int max_group,
                          double* out_host);
/* Device time of the last S11 with the S8 beside it, milliseconds; 0 when it launched nothing. */
int rpsf_stars_fit_groups_ms(const rpsf_stars* finder, double* ms);
/* The columns of a row, the largest group, and the groups a workgroup of S11 takes; any pointer may be NULL. */
int rpsf_stars_fit_groups_info(int* columns, int* max_group, int* groups_per_workgroup);

/* WEIGHTED FITS (kernel S12): rpsf_stars_fit with one weight per pixel, w = 1 / v, and the formal variances of what it
 * fits.  rpsf_stars_fit's arguments, state rules, return codes and messages, its box, walk, disc, model m, residual d, summation order and
 * flags.  THE VARIANCE v of a pixel p is a float64, from one of two sources:
 *   RPSF_STARS_VARIANCE_MAP (0)    v = (double)var[p]: a float32 frame of the finder's shape that rpsf_stars_variance_host / _view brought
 *                                  to the device (RPSF_E_STATE before such a call).  The two take the route and the rounding of
 *                                  rpsf_stars_background_host / _view - float64 is rounded to float32 once, a view may have any dtype and
 *                                  strides of rpsf_view - into a buffer of the finder that is allocated at the first call and freed with
 *                                  the finder.  They launch no kernel S1 and change nothing else of the finder; the variance frame stays
 *                                  until the next such call, whatever frames the finder is given in between.
 *   RPSF_STARS_VARIANCE_MODEL (1)  v = sky_variance + (img[p] > 0 ? (double)img[p] : 0.0) / gain, from the raw float32 pixel, not from d.
 *                                  sky_variance >= 0 and finite, gain > 0 (+inf: no photon term), not sky_variance == 0 with gain == +inf;
 *                                  anything else is RPSF_E_BADARG, before anything is launched.  (In MAP mode the two are not read.)
 * w = 1.0 / v.  A pixel is USABLE when rpsf_stars_fit's rule holds (finite, not masked, on the frame) and w > 0 and w is finite: a v that
 * is NaN, <= 0, +inf or so small that w overflows takes the pixel out of the fit.  It still counts in n_all and Sm_all and shows as lower
 * coverage; there is no flag of its own.  PASS 1, per usable pixel, in this order:  wm = w m, wd = w d, Sm += m, Sw += w, Swm += wm,
 * Swmm += wm m, Swd += wd, Swdm += wd m, Swdd += wd d.  THE SOLVE: with fit_background D = Sw Swmm - Swm Swm, f = (Sw Swdm - Swm Swd) / D,
 * bg = (Swd - f Swm) / Sw, var_f = Sw / D, var_bg = Swmm / D, cov = - Swm / D; without, D = Swmm, f = Swdm / D, bg = 0, var_f = 1 / D,
 * var_bg = cov = 0.  FLAGS are rpsf_stars_fit's (TOO_FEW on the usable count n); with any flag f, bg, the three variances and PASS 2's
 * columns are NaN and the peak sits at (-1, -1).  PASS 2, with e = d - (f m + bg): chi2 = sum w (e e); abs_res = sum |e| and the peak of e
 * are unweighted, rpsf_stars_fit's.  No square root is taken on the device.  With v = 1 everywhere f, bg, chi2, abs_res and the peak are
 * rpsf_stars_fit's bit for bit; with v = 2^k everywhere f, bg, abs_res and the peak stay, chi2 is 2^-k times and var_f = 2^k (n / D) of
 * rpsf_stars_fit's sums, exactly.  A row of out_host is RPSF_STARS_FIT_WEIGHTED_COLUMNS float64:
 *   y, x, cell, flags, n, n_all, Sm, Sm_all, Sw, Swm, Swmm, Swd, Swdm, Swdd, f, bg, var_f, var_bg, cov, chi2, abs_res, peak_res, peak_e,
 *   peak_row, peak_col.
 * n == 0 launches nothing and needs no pointers.  No atomics, no workgroup waits for another, two runs agree bit for bit; nothing of the
 * finder is replaced.  This is not a PSF-photometry package's fit: the position is given and not fitted, the interpolation is bilinear, the
 * model is cut at R, and the variances are formal - what the given v imply and nothing else. */
#define RPSF_STARS_FIT_WEIGHTED_COLUMNS 25
#define RPSF_STARS_VARIANCE_MAP 0
#define RPSF_STARS_VARIANCE_MODEL 1
int rpsf_stars_variance_host(rpsf_stars* finder, const void* variance_host, int variance_is_f64);
int rpsf_stars_variance_view(rpsf_stars* finder, const rpsf_view* variance);
int rpsf_stars_fit_weighted(rpsf_stars* finder, const rpsf_stars_model* model, size_t n, const double* positions_host,
                            const int32_t* cells_host, double radius, int fit_background, int use_mesh, int variance_mode,
                            double sky_variance, double gain, double* out_host);
/* Device time of the last S12, milliseconds; 0 when it launched nothing. */
int rpsf_stars_fit_weighted_ms(const rpsf_stars* finder, double* ms);

/* rpsf_builder_add_frame on a dense float32 frame that is already on the builder's device - a finder's (rpsf_stars_frame) or the caller's
 * own; it is only read, nothing is uploaded but the star list.  On a scaled builder the frame is the SCALED one and height and width are
 * its. */
int rpsf_builder_add_frame_device(rpsf_builder* builder, const float* frame_dev, int height, int width, int n_stars,
                                  const int32_t* corners_i32, const double* frac_f64, double saturation_threshold, double star_minimum,
                                  double star_maximum, uint8_t* accepted_u8_host);

/* NEIGHBOUR-SUBTRACTED PATCHES (kernel B1n): rpsf_builder_add_frame with the fitted stars of the frame taken out of every
 * patch except the patch's own star, so that a neighbour inside a patch does not enter the cell's average.  The subtraction set is S10's
 * (rpsf_stars_render): n_all stars with positions_host (n_all x 2 float64, (row, col)), flux_host (float64), cells_host (int32) and their
 * cells of `model`; a star is drawn when its flux is finite and its cell is one of the model's, every other star takes no part.  Patch k
 * (k < n_stars: corners_i32, frac_f64 as in rpsf_builder_add_frame) leaves star own_i32[k] of the set in; own_i32[k] = -1 leaves nobody in
 * (a patch cut at a position that is not in the set).
 *
 * DEFINITION.  For patch pixel (r, c), with (rr, rc) the patch's rounded corner and mirror the reflect index map of
 * rpsf_builder_add_frame: fr = mirror(rr + r, height), fc = mirror(rc + c, width); s = 0; for the drawn stars j != own[k] in ascending j:
 * pr = fr - row_j, pc = fc - col_j, and when pr pr + pc pc <= R R: s += flux_j * m with m rpsf_stars_fit's bilinear model of cell_j at
 * (pr, pc), all in float64.  The pixel enters the patch as (double)(float)((double)frame[fr][fc] - s): bit for bit the value
 * rpsf_builder_add_frame_device reads from the float32 frame rpsf_stars_render(RPSF_STARS_RENDER_RESIDUAL) writes with star own[k] left out,
 * and the frame's own bits where no star reaches.  Everything after this gather - the spline shift, the background plane, the tests, the
 * append to the stack - is rpsf_builder_add_frame's and unchanged (regularizepsf/image_processing.py:82-121).  The host builds one
 * neighbour list per patch through a bucket grid (time linear in stars and patches); no atomics, two calls agree bit for bit.
 *
 * RPSF_E_BADARG before anything is launched or written: a null argument, `radius` outside 0 < R <= min(64, N_m / 2 - 1) of the model's
 * N_m, a position that is not finite or not inside |row|, |col| < 2^20, an own_i32[k] outside -1 ... n_all - 1, a model on another
 * device than the builder, and what rpsf_builder_add_frame refuses.  RPSF_E_UNSUPPORTED: a wide builder (rpsf_builder_create_wide) or a
 * scaled one.  n_all == 0 is valid (model and the three arrays may then be NULL) and is rpsf_builder_add_frame itself.  The device time of
 * B1n is the patch figure of rpsf_builder_kernel_ms. */
int rpsf_builder_add_frame_subtracted(rpsf_builder* builder, const void* image_host, int image_is_f64, int height, int width,
                                      const rpsf_stars_model* model, size_t n_all, const double* positions_host, const double* flux_host,
                                      const int32_t* cells_host, double radius, int n_stars, const int32_t* own_i32,
                                      const int32_t* corners_i32, const double* frac_f64, double saturation_threshold, double star_minimum,
                                      double star_maximum, uint8_t* accepted_u8_host);
/* The same on a dense float32 frame that is already on the builder's device (rpsf_builder_add_frame_device's frame_dev). */
int rpsf_builder_add_frame_device_subtracted(rpsf_builder* builder, const float* frame_dev, int height, int width,
                                             const rpsf_stars_model* model, size_t n_all, const double* positions_host,
                                             const double* flux_host, const int32_t* cells_host, double radius, int n_stars,
                                             const int32_t* own_i32, const int32_t* corners_i32, const double* frac_f64,
                                             double saturation_threshold, double star_minimum, double star_maximum,
                                             uint8_t* accepted_u8_host);
/* The star records B1n stages at a time, the side of a bucket of the host's grid in pixels, and the LDS of a B1n workgroup at N = 128 in
 * bytes; any pointer may be NULL. */
int rpsf_builder_subtract_info(int* chunk, int* bucket, size_t* lds_bytes_128);

/* Host-side helper for the saturation branch of apply (transform.py:135-138): sequential, row-major
 * NaN-ignoring neighbourhood-mean fill of the masked pixels of the float64 padded image (no GPU involved). */
int rpsf_saturation_fill(double* padded, int rows, int cols, const uint8_t* mask, int neighborhood_width);

/* Device memory helpers for callers that keep frames resident (bench, tests, streaming). */
int rpsf_dev_alloc(int device, size_t bytes, void** out);
int rpsf_dev_free(int device, void* ptr);
int rpsf_memcpy_h2d(int device, void* dst_dev, const void* src_host, size_t bytes);
int rpsf_memcpy_d2h(int device, void* dst_host, const void* src_dev, size_t bytes);
/* A plain copy between two buffers of one device, finished on return; *ms (may be NULL) takes its device time in milliseconds - the
 * yardstick the timing scripts put a frame-sized kernel next to. */
int rpsf_memcpy_d2d(int device, void* dst_dev, const void* src_dev, size_t bytes, double* ms);
int rpsf_device_synchronize(int device);

/* Multi-GPU row-band sharding (one process per GPU).  The caller splits the patch lattice into
 * contiguous row bands; each rank builds a plan for its band only (image rows it reads, patches it
 * owns) and, after the local apply, exchanges the seam rows its last lattice row spilled into the
 * next rank's band.  rpsf_comm_* wraps RCCL (loaded with dlopen) for exactly that neighbour
 * exchange; unique_id is 128 bytes, created on rank 0 and distributed by the caller. */
typedef struct rpsf_comm rpsf_comm;
int rpsf_comm_unique_id(void* id128);
int rpsf_comm_create(rpsf_comm** out, int device, int rank, int world, const void* id128);
void rpsf_comm_destroy(rpsf_comm* comm);
/* Send `send_count` floats at send_dev to rank+1 (if any) and receive `recv_count` floats from
 * rank-1 (if any) into recv_dev, then add recv_dev[0:recv_count] into accum_dev.  Any count may be 0. */
int rpsf_comm_seam_exchange_add(rpsf_comm* comm, const void* send_dev, size_t send_count, void* recv_dev,
                                size_t recv_count, void* accum_dev, void* stream);
/* The exchange alone, without the add - for callers that compute the spill rows first, on a stream of their own,
 * and let the transfer run beside the rest of the band (regularizepsf_amd/sharding.py).  stream NULL: the
 * communicator's own stream (rpsf_comm_stream). */
int rpsf_comm_seam_exchange(rpsf_comm* comm, const void* send_dev, size_t send_count, void* recv_dev, size_t recv_count,
                            void* stream);
void* rpsf_comm_stream(rpsf_comm* comm);
/* The number of ranks RCCL reports for the communicator (ncclCommCount) - evidence for a harness that the seam exchange
 * spans the GPUs it was launched on. */
int rpsf_comm_ranks(rpsf_comm* comm, int* ranks);
/* Make `waiter` (a hipStream_t) wait for everything enqueued on `signaller` so far. */
int rpsf_stream_wait(int device, void* waiter, void* signaller);
/* Block the calling thread until everything enqueued on `stream` (a hipStream_t of `device`) has finished: what DeviceArray.to_host waits
 * with for the one stream its array was last written on, instead of for the whole device. */
int rpsf_stream_synchronize(int device, void* stream);
/* Events (hipEvent_t without timing) for dependencies that span steps: record on one stream now, make another stream wait for
 * it later (the sharded step's double-buffered seam rows). */
int rpsf_event_create(int device, void** event);
int rpsf_event_record(void* event, void* stream);
int rpsf_stream_wait_event(void* stream, void* event);
int rpsf_event_destroy(void* event);
/* accum_dev[0:count] += src_dev[0:count] (float32, on `device`, asynchronous on stream): the add of the seam
 * exchange by itself, for callers that move the seam rows with their own transport. */
int rpsf_add_rows(int device, void* accum_dev, const void* src_dev, size_t count, void* stream);
/* The same add on at most max_workgroups workgroups of 256 threads: for a caller that runs it beside a persistent patch launch
 * (the pipelined seam exchange of regularizepsf_amd/sharding.py), whose workgroups need whole CUs. */
int rpsf_add_rows_narrow(int device, void* accum_dev, const void* src_dev, size_t count, int max_workgroups, void* stream);
int rpsf_comm_barrier(rpsf_comm* comm, void* stream);
/* max over ranks of one double (used for whole-job timing) */
int rpsf_comm_allreduce_max(rpsf_comm* comm, double* value);

#ifdef __cplusplus
}
#endif
#endif /* RPSF_H */
