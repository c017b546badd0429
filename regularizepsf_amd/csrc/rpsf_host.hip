// rpsf_host.hip - the host-array entry points of librpsf_hip.so: one frame whole or in row bands (views of the plan), the streamed
// pipeline of a frame sequence, page-locked memory for callers, the NUMA node of a device, the PCIe probe and the self-test of the
// worker pool.  Stands in for the astype on the way into ArrayPSFTransform.apply and the float64 result on the way out
// (regularizepsf/transform.py:117, :174-177); the correction itself is the plan's launch (rpsf.hip: rpsf_detail_launch_apply once per band,
// rpsf_detail_launch_batch once per group).  Launches no kernel of its own: staging, threads and copies (rpsf_hostpipe.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "rpsf_plan.hpp"

// ------------------------------------------------------------------------------------------------
// Host arrays in, host arrays out (what ArrayPSFTransform.apply hands over and gets back: transform.py:117 astype on the
// way in, :174-177 a float64 result on the way out).  Nothing below creates a thread or allocates per call once a plan
// has seen its frame size: conversions run on the persistent pool, staging lives in the plan's HostPipe.
// ------------------------------------------------------------------------------------------------
using rpsf_host::HostPipe;
using rpsf_host::HostPool;

int rpsf_detail_pipe_ensure(rpsf_plan* p, size_t slot_floats, int depth) {
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
int rpsf_detail_host_parts_for(size_t bytes) {
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

// Row bands of one large host frame: the lattice rows are cut into `want` groups; band b owns the output rows from its first lattice
// row to the next band's and runs every patch that reaches into them - its own lattice rows and the one above, which both neighbours
// compute (the collective-free seam of regularizepsf_amd/sharding.py, on one GPU) - as a view of the plan.  A band can run as soon as the
// image rows its patches read are on the device, and its rows can leave while the next band is still arriving: upload, patches and download
// of one frame overlap.  Returns the number of bands (0: this plan / frame is not cut - the caller takes the whole-frame path).
static int ensure_bands(rpsf_plan* p, const rpsf_geometry& g, int want) {
  if (p->bands_h == g.height && p->bands_w == g.width && p->bands_mode == g.pad_mode && p->bands_want == want) return (int)p->bands.size();
  rpsf_detail_drop_bands(p);
  p->bands_h = g.height, p->bands_w = g.width, p->bands_mode = g.pad_mode, p->bands_want = want;  // (remembered also when the answer is "no bands")
  if (p->generic || p->parent || !p->lattice || (rpsf_detail_overlap_kind(p) != OV_PLANES && rpsf_detail_overlap_kind(p) != OV_SWEEP) || g.pad_mode == RPSF_PAD_WRAP || want < 2) return 0;
  RowBands cuts;
  const int B = row_bands(p->N, p->n_patches, p->h_coords.data(), g.height, want, (int)HostPipe::MAX_BANDS, cuts);
  std::vector<std::unique_ptr<rpsf_plan>> bands;
  for (int b = 0; b < B; ++b) {
    std::vector<int32_t> coords;
    for (const int32_t i : cuts.patches[b]) coords.push_back(p->h_coords[2 * i]), coords.push_back(p->h_coords[2 * i + 1]);
    rpsf_plan* view = nullptr;
    if (rpsf_detail_plan_create_impl(&view, p->device, p->N, (int)cuts.patches[b].size(), coords.data(), p, cuts.patches[b].data()) != RPSF_OK) return 0;
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
          if (err == hipSuccess && rpsf_detail_launch_apply(p->bands[b].get(), q.d_in[0], q.d_out[0] + (size_t)R0 * W, gb, p->stream, nullptr) != RPSF_OK)
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
    std::fprintf(stderr, "[rpsf host frame] %zu chunks, %d bands, %zu + %zu pieces: last chunk enqueued %.3f ms, first piece back %.3f, last %.3f, total %.3f ms\n",
                 chunks.size(), B, n_in, (size_t)out_avail.load(), t_enqueued, t_first_out, t_last_out, ms_since(t_start));
  if (err != hipSuccess) return rpsf_detail_drain_after_error(p, err, "host frame");
  return rpsf_detail_sweep_check(p);
}

// One frame.  The conversions run chunk by chunk (>= 4 MiB) on the pool, each chunk's H2D copy starts as soon as it is staged,
// and on the way back each chunk is widened as soon as it has landed: conversion and PCIe overlap inside the frame.
static int host_one_frame(rpsf_plan* p, const void* image, int in_f64, void* out, int out_f64, const rpsf_geometry& g) {
  const size_t count = (size_t)g.height * g.width, bytes = count * sizeof(float);
  int rc = rpsf_detail_pipe_ensure(p, count, 1);
  if (rc != RPSF_OK) return rc;
  HostPipe& q = *p->pipe;
  HostPool& pool = HostPool::get(p->device);
  const int T = rpsf_detail_host_parts_for(bytes / std::max<size_t>(1, std::min<size_t>(HostPipe::MAX_CHUNKS, std::max<size_t>(1, bytes >> 22))));
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
  if (one_stream && err == hipSuccess && rpsf_detail_overlap_kind(p) == OV_SWEEP && p->sweep.ok && !dev_env("RPSF_NO_ZC_OUT")) {
    void* dev = nullptr;
    if (rpsf_detail_lattice_covers_window(p, g) && hipHostGetDevicePointer(&dev, direct_out ? out : static_cast<void*>(q.h_out[0]), 0) == hipSuccess) zc_out = static_cast<float*>(dev);
    else (void)hipGetLastError();
  }
  if (err == hipSuccess && rpsf_detail_launch_apply(p, q.d_in[0], zc_out ? zc_out : q.d_out[0], g, p->stream, nullptr) != RPSF_OK) err = hipErrorUnknown;
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
  if (err != hipSuccess) return rpsf_detail_drain_after_error(p, err, "host frame");
  return rpsf_detail_sweep_check(p);
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
  int rc = rpsf_detail_pipe_ensure(p, count * G, depth);
  if (rc != RPSF_OK) return rc;
  HostPipe& q = *p->pipe;
  HostPool& pool = HostPool::get(p->device);
  const int T = rpsf_detail_host_parts_for(bytes * G);  // (a job stages / unstages a whole group: small frames still give every worker a part)
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
    if (err == hipSuccess && rpsf_detail_launch_batch(p, q.d_in[sg], q.d_out[sg], fg, count, count, g, p->stream) != RPSF_OK) err = hipErrorUnknown;
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
  if (err != hipSuccess) return rpsf_detail_drain_after_error(p, err, "streamed frames");
  return rpsf_detail_sweep_check(p);
}

static int check_host_call(rpsf_plan* p, const void* a, const void* b, int n_frames, int height, int width, int pad_mode, float pad_value,
                           rpsf_geometry* g) {
  if (!p || !a || !b) return fail(RPSF_E_BADARG, "null argument");
  if (n_frames <= 0) return fail(RPSF_E_BADARG, "n_frames must be positive");
  if (!p->have_k) return fail(RPSF_E_STATE, "no transfer kernel installed (call rpsf_plan_set_transfer first)");
  *g = rpsf_geometry{height, width, pad_mode, pad_value, 0, 0, 0, height, width, 0, height, width};
  int rc = rpsf_detail_check_geometry(p, g);
  if (rc != RPSF_OK) return rc;
  HIP_TRY(hipSetDevice(p->device));
  // every host-array entry point: the plan's launch lanes are joined first (rpsf_lanes.hpp), and an error word nobody collected is not this call's
  if (const int jrc = rpsf_detail_join_lanes(p); jrc != RPSF_OK) return jrc;
  rpsf_detail_clear_error(p);
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
