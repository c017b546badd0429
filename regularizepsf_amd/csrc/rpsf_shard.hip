// rpsf_shard.hip - what the sharded row-band step (regularizepsf_amd/sharding.py) and other callers that manage device memory themselves
// take from librpsf_hip.so beside the plan: device allocations and copies, the RCCL loader with the communicator and its seam exchange,
// streams and events, and the seam add (kernel K4: add_rows_kernel, rpsf_kernels_shard.hpp, defined in this unit).  No counterpart in the
// reference, which runs on one host.  Touches nothing of a plan.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>

#include "rpsf_side_unit.hpp"
#include "rpsf_kernels_shard.hpp"

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
extern "C" int rpsf_memcpy_d2d(int device, void* dst, const void* src, size_t bytes, double* ms) {
  HIP_TRY(hipSetDevice(device));
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (ms) {
    for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(ev[0], nullptr));
  }
  const hipError_t copied = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, nullptr);
  if (ms && copied == hipSuccess) {
    float t = 0;
    HIP_TRY(hipEventRecord(ev[1], nullptr));
    HIP_TRY(hipEventSynchronize(ev[1]));
    HIP_TRY(hipEventElapsedTime(&t, ev[0], ev[1]));
    *ms = t;
  }
  for (auto e : ev)
    if (e) (void)hipEventDestroy(e);
  HIP_TRY(copied);
  HIP_TRY(hipStreamSynchronize(nullptr));
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
