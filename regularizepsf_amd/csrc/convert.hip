// convert.hip - the conversion kernels of the device-array views (include/rpsf.h, rpsf_view): C1 gathers a view of any supported dtype and
// strides into a dense float32 frame, C2 scatters a dense float32 frame into a float32 / float64 / float16 view.  The per-thread bodies,
// the zero-copy predicate and the argument checks are csrc/rpsf_core_convert.hpp (run on the CPU by tests/emu/emu_convert.cpp); here are
// the kernels, their launches and the two entry points that need no plan.  A launch is a grid-stride grid of at most
// rpsfconv::MAX_WORKGROUPS workgroups per frame, the frame of a stack being blockIdx.y.
#include "rpsf_convert.hpp"
#include "rpsf_core_convert.hpp"
#include "rpsf_side_unit.hpp"

using namespace rpsfconv;

template <class T>
__global__ void __launch_bounds__(WG) convert_c1_kernel(Args a) {
  c1_thread<T>(a, (int64_t)blockIdx.x * WG + threadIdx.x, (int64_t)gridDim.x * WG, (int)blockIdx.y);
}
template <class T>
__global__ void __launch_bounds__(WG) convert_c2_kernel(Args a) {
  c2_thread<T>(a, (int64_t)blockIdx.x * WG + threadIdx.x, (int64_t)gridDim.x * WG, (int)blockIdx.y);
}

int rpsf_conv_gather(const rpsf_view& v, int frames, int64_t frame_stride, float* dense, int64_t dense_frame_stride, hipStream_t st) {
  if (frames <= 0 || v.rows == 0 || v.cols == 0) return RPSF_OK;
  if (frames > 65535) return fail(RPSF_E_BADARG, "more than 65535 frames in one conversion launch");
  const Args a = make_args(v, frames, frame_stride, dense, dense_frame_stride);
  const dim3 grid(workgroups_for(chunks_of(a, chunk_elems(v.dtype))), (unsigned)frames);
  const bool known = dispatch_dtype(v.dtype, [&]<class T>() { convert_c1_kernel<T><<<grid, dim3(WG), 0, st>>>(a); });
  if (!known) return fail(RPSF_E_BADARG, "unknown dtype");
  HIP_TRY(hipGetLastError());
  return RPSF_OK;
}

int rpsf_conv_scatter(const float* dense, int64_t dense_frame_stride, const rpsf_view& v, int frames, int64_t frame_stride, hipStream_t st) {
  if (frames <= 0 || v.rows == 0 || v.cols == 0) return RPSF_OK;
  if (frames > 65535) return fail(RPSF_E_BADARG, "more than 65535 frames in one conversion launch");
  const Args a = make_args(v, frames, frame_stride, const_cast<float*>(dense), dense_frame_stride);
  const dim3 grid(workgroups_for(chunks_of(a, chunk_elems(v.dtype))), (unsigned)frames);
  switch (v.dtype) {
    case RPSF_DTYPE_FLOAT32: convert_c2_kernel<float><<<grid, dim3(WG), 0, st>>>(a); break;
    case RPSF_DTYPE_FLOAT64: convert_c2_kernel<double><<<grid, dim3(WG), 0, st>>>(a); break;
    case RPSF_DTYPE_FLOAT16: convert_c2_kernel<Half><<<grid, dim3(WG), 0, st>>>(a); break;
    default: return fail(RPSF_E_BADARG, "an output view is float32, float64 or float16");
  }
  HIP_TRY(hipGetLastError());
  return RPSF_OK;
}

extern "C" int rpsf_view_route(const rpsf_view* image, const rpsf_view* out, int* route) {
  if (!route) return fail(RPSF_E_BADARG, "route is null");
  bool e_in, e_out;
  if (const char* why = view_problem(image, false, &e_in)) return fail(RPSF_E_BADARG, std::string("image: ") + why);
  if (const char* why = view_problem(out, true, &e_out)) return fail(RPSF_E_BADARG, std::string("out: ") + why);
  *route = (zero_copy(*image) ? 0 : RPSF_ROUTE_C1) | (zero_copy(*out) ? 0 : RPSF_ROUTE_C2);
  return RPSF_OK;
}

extern "C" int rpsf_convert_view(int device, const rpsf_view* src, const rpsf_view* dst, void* stream) {
  bool e_in, e_out;
  if (const char* why = view_problem(src, false, &e_in)) return fail(RPSF_E_BADARG, std::string("src: ") + why);
  if (const char* why = view_problem(dst, false, &e_out)) return fail(RPSF_E_BADARG, std::string("dst: ") + why);
  if (src->rows != dst->rows || src->cols != dst->cols) return fail(RPSF_E_BADARG, "src and dst must have one shape");
  const bool gather = dense_f32(*dst);
  if (!gather) {
    if (!dense_f32(*src)) return fail(RPSF_E_BADARG, "one side must be a dense float32 view");
    if (const char* why = view_problem(dst, true, &e_out)) return fail(RPSF_E_BADARG, std::string("dst: ") + why);
  }
  if (e_in) return RPSF_OK;
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return gather ? rpsf_conv_gather(*src, 1, 0, static_cast<float*>(dst->data), 0, st)
                : rpsf_conv_scatter(static_cast<const float*>(src->data), 0, *dst, 1, 0, st);
}
