// rpsf_construct.hip - the construct side of librpsf_hip.so: the transfer kernel from two sets of spectra (regularizepsf/transform.py:78-82,
// kernel K2: build_transfer_kernel, rpsf_kernels.hpp), the spectra of PSF samples (regularizepsf/psf.py:216-219, kernel K3: psf_fft_kernel<C>,
// the forward half of the first-generation patch plans, instantiated in the k1_*.hip units) and the built-in PSF models rasterised on
// the device (psf.py:65-70,159-165, kernel K6: rasterize_kernel, rpsf_kernels_construct.hpp, defined in this unit).  Needs no rpsf_plan:
// from rpsf_plan.hpp it takes dispatch_n, PatchPlan, upload_tables and DevBuf.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "rpsf_plan.hpp"
#include "rpsf_kernels_construct.hpp"

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
