// CPU emulator for rpsf_core_convert.hpp (test infrastructure, never shipped in the product path): the thread bodies of the conversion
// kernels C1 and C2 run one after the other over the grid csrc/convert.hip launches - the same chunking, the same choice between 16-byte
// and element accesses (make_args), the same conversions - so that every dtype, shape and view is checked against NumPy without a GPU.
#include <cstdint>

#include "../../regularizepsf_amd/csrc/rpsf_core_convert.hpp"

using namespace rpsfconv;

// `view`: the strided side; `dense`: rows x cols float32.  gather != 0: C1 (view -> dense), else C2 (dense -> view).
// workgroups <= 0: the launch's own grid, else that many workgroups (a small grid makes every thread stride).
// *vec_or_null: bit 0 the strided side moved by 16-byte accesses, bit 1 the dense side did.
extern "C" int emu_convert(const rpsf_view* view, float* dense, int gather, int workgroups, int* vec_or_null) {
  bool empty;
  if (view_problem(view, gather == 0, &empty)) return -1;
  if (empty) return 0;
  const Args a = make_args(*view, 1, 0, dense, 0);
  if (vec_or_null) *vec_or_null = (a.strided_vec ? 1 : 0) | (a.dense_vec ? 2 : 0);
  const int64_t wgs = workgroups > 0 ? workgroups : workgroups_for(chunks_of(a, chunk_elems(view->dtype)));
  const int64_t threads = wgs * WG;
  bool known = true;
  for (int64_t tid = 0; tid < threads && known; ++tid) {
    if (gather) known = dispatch_dtype(view->dtype, [&]<class T>() { c1_thread<T>(a, tid, threads, 0); });
    else if (view->dtype == RPSF_DTYPE_FLOAT32) c2_thread<float>(a, tid, threads, 0);
    else if (view->dtype == RPSF_DTYPE_FLOAT64) c2_thread<double>(a, tid, threads, 0);
    else c2_thread<Half>(a, tid, threads, 0);
  }
  return known ? 0 : -1;
}
