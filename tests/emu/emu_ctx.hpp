// The context of the CPU lane emulators: each() runs the body for every thread of a workgroup in turn, and returning from it is the
// barrier.  (Test infrastructure, never shipped in the product path.)
#pragma once

struct CpuCtx {
  int threads;
  template <class F>
  void each(F&& f) {
    for (int t = 0; t < threads; ++t) f(t);
  }
};
