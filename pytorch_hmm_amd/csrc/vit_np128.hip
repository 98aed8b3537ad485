// hmm355 — Viterbi kernels for NP = 128 (vit_kern.h; one translation unit per NP).
#include "vit_kern.h"

namespace hmm355 {
template hipError_t launch_vit<128>(const VitArgs& va, bool prep, hipStream_t sm);
}  // namespace hmm355

// diagnostic builds: the stamps live in this translation unit's code object (recur.h)
#if HMM355_STAMP
HMM355_API int hmm355_debug_stamps_vit(unsigned long long* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(hmm355::g_rec_stamps), sizeof(unsigned long long) * (size_t)n);
}
#endif
// diagnostic builds: every form of the chains' wave reduction on n host vectors of 64 floats
// (recur.h red_probe_kernel); out[n][8]
#if HMM355_RED_PROBE
HMM355_API int hmm355_debug_red_probe(const float* in, float* out, int n) {
  float *din = nullptr, *dout = nullptr;
  const size_t ib = sizeof(float) * 64 * (size_t)n, ob = sizeof(float) * 8 * (size_t)n;
  hipError_t e = hipMalloc(&din, ib);
  if (e == hipSuccess) e = hipMalloc(&dout, ob);
  if (e == hipSuccess) e = hipMemcpy(din, in, ib, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hmm355::launch(hmm355::red_probe_kernel, dim3((n + 3) / 4), dim3(256), 0, 0, din, dout, n);
  if (e == hipSuccess) e = hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost);
  (void)hipFree(din);
  (void)hipFree(dout);
  return (int)e;
}
#endif
