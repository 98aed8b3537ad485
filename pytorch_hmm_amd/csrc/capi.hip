// hmm355 — C ABI housekeeping (error strings, version).
#include "common.h"

HMM355_API int hmm355_version(void) { return 14; }

HMM355_API const char* hmm355_strerror(int code) {
  switch (code) {
    case HMM355_OK: return "ok";
    case HMM355_E_ARG: return "invalid argument (null pointer, negative size or unknown mode)";
    case HMM355_E_STATES: return "number of states outside the op's range (HMM recursions [1, 256], their *_wide forms [1, 4096], HSMM [1, 1024], HSMM forward-backward [1, 256], CTC target length [1, 2048], duration-constrained Viterbi [1, 256] with group * S <= 4096, forced-alignment chain positions [1, 4096], explicit-duration forced alignment positions [1, 1024] with durations [1, 128] and positions * durations <= 16384, emission statistics components per state [1, 256] with states * components <= 65536, N-best Viterbi [1, 256] with at most 16 paths, arc-list recursions hmm355_sparse_* [1, 8192])";
    case HMM355_E_SHAPE: return "invalid shape (T < 1, a DTW matrix without rows or columns, or size overflow)";
    case HMM355_E_WORKSPACE: return "workspace too small";
    case HMM355_E_DURATION: return "HSMM max_duration outside [1, 1024] (HSMM forward-backward: [1, 128] with S * max_duration <= 16384)";
    default: break;
  }
  if (code > 0) return hipGetErrorString(static_cast<hipError_t>(code));
  return "unknown hmm355 error";
}
