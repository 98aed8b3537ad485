// hmm355 — the host plumbing in front of every kernel: one launch, one early return, the
// state-count and flag dispatch, the row-pass grid and the workspace carver.  Host code only;
// an op's .hip file uses these and carries no plumbing of its own.
#pragma once
#include "common.h"

namespace hmm355 {

// hipError_t is an unscoped enum and success is 0 on both sides, so `return e_;` is right in the
// internal launchers (hipError_t) and in the extern "C" entry points (int status) alike.
static_assert(HMM355_OK == 0 && hipSuccess == 0, "HMM355_TRY returns a hipError_t as a status");
#define HMM355_TRY(expr)                  \
  do {                                    \
    const hipError_t e_ = (expr);         \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

template <typename T>
struct as_given { using type = T; };

// Raises the kernel's dynamic-LDS cap where lds_bytes needs it, launches, and returns the launch's
// status.  The arguments are not deduced: a literal or nullptr converts to the kernel's own
// parameter type.
template <typename... P>
inline hipError_t launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st,
                         typename as_given<P>::type... args) {
  HMM355_TRY(allow_lds(kernel, lds_bytes));
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, st, args...);
  return hipGetLastError();
}

// f(std::integral_constant<int, NP>{}) for the padded state count NP (pad_states: 64, 128, else 256)
template <typename F>
inline auto with_np(int NP, F&& f) {
  switch (NP) {
    case 64: return f(std::integral_constant<int, 64>{});
    case 128: return f(std::integral_constant<int, 128>{});
    default: return f(std::integral_constant<int, 256>{});
  }
}
// f(std::true_type{}) or f(std::false_type{}): one boolean template argument
template <typename F>
inline auto with_flag(bool on, F&& f) {
  return on ? f(std::true_type{}) : f(std::false_type{});
}

// the grid of a one-wave-per-row pass of 256 threads (four rows a workgroup), at most cap workgroups
inline unsigned row_grid(size_t rows, size_t cap) {
  const size_t blocks = (rows + 3) / 4;
  return (unsigned)(blocks < cap ? blocks : cap);
}

// Carves a workspace into 256-B aligned pieces in the order they are taken.  With base == nullptr
// it only sizes: a layout function is one pass that fills its struct and returns bytes().
struct Carver {
  char* base;
  size_t at = 0;
  template <typename T>
  T* take(size_t count) {
    const size_t o = at;
    at += align_up(count * sizeof(T), 256);
    return base ? reinterpret_cast<T*>(base + o) : nullptr;
  }
  size_t bytes() const { return at; }
};

// zeroes n 4-byte words with zero_words_kernel (common.h: a kernel node, not a memset)
inline hipError_t zero_words(void* p, size_t bytes, hipStream_t st) {
  const int n = (int)((bytes + 3) / 4);
  const int blocks = n < 256 * 64 ? (n + 255) / 256 : 64;
  return launch(zero_words_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, st, static_cast<unsigned*>(p), n);
}
// the counts before a publishing launch: a fresh token for an eager call, else token 0 and
// the reset kernel
inline hipError_t prepare_counts(void* p, size_t bytes, hipStream_t st, unsigned* token) {
  if (!stream_capturing(st)) {
    *token = next_count_token();
    return hipSuccess;
  }
  *token = 0u;
  return zero_words(p, bytes, st);
}

}  // namespace hmm355
