// hmm355 — shared device helpers for the gfx950 (CDNA4) kernels.
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/hmm355.h"

#define HMM355_API extern "C" __attribute__((visibility("default")))

// Ablation knobs for diagnostic builds only (tools/ablate.py); 0 in the product build.  The bits
// are named in namespace abl below.
#ifndef HMM355_ABL
#define HMM355_ABL 0
#endif

#ifndef HMM355_STAMP
#define HMM355_STAMP 0
#endif

// HMM355_RED_FORM: the form of the banded chains' wave reduction (recur.h wave_red_level, namespace
// red: 0 six dependent DPP levels, 1 the quad_perm pair as three row_shr of one register, 2 the
// row_ror pair likewise, 3 both).  Not defined in the product build: recur.h then takes the form
// each chain measured fastest with (red_form: HMM355_RED_FORM_ALPHA / _BETA / _VIT); defined, it
// sets all three chains, for diagnostic builds.  HMM355_RED_PROBE (diagnostic builds,
// tools/probe_wave_reduce.py): exports a kernel that runs every form on caller-given vectors.
#ifndef HMM355_RED_PROBE
#define HMM355_RED_PROBE 0
#endif

// HMM355_FABL: ablation knobs of the work beside the chains (csrc/follow.h), diagnostic builds
// only; the bits are named in namespace fabl below.
#ifndef HMM355_FBR
#define HMM355_FBR 4  // posterior rows per follower wave per pass (follow.h)
#endif
#ifndef HMM355_FBF
#define HMM355_FBF 0  // diagnostic builds: posterior followers per sequence (0: the host's choice)
#endif
#ifndef HMM355_FABL
#define HMM355_FABL 0
#endif

namespace hmm355 {

constexpr int kWave = 64;
constexpr bool kStamp = HMM355_STAMP;

// In-kernel cycle stamp (diagnostic builds only, cdna guide §7): s_memtime with its
// lgkmcnt wait in ONE asm statement, fenced by sched_barrier on both sides.
__device__ __forceinline__ unsigned long long stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
template <typename T>
__device__ __forceinline__ void keep(T& v) { asm volatile("" : "+v"(v)); }
constexpr int kAbl = HMM355_ABL;
constexpr int kFAbl = HMM355_FABL;

// The bits of HMM355_ABL: one meaning each, tested as `kAbl & abl::kName`.  Every one of them
// gives wrong results: timing only.  The values 1, 2, 4, 8, 16 (tools/ablate.py) and 1, 1 << 20,
// 1 << 21 (tools/ablate_hsmm.py) are passed by number: keep them.  Free: bits 8..13.
namespace abl {
constexpr int kNoStepBarrier = 1;           // step_barrier(): rec_run_dpp / rec_run_rb, hsmm.hip, semimarkov.hip
constexpr int kDppNoProducts = 2;           // rec_run_dpp (NP = 256 only): sums / maxima of the inputs, no matrix
constexpr int kDppNoBlockWork = 4;          // rec_run_dpp (NP = 256 only): no staging, loads or flushes
constexpr int kPrepScanOnly = 8;            // band.h: the plan kernel stops after the matrix scan
constexpr int kNoPrep = 16;                 // band.h: the plan kernel returns at once
constexpr int kBandNoFlush = 32;            // rec_band helpers: no log-scale scan, no row flush
constexpr int kBandNoStage = 64;            // rec_band helpers: no emission staging, no loads
constexpr int kNoPsiRows = 128;             // rec_band, fused Viterbi: the psi waves compute nothing
constexpr int kBandNoBlockBarrier = 1 << 14;  // band_chain / rec_band: no barrier per 16-step block
constexpr int kBandNoHelperWork = 1 << 15;  // rec_band helpers: no block work at all
constexpr int kFbAlphaOnly = 1 << 16;       // fb_kern.h: the beta workgroups return at once
constexpr int kFbBetaOnly = 1 << 17;        // fb_kern.h: the alpha workgroups return at once
constexpr int kPostPlainStores = 1 << 18;   // post.h: plain instead of non-temporal output stores
constexpr int kHsmmForwardOnly = 1 << 19;   // hsmm.hip: no backtrace launches
constexpr int kHsmmNoPred = 1 << 20;        // hsmm.hip: no predecessor scores
constexpr int kHsmmNoSlots = 1 << 21;       // hsmm.hip: no slot work
constexpr int kStageNoLog = 1 << 22;        // rec_stage: OBS_PROB Viterbi staging takes no log
constexpr int kBandNoReduce = 1 << 23;      // band_chain: lane 0's value instead of the wave reduction
constexpr int kBandReducePrev = 1 << 24;    // band_chain, Viterbi: the previous step's reduction (off the chain)
constexpr int kPairNoScale = 1 << 25;       // fbpair.h: posteriors without the 1/s scaling
constexpr int kPairNoTasks = 1 << 26;       // fbpair.h: no row tasks
constexpr int kBandEmisReg = 1 << 27;       // band_chain: the block's first emission row in every step, no per-step LDS read
constexpr int kPairNoPostStores = 1 << 28;  // fbpair.h: no posterior stores
constexpr int kPairNoStores = 1 << 29;      // fbpair.h: no output, scratch or posterior stores
constexpr int kPairPlainStores = 1 << 30;   // fbpair.h: default cache policy instead of non-temporal
}  // namespace abl
// The bits of HMM355_FABL (`kFAbl & fabl::kName`); 2 and 4 are timing only.
namespace fabl {
constexpr int kNoBlockPublish = 1;  // rec_band: completion is published, the per-block counts are not
constexpr int kNoFollowers = 2;     // follow.h: followers and log leaders return at once
constexpr int kPlainStores = 4;     // rec_flush / psi copies: plain instead of write-through (sc1) stores
constexpr int kNoLogLeaders = 8;    // follow.h: the log leaders return at once
}  // namespace fabl

// compile-time loop: f(integral_constant<int, J>) for J in [B, E)
template <int J, int E, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (J < E) {
    f(std::integral_constant<int, J>{});
    static_for<J + 1, E>(f);
  }
}

// ---- DPP: row_newbcast:N — every lane of a 16-lane row receives lane N of that row. ----
template <int N>
__device__ __forceinline__ float row_bcast(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x150 + N, 0xF, 0xF, false));
}

// acc += row_bcast<N>(v) * m as ONE instruction (v_fmac_f32_dpp).  hipcc does not fold the
// DPP mov into v_fmac, so it is written out; the hazard recognizer still pads around it.
template <int N>
__device__ __forceinline__ void fmac_bcast(float& acc, float v, float m) {
  asm("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
      : "+v"(acc)
      : "v"(v), "v"(m), "n"(N));
}

// ---- cross-lane sums / maxima without LDS ----
// v_permlane16_swap / v_permlane32_swap written out: hipcc 7.2's
// __builtin_amdgcn_permlane{16,32}_swap reads the same register for both halves of the
// returned pair (miscompile observed at -O0 and -O3), so the pair is kept in two named
// VGPRs here.  "s_nop 1" covers the VALU-write -> permlane-read hazard inside the asm.
__device__ __forceinline__ void permlane16_swap(float& a, float& b) {
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void permlane32_swap(float& a, float& b) {
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void permlane16_swap_i(int& a, int& b) {
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void permlane32_swap_i(int& a, int& b) {
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

// sum over the four 16-lane rows of a wave (lanes c, c+16, c+32, c+48), result in every lane
__device__ __forceinline__ float rows_sum(float x) {
  float a = x, b = x;
  permlane16_swap(a, b);   // a = rows [0,0,2,2], b = rows [1,1,3,3]
  float y = a + b;
  float c = y, d = y;
  permlane32_swap(c, d);   // c = halves [0,0], d = halves [1,1]
  return c + d;
}

__device__ __forceinline__ float rows_max(float x) {
  float a = x, b = x;
  permlane16_swap(a, b);
  float y = fmaxf(a, b);
  float c = y, d = y;
  permlane32_swap(c, d);
  return fmaxf(c, d);
}

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float,
                            __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}

// sum over the 16 lanes of a row (all lanes of the row get the row sum)
__device__ __forceinline__ float row16_sum(float x) {
  x += dpp_f<0xB1>(x);   // quad_perm [1,0,3,2]
  x += dpp_f<0x4E>(x);   // quad_perm [2,3,0,1]
  x += dpp_f<0x124>(x);  // row_ror:4
  x += dpp_f<0x128>(x);  // row_ror:8
  return x;
}

// (value, index) argmax combine: larger value wins; equal values -> smaller index
__device__ __forceinline__ void argmax_combine(float& v, int& i, float v2, int i2) {
  // bitwise, not short-circuit: || / && here compile to exec-mask branches
  const bool take = (v2 > v) | ((v2 == v) & (i2 < i));
  v = take ? v2 : v;
  i = take ? i2 : i;
}

// full-wave (value, index) argmax via ds_bpermute-free shuffles (used off the hot loop)
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    float v2 = __shfl_xor(v, off);
    int i2 = __shfl_xor(i, off);
    argmax_combine(v, i, v2, i2);
  }
}

// full-wave (value, index) argmax on DPP + permlane swaps (no LDS round trips): the four
// in-row levels by quad_perm / row_ror, then the two cross-row levels by permlane16/32 swaps.
// Every lane ends with the wave's (max value, smallest index attaining it).
__device__ __forceinline__ void wave_argmax_dpp(float& v, int& i) {
  argmax_combine(v, i, dpp_f<0xB1>(v), dpp_i<0xB1>(i));
  argmax_combine(v, i, dpp_f<0x4E>(v), dpp_i<0x4E>(i));
  argmax_combine(v, i, dpp_f<0x124>(v), dpp_i<0x124>(i));
  argmax_combine(v, i, dpp_f<0x128>(v), dpp_i<0x128>(i));
  float a = v, b = v;
  int ia = i, ib = i;
  permlane16_swap(a, b);
  permlane16_swap_i(ia, ib);
  argmax_combine(a, ia, b, ib);
  float c = a, d = a;
  int ic = ia, id = ia;
  permlane32_swap(c, d);
  permlane32_swap_i(ic, id);
  argmax_combine(c, ic, d, id);
  v = c;
  i = ic;
}

// All-reduce over the `sub` lanes of a group (a power of two, aligned inside a wave), on DPP and
// permlane swaps: quad_perm [1,0,3,2] and [2,3,0,1], row_half_mirror, row_mirror, then the row
// pairs and the wave halves.  Every level pairs a lane with the lane that holds the other half's
// value, so a lane and its partner combine the same two numbers: the result has the same bits in
// every lane of the group.  (`sub` is uniform: the branches are scalar.)
template <typename Op>
__device__ __forceinline__ float grp_reduce(float v, int sub, Op op) {
  if (sub >= 2) v = op(v, dpp_f<0xB1>(v));
  if (sub >= 4) v = op(v, dpp_f<0x4E>(v));
  if (sub >= 8) v = op(v, dpp_f<0x141>(v));
  if (sub >= 16) v = op(v, dpp_f<0x140>(v));
  if (sub >= 32) {
    float a = v, b = v;
    permlane16_swap(a, b);  // a = rows [0,0,2,2], b = rows [1,1,3,3]
    v = op(a, b);
  }
  if (sub >= 64) {
    float a = v, b = v;
    permlane32_swap(a, b);
    v = op(a, b);
  }
  return v;
}
__device__ __forceinline__ float grp_max_rt(float v, int sub) {
  return grp_reduce(v, sub, [](float a, float b) { return fmaxf(a, b); });
}
__device__ __forceinline__ float grp_sum_rt(float v, int sub) {
  return grp_reduce(v, sub, [](float a, float b) { return a + b; });
}
// its (value, index) form: the larger value, of equal values the smaller index
__device__ __forceinline__ void grp_argmax_rt(float& v, int& i, int sub) {
  if (sub >= 2) argmax_combine(v, i, dpp_f<0xB1>(v), dpp_i<0xB1>(i));
  if (sub >= 4) argmax_combine(v, i, dpp_f<0x4E>(v), dpp_i<0x4E>(i));
  if (sub >= 8) argmax_combine(v, i, dpp_f<0x141>(v), dpp_i<0x141>(i));
  if (sub >= 16) argmax_combine(v, i, dpp_f<0x140>(v), dpp_i<0x140>(i));
  if (sub >= 32) {
    float a = v, b = v;
    int ia = i, ib = i;
    permlane16_swap(a, b);
    permlane16_swap_i(ia, ib);
    argmax_combine(a, ia, b, ib);
    v = a;
    i = ia;
  }
  if (sub >= 64) {
    float a = v, b = v;
    int ia = i, ib = i;
    permlane32_swap(a, b);
    permlane32_swap_i(ia, ib);
    argmax_combine(a, ia, b, ib);
    v = a;
    i = ia;
  }
}

// all-reduce over a compile-time SUB lanes (16: one DPP row; 8: half a row; 4: a quad)
template <int SUB>
__device__ __forceinline__ float grp_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));                       // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_f<0x4E>(v));                       // quad_perm [2,3,0,1]
  if constexpr (SUB == 8) v = fmaxf(v, dpp_f<0x141>(v));   // row_half_mirror
  if constexpr (SUB == 16) {
    v = fmaxf(v, dpp_f<0x124>(v));                    // row_ror:4
    v = fmaxf(v, dpp_f<0x128>(v));                    // row_ror:8
  }
  return v;
}
template <int SUB>
__device__ __forceinline__ int grp_min_i(int v) {
  v = min(v, dpp_i<0xB1>(v));
  v = min(v, dpp_i<0x4E>(v));
  if constexpr (SUB == 8) v = min(v, dpp_i<0x141>(v));
  if constexpr (SUB == 16) {
    v = min(v, dpp_i<0x124>(v));
    v = min(v, dpp_i<0x128>(v));
  }
  return v;
}

// Out of the fp32 range (hmm355.h, range contract) the chains can leave 0, denormals, inf and NaN
// in their rows and log-scales.  What is formed from them afterwards -- the row passes' posterior,
// forward and backward rows, the arc counts, the stored loglik -- must still be clean: a dead row
// is all zero, a dead sequence's loglik -inf.  The tests below are on the bits, not float
// compares: the library is built with -fno-honor-nans, under which a compare may be folded as
// if no operand were NaN, and the device keeps denormals, so 1 / x of a positive x can be inf.
__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
// 1 / x of a positive normal x (so finite, at most 2^126); 0 for 0, a denormal, a negative, inf or NaN
__device__ __forceinline__ bool normal_bits(float x) { return (__float_as_uint(x) - 0x00800000u) < 0x7f000000u; }
__device__ __forceinline__ float rcp_normal(float x) { return normal_bits(x) ? 1.f / x : 0.f; }
__device__ __forceinline__ float clean_loglik(float x) { return finite_bits(x) ? x : -INFINITY; }
// x where a row's factor `is` (rcp_normal of its sum) is alive and x is finite, else 0
__device__ __forceinline__ float row_value(float x, float is) {
  return (__float_as_uint(is) != 0u && finite_bits(x)) ? x : 0.f;
}

// all-lane wave sum / max on DPP + permlane swaps (no LDS round trips)
__device__ __forceinline__ float wave_sum_dpp(float x) { return rows_sum(row16_sum(x)); }
__device__ __forceinline__ float wave_max_dpp2(float x) {
  x = fmaxf(x, dpp_f<0xB1>(x));
  x = fmaxf(x, dpp_f<0x4E>(x));
  x = fmaxf(x, dpp_f<0x124>(x));
  x = fmaxf(x, dpp_f<0x128>(x));
  return rows_max(x);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

// workgroup reductions over NT threads through LDS (`red`: NT / 64 words): max of a float; min of
// an int
template <int NT>
__device__ __forceinline__ float wg_max(float v, float* red) {
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int k = 1; k < NT / 64; ++k) r = fmaxf(r, red[k]);
  return r;
}
template <int NT>
__device__ __forceinline__ int wg_min(int v, int* red) {
  for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
  for (int k = 1; k < NT / 64; ++k) r = min(r, red[k]);
  return r;
}

__device__ __forceinline__ int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// sequence b's length clamped to 1 .. T; no lengths: T
template <typename I>  // (the index as the caller holds it: int or size_t)
__device__ __forceinline__ int seq_len(const int* lengths, I b, int T) {
  if (!lengths) return T;
  return clamp_int(lengths[b], 1, T);
}

// log(e^a + e^b + e^c); -inf when all three are
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  const float ms = m == -INFINITY ? 0.f : m;
  const float s = expf(a - ms) + expf(b - ms) + expf(c - ms);
  const float r = ms + logf(s);
  return m == -INFINITY ? -INFINITY : r;
}
__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  const float ms = m == -INFINITY ? 0.f : m;
  const float s = expf(a - ms) + expf(b - ms);
  const float r = ms + logf(s);
  return m == -INFINITY ? -INFINITY : r;
}

// Correctly rounded fp32 log(x + 1e-8f): the sum is formed in fp32 exactly as the
// reference does (hmm.py:86), the log in fp64 then rounded once.  torch-CPU's logf agrees
// with the correctly rounded value on all but ~2.5e-5 of softmax-distributed inputs.
__device__ __forceinline__ float log_obs_cr(float x) {
  float s = x + 1e-8f;
  return (float)log((double)s);
}

// LDS barrier: waits for this wave's LDS ops, then s_barrier.  Global stores stay in flight
// (no vmcnt(0) per step); the "memory" clobber keeps the compiler from moving LDS accesses
// across it.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// the per-time-step barrier of the recursions (abl::kNoStepBarrier drops it: timing only)
__device__ __forceinline__ void step_barrier() {
  if constexpr (kAbl & abl::kNoStepBarrier)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  else
    lds_barrier();
}
// workgroup barrier that also waits for the workgroup's global stores: behind it every thread
// sees what any thread of the workgroup stored to memory before it
__device__ __forceinline__ void global_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __threadfence_block();
  __syncthreads();
}
// an L1-bypassing load (agent scope): rows that other waves of this workgroup wrote earlier
__device__ __forceinline__ float ld_fresh(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Allow a kernel more than the default 64 KiB of dynamic LDS (gfx950 has 160 KiB per CU).
template <typename K>
inline hipError_t allow_lds(K kernel, size_t bytes) {
  if (bytes <= 65536) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             static_cast<int>(bytes));
}

constexpr size_t kExclusiveLds = 160 * 1024;  // a workgroup that owns its CU

// ---- hand-offs between workgroups of one launch (MI355X_MICROARCH.md, inter-workgroup
// visibility; cdna_hip_programming.md Guideline 16, R1): payload stored write-through (sc1),
// every storing wave's stores complete before a workgroup barrier, then ONE lane stores the
// count (relaxed, agent scope: an sc1 store); the consumer polls the count relaxed and loads the
// payload with sc1 loads only (no L1 copy can be stale), so neither side needs a fence.
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
constexpr int kAuxSc1 = 16;  // buffer instruction cache-policy bits: sc1
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, size_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
// published counts sit one per 128-B line (no two counters share a line: a chain's store and
// another chain's follower polls never meet on one)
constexpr int kPubStride = 32;
// A count is one 8-byte word {call token, count ^ mix(token)}, stored and polled whole (8-B
// granules are untorn).  An eager call takes a fresh nonzero token (count_token()), so the
// words a previous call or any other use of the workspace left behind read as 0 -- no reset
// launch before the chains; a stale word passes only if its high half equals the token AND its
// low half decodes to a count <= cap.  Token 0 (calls captured into a HIP graph, whose replays
// share one token) keeps the reset kernel below before every launch.
__device__ __host__ __forceinline__ unsigned count_mix(unsigned token) { return token * 2654435761u; }
__device__ __forceinline__ int poll_count(const int* p, unsigned token, int cap) {
  const unsigned long long v =
      __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned c = (unsigned)v ^ count_mix(token);
  return ((unsigned)(v >> 32) == token && c <= (unsigned)cap) ? (int)c : 0;
}
__device__ __forceinline__ void publish_count(int* p, int v, unsigned token) {
  const unsigned long long w = ((unsigned long long)token << 32) | ((unsigned)v ^ count_mix(token));
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// a fresh nonzero token per eager call (process-wide, wraps past 0)
inline unsigned next_count_token() {
  static std::atomic<unsigned> g_token{0x5bd1e995u};
  unsigned t;
  do t = g_token.fetch_add(0x9e3779b9u, std::memory_order_relaxed) + 0x9e3779b9u; while (t == 0u);
  return t;
}
// true while `st` is being captured into a graph (its replays would share one token)
inline bool stream_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// Zeroes n 4-byte words (the followers' counters under token 0) as a kernel node: a
// hipMemsetAsync captured into a HIP graph was measured not to order against the chain launch
// that follows it in replay (the followers then saw the previous replay's final counts;
// tools/diag_graph.py)
static __global__ void zero_words_kernel(unsigned* p, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0u;
}
// (its launcher zero_words and prepare_counts: launch.h)

// The row maxima M_t = max_j lo_t[j] of log-emissions (B,T,N): one wave per (b,t) row,
// grid-stride.  A row without a finite maximum gets M = 0 (its emissions stay exp(lo)).  RAGGED:
// only frames t < seq_len(lengths, b, T) are read; a padded frame gets 0.
template <bool RAGGED>
__global__ void __launch_bounds__(256) row_max_kernel(const float* __restrict__ lo, const int* __restrict__ lengths,
                                                      int T, int N, size_t rows, float* __restrict__ m) {
  const int l = threadIdx.x & 63;
  const size_t nw = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t row = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; row < rows; row += nw) {
    bool valid = true;
    if constexpr (RAGGED) {
      const int b = (int)(row / T), t = (int)(row % T);
      valid = t < seq_len(lengths, b, T);
    }
    float v = -INFINITY;
    if (valid) {
      const float* src = lo + row * N;
      for (int j = l; j < N; j += 64) v = fmaxf(v, src[j]);
      v = wave_max_dpp2(v);
    }
    if (l == 0) m[row] = (v > -INFINITY && v < INFINITY) ? v : 0.f;
  }
}

inline int pad_states(int N) { return N <= 64 ? 64 : (N <= 128 ? 128 : 256); }

__host__ __device__ inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// The compact chain of adjoint.hip and ragged.hip: NP/32 waves; wave w owns outputs
// o = 32w + (lane & 31), the two half-waves split the inputs (lane >> 5 = input half h).
template <int NP>
struct ChainGeo {
  static constexpr int NW = NP / 32;     // waves
  static constexpr int NT = NW * kWave;  // threads
  static constexpr int HALF = NP / 2;    // inputs per lane
  static constexpr int XS = HALF + 4;    // LDS stride of an input half (the two half-wave
                                         // broadcast addresses fall in different banks)
  static constexpr int PD = 8;           // steps of loads in flight
  static constexpr int K = NP / 64;      // states per lane of a one-wave row pass
};

}  // namespace hmm355
