// hmm355 — posterior path sampling on gfx950: the backward-sampling pass of forward-filter
// backward-sample over the scaled forward rows the forward chains leave behind (U of
// hmm355_fb_workspace_layout).
//
// For sequence b, sample k and t = len - 1 .. 0 (hmm355.h has the full definition):
//     w[i] = fwd[b,t,i]                      at t = len - 1
//     w[i] = fwd[b,t,i] * A[i][z_{t+1}]      below it,            A = exp(log_P)
//     C    = the inclusive prefix sums of w, total = C[N-1], r = uniforms[b,k,t] * total
//     z_t  = the smallest i with C[i] > r
// One wave per (b,k) chain, four waves per workgroup (four samples of one sequence), blockIdx.y
// and a loop for the samples beyond them.  No wave waits on another (one barrier after the matrix
// is staged), no atomics, no flags: two calls on the same inputs return the same bits.
//
// A lane holds NP/64 consecutive entries (NP = N padded to 64/128/256).  A step is the lane's own
// prefix, a DPP wave scan of the lane totals (row_shr 1/2/4/8, row_bcast 15/31), wave_shr:1 for the
// exclusive lane offset, a ballot of "the lane's last prefix > r", and v_readlane of the winning
// lane's index: C[i] = E_lane + c_lane[i] is non-decreasing inside a lane and the first lane whose
// last prefix exceeds r holds the smallest i with C[i] > r.  The tree scan is not exactly monotone
// from one lane to the next, so that lane's first entry can have zero weight: the (rare,
// wave-uniform) fix-up moves the choice to the nearest positive weight at or below it, else above.
//
// On the dependency chain sit only the read of row z_{t+1} of A^T and the scan.  A^T =
// exp(log_P)^T (NP x NP, zero padded) is built once per call into the workspace, so that row is
// contiguous; for NP <= HMM355_FFBS_LDS_MAX_NP each workgroup stages it in LDS (64 KiB at NP = 128),
// above that the row comes from global memory (L2).  The fwd rows are loaded 8 steps ahead into a
// register ring; the uniforms of 64 steps are one coalesced load a chunk ahead (lane j keeps step
// j's, v_readlane hands it out), and the 64 drawn states of a chunk leave as one coalesced store.
// In the global form the row load is issued before the step's look-ahead loads, so its wait does
// not cover them (vmcnt counts in order).
#include "launch.h"

#ifndef HMM355_FFBS_LDS_MAX_NP
#define HMM355_FFBS_LDS_MAX_NP 128  // diagnostic builds (tools/time_ffbs.py): 0 reads A^T from global at every NP
#endif

namespace hmm355 {
namespace {

constexpr int kFfbsWaves = 4;   // samples (waves) per workgroup
constexpr int kFfbsPD = 8;      // steps of fwd rows in flight
constexpr int kFfbsChunk = 64;  // steps per uniform load / state store

// A^T, zero padded: AT[j * NP + i] = exp(log_P[i][j])
__global__ void __launch_bounds__(256) ffbs_at_kernel(const float* __restrict__ log_P, int N, int NP,
                                                      float* __restrict__ AT) {
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < NP * NP; idx += gridDim.x * 256) {
    const int j = idx / NP, i = idx % NP;
    AT[idx] = (i < N && j < N) ? expf(log_P[(size_t)i * N + j]) : 0.f;
  }
}

// x + (the DPP-moved x, 0 where the source lane is outside the row or the row is masked)
template <int CTRL, int ROWS>
__device__ __forceinline__ float dpp_add0(float x) {
  return x + __builtin_bit_cast(float,
                                __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, ROWS, 0xF, false));
}
// inclusive prefix sum over the 64 lanes
__device__ __forceinline__ float wave_scan_incl(float x) {
  x = dpp_add0<0x111, 0xF>(x);  // row_shr:1
  x = dpp_add0<0x112, 0xF>(x);  // row_shr:2
  x = dpp_add0<0x114, 0xF>(x);  // row_shr:4
  x = dpp_add0<0x118, 0xF>(x);  // row_shr:8
  x = dpp_add0<0x142, 0xA>(x);  // row_bcast:15 into rows 1 and 3
  x = dpp_add0<0x143, 0xC>(x);  // row_bcast:31 into rows 2 and 3
  return x;
}
// lane l receives lane l - 1's value, lane 0 receives 0
__device__ __forceinline__ float wave_shr1(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x138, 0xF, 0xF, false));
}
__device__ __forceinline__ float readlane_f(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

struct FfbsArgs {
  const float* fwd;      // (B,T) rows of ld floats
  const float* AT;       // (NP,NP) workspace
  const int* lengths;    // (B) or null
  const float* uniforms; // (B,K,T)
  int64_t* states;       // (B,K,T)
  int ld, B, T, N, K;
};

template <int NP, bool LDS>
__global__ void __launch_bounds__(kFfbsWaves * kWave) ffbs_kernel(FfbsArgs a) {
  constexpr int K4 = NP / 64;  // entries per lane
  constexpr int PD = kFfbsPD;
  extern __shared__ __attribute__((aligned(16))) float at_lds[];
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  if constexpr (LDS) {
    const float4* src = reinterpret_cast<const float4*>(a.AT);
    float4* dst = reinterpret_cast<float4*>(at_lds);
    for (int i = tid; i < NP * NP / 4; i += kFfbsWaves * kWave) dst[i] = src[i];
    __syncthreads();
  }
  const float* at = LDS ? at_lds : a.AT;
  const int T = a.T, N = a.N;
  int len = T;
  if (a.lengths) {
    const int n = a.lengths[b];
    len = n < 1 ? 1 : (n > T ? T : n);
  }
  const int last_lane = (N - 1) / K4;  // the lane of entry N - 1
  const unsigned long long lanes = last_lane == 63 ? ~0ull : ((1ull << (last_lane + 1)) - 1ull);
  const float* frow = a.fwd + (size_t)b * T * a.ld + l * K4;

  for (int k = blockIdx.y * kFfbsWaves + w; k < a.K; k += gridDim.y * kFfbsWaves) {
    const float* urow = a.uniforms + ((size_t)b * a.K + k) * T;
    int64_t* srow = a.states + ((size_t)b * a.K + k) * T;
    // step q draws frame len - 1 - q; a step past the end re-loads frame 0 (never a padded frame)
    float rf[PD][K4];
    auto load = [&](int q, auto PP) {
      constexpr int p = decltype(PP)::value;
      const int t = len - 1 - q;
      const float* src = frow + (size_t)(t > 0 ? t : 0) * a.ld;
#pragma unroll
      for (int kk = 0; kk < K4; ++kk) rf[p][kk] = (l * K4 + kk < N) ? src[kk] : 0.f;
    };
    auto load_u = [&](int c0) {  // lane j: the uniform of step c0 + j
      const int t = len - 1 - (c0 + l);
      return urow[t > 0 ? t : 0];
    };
    static_for<0, PD>([&](auto PP) { load(PP.value, PP); });
    float u_next = load_u(0);

    int z = -1;   // the state of frame t + 1 (none yet)
    int zs = 0;   // lane j: the state drawn at step c0 + j of the chunk
    float u_cur = 0.f;
    auto step = [&](int q, auto PP, auto LOAD) {
      constexpr int p = decltype(PP)::value;
      float f[K4], wv[K4];
#pragma unroll
      for (int kk = 0; kk < K4; ++kk) f[kk] = rf[p][kk];
      if (z >= 0) {
        const float* row = at + z * NP + l * K4;
        if constexpr (K4 == 1) {
          wv[0] = row[0];
        } else if constexpr (K4 == 2) {
          const float2 r2 = *reinterpret_cast<const float2*>(row);
          wv[0] = r2.x;
          wv[1] = r2.y;
        } else {
          const float4 r4 = *reinterpret_cast<const float4*>(row);
          wv[0] = r4.x;
          wv[1] = r4.y;
          wv[2] = r4.z;
          wv[3] = r4.w;
        }
        if constexpr (!LDS) __builtin_amdgcn_sched_barrier(0);  // the row load leaves before the look-ahead loads
      } else {
#pragma unroll
        for (int kk = 0; kk < K4; ++kk) wv[kk] = 1.f;
      }
      if constexpr (decltype(LOAD)::value) load(q + PD, PP);
      const float u = readlane_f(u_cur, q & (kFfbsChunk - 1));
      float c[K4];
#pragma unroll
      for (int kk = 0; kk < K4; ++kk) {
        wv[kk] *= f[kk];
        c[kk] = kk == 0 ? wv[0] : c[kk - 1] + wv[kk];
      }
      const float e = wave_shr1(wave_scan_incl(c[K4 - 1]));  // the sum of the lanes below
      const float top = e + c[K4 - 1];
      const float total = readlane_f(top, last_lane);        // C[N-1]
      int zn;
      if (total > 0.f && total < INFINITY) {
        const float r = u * total;
        const unsigned long long m = __ballot(top > r) & lanes;
        // the lane's first entry whose prefix exceeds r (its prefixes are non-decreasing)
        int cnt = 0;
#pragma unroll
        for (int kk = 0; kk < K4 - 1; ++kk) cnt += (e + c[kk] > r) ? 0 : 1;
        float wz = wv[0];
#pragma unroll
        for (int kk = 1; kk < K4; ++kk) wz = cnt == kk ? wv[kk] : wz;
        const int zi = l * K4 + cnt;
        const int src_lane = m ? (int)__builtin_ctzll(m) : last_lane;
        zn = __builtin_amdgcn_readlane(zi, src_lane);
        const int ok = __builtin_amdgcn_readlane((wz > 0.f && zi < N) ? 1 : 0, src_lane);
        if (!m || !ok) {
          // no prefix above r (u * total rounded up to total): the largest positive weight; a
          // zero-weight landing: the nearest positive weight at or below it, else above it
          const int pivot = m ? zn : N - 1;
          int lo = -1, hi = -1;
#pragma unroll
          for (int kk = 0; kk < K4; ++kk) {
            const int i = l * K4 + kk;
            const bool pos = wv[kk] > 0.f;
            lo = (pos && i <= pivot) ? i : lo;
            hi = (pos && i > pivot && hi < 0) ? i : hi;
          }
          const unsigned long long mb = __ballot(lo >= 0);
          const unsigned long long ma = __ballot(hi >= 0);
          if (mb) zn = __builtin_amdgcn_readlane(lo, 63 - (int)__builtin_clzll(mb));
          else if (ma) zn = __builtin_amdgcn_readlane(hi, (int)__builtin_ctzll(ma));
          else zn = pivot;
        }
      } else {
        // a row without a positive finite total: the first index maximising fwd[b,t,.]
        float bv = (l * K4 < N) ? f[0] : -INFINITY;
        int bi = l * K4;
#pragma unroll
        for (int kk = 1; kk < K4; ++kk) {
          const bool tk = (l * K4 + kk < N) & (f[kk] > bv);
          bv = tk ? f[kk] : bv;
          bi = tk ? l * K4 + kk : bi;
        }
        wave_argmax_dpp(bv, bi);
        zn = __builtin_amdgcn_readfirstlane(bi);
      }
      zn = zn < 0 ? 0 : (zn > N - 1 ? N - 1 : zn);
      z = zn;
      zs = (l == (q & (kFfbsChunk - 1))) ? zn : zs;
    };

    for (int c0 = 0; c0 < len; c0 += kFfbsChunk) {
      u_cur = u_next;
      u_next = load_u(c0 + kFfbsChunk);
      const int n = len - c0 < kFfbsChunk ? len - c0 : kFfbsChunk;
      // whole blocks of PD steps without a branch between a load and its use, then the last < PD
      // steps, whose rows are in the ring already (ragged.hip's form)
      int qb = 0;
      for (; qb + PD <= n; qb += PD)
        static_for<0, PD>([&](auto PP) { step(c0 + qb + PP.value, PP, std::true_type{}); });
      static_for<0, PD>([&](auto PP) {
        if (qb + PP.value < n) step(c0 + qb + PP.value, PP, std::false_type{});
      });
      if (l < n) srow[len - 1 - (c0 + l)] = zs;
    }
    for (int t = len + l; t < T; t += kWave) srow[t] = -1;  // padded frames
  }
}

size_t ffbs_ws(int N) {
  const int NP = pad_states(N);
  return (size_t)NP * NP * sizeof(float);
}

template <int NP, bool LDS>
hipError_t ffbs_launch(const FfbsArgs& a, dim3 grid, hipStream_t st) {
  const size_t lds = LDS ? (size_t)NP * NP * sizeof(float) : 0;
  return launch(ffbs_kernel<NP, LDS>, grid, dim3(kFfbsWaves * kWave), lds, st, a);
}

}  // namespace
}  // namespace hmm355

using namespace hmm355;

HMM355_API size_t hmm355_ffbs_workspace_bytes(int N) {
  if (N < 1 || N > 256) return 0;
  return ffbs_ws(N);
}

HMM355_API int hmm355_ffbs_f32(const float* fwd, int ld, const float* log_P, const int* lengths,
                               const float* uniforms, int B, int T, int N, int K, int64_t* states, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (B < 0 || N < 0) return HMM355_E_ARG;
  if (N < 1 || N > 256) return HMM355_E_STATES;
  if (T < 1 || K < 1) return HMM355_E_SHAPE;
  if (B == 0) return HMM355_OK;
  if (!fwd || !log_P || !uniforms || !states || !workspace) return HMM355_E_ARG;
  if (ld < N) return HMM355_E_ARG;
  if ((size_t)B * T > (size_t)1 << 40 || (size_t)K > ((size_t)1 << 40) / ((size_t)B * T)) return HMM355_E_SHAPE;
  if (workspace_bytes < ffbs_ws(N)) return HMM355_E_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int NP = pad_states(N);
  float* AT = static_cast<float*>(workspace);
  HMM355_TRY(launch(ffbs_at_kernel, dim3(NP * NP / 256), dim3(256), 0, st, log_P, N, NP, AT));
  // samples over blockIdx.y while the grid stays near 2048 workgroups (at least 8 per sequence), a
  // loop in the kernel beyond that
  int gy = (K + kFfbsWaves - 1) / kFfbsWaves;
  const int cap = 2048 / B > 8 ? 2048 / B : 8;
  gy = gy < cap ? gy : cap;
  const dim3 grid((unsigned)B, (unsigned)gy);
  FfbsArgs a{fwd, AT, lengths, uniforms, states, ld, B, T, N, K};
  const bool lds = NP <= HMM355_FFBS_LDS_MAX_NP;
  switch (NP) {  // (no LDS form at NP = 256: not with_np)
    case 64: return lds ? ffbs_launch<64, true>(a, grid, st) : ffbs_launch<64, false>(a, grid, st);
    case 128: return lds ? ffbs_launch<128, true>(a, grid, st) : ffbs_launch<128, false>(a, grid, st);
    default: return ffbs_launch<256, false>(a, grid, st);
  }
}
