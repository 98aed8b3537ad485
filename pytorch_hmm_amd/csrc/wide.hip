// hmm355 — batch-tiled forward-backward and Viterbi for 1 <= N <= 4096 states (the "wide" form).
//
// The chains of fb.hip / viterbi.hip keep the whole N x N matrix beside one CU and run one
// workgroup per sequence, which stops at N = 256.  Here the B sequences of a call share log_P,
// so one time step of the whole batch is a (B x N) . (N x N) product (max-plus for Viterbi),
// tiled over 64 output columns and kBT sequences per workgroup:
//   - lanes run over the output column j, so row i of the matrix is one coalesced 256-B segment;
//   - the eight waves split the input range i into ascending slices and combine through LDS;
//   - the previous step's rows of the batch tile are staged in LDS and read as wave-uniform
//     broadcasts (16 B per read);
//   - every matrix element a workgroup loads is used for kBT sequences.
// Consecutive time steps are separate launches: stream order is the only dependency between
// steps.  No kernel here waits on another workgroup, uses an atomic or a flag, and every kernel
// is complete on its own.
//
// Tile choice: 64 columns x kBT = 2 sequences.  N = 1024, B = 32 gives 16 x 16 = 256 workgroups
// per Viterbi step (one per CU) and 512 per forward-backward step (both directions in one
// launch); N = 512, B = 32 gives 128 / 256.  A larger batch tile halves the matrix traffic per
// step but leaves CUs idle at these sizes.
//
// Viterbi: delta_t[b][j] = max_i(delta_{t-1}[b][i] + log_P[i][j]) + lo_t[b][j], one fp32 add of
// an exact max, so delta and the path are bit-identical to the reference's (hmm.py:164-168,
// first index on ties).  psi is uint16 in the workspace; one backtrace kernel ends the call.
//
// Forward-backward: the scaled probability-domain recursion of fb.hip with a deferred
// normaliser.  A step stores its raw row; the next step's workgroups form that row's sum s while
// they stage it (same code, same order, so the same bits in every workgroup) and use row / s;
// column tile 0 stores s.  A = exp(log_P) and its transpose are written once per call, so the
// backward step reads coalesced rows too and one step kernel serves both directions
// (blockIdx.z).  An epilogue accumulates the log-scales per sequence in fp64 and forms
// posterior / forward / backward / loglik / lik_ref in one pass over (B,T,N).
#include "launch.h"
#include "logcr.h"

namespace hmm355 {
namespace {

constexpr int kWideMaxN = 4096;
constexpr int kColTile = 64;  // output columns per workgroup (one per lane)
constexpr int kBT = 2;        // sequences per workgroup
constexpr int kWaves = 8;     // input slices per workgroup of a step kernel (one per wave)
constexpr int kStepThreads = kWaves * 64;

// input slice of one wave: ceil(N / kWaves) rounded up to 4 (slices start 16-B aligned in LDS)
__host__ __device__ inline int wide_slice(int N) { return (((N + kWaves - 1) / kWaves) + 3) & ~3; }

// OBS_PROB emissions of a decode: log(x + 1e-8) correctly rounded (logcr.h), the bits of
// viterbi.hip's vit_log_obs_kernel
__global__ void __launch_bounds__(256) wide_log_obs_kernel(const float* __restrict__ x, float* __restrict__ lo, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    lo[i] = logcr_fast(x[i] + 1e-8f, g_logcr_tab);
}

// ------------------------------------------------------------------------------ Viterbi
struct WVitArgs {
  const float* lo;     // (B,T,N) log-emissions
  const float* log_P;  // (N,N)
  float* delta;        // (B,T,N) the caller's trellis
  uint16_t* psi;       // (B,T,N) workspace
  int B, T, N;
};

// delta_0 = init + lo_0
__global__ void __launch_bounds__(256) wide_vit_init_kernel(WVitArgs a, const float* __restrict__ init) {
  const size_t n = (size_t)a.B * a.N;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const size_t b = e / a.N, j = e % a.N;
    const size_t off = b * a.T * a.N + j;
    a.delta[off] = init[j] + a.lo[off];
  }
}

__global__ void __launch_bounds__(kStepThreads) wide_vit_step_kernel(WVitArgs a, int t) {
  __shared__ __attribute__((aligned(16))) float dl[kBT][kWideMaxN];
  __shared__ float pv[kWaves][kBT][kColTile];
  __shared__ int pi[kWaves][kBT][kColTile];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int N = a.N;
  const size_t T = a.T;
  const size_t b0 = (size_t)blockIdx.y * kBT;
  const int j = blockIdx.x * kColTile + l;
  const int jc = j < N ? j : N - 1;
  // stage delta_{t-1} of the batch tile (a tile row past B re-reads the last sequence: computed, not stored)
#pragma unroll
  for (int bb = 0; bb < kBT; ++bb) {
    const size_t b = b0 + bb < (size_t)a.B ? b0 + bb : (size_t)a.B - 1;
    const float* src = a.delta + (b * T + (size_t)(t - 1)) * N;
    for (int i = tid; i < N; i += kStepThreads) dl[bb][i] = src[i];
  }
  __syncthreads();
  const int S = wide_slice(N);
  const int i0 = w * S;
  const int i1 = i0 + S < N ? i0 + S : N;
  float best[kBT];
  int arg[kBT];
#pragma unroll
  for (int bb = 0; bb < kBT; ++bb) {
    best[bb] = -INFINITY;
    arg[bb] = 0x7fffffff;  // an empty slice: loses every combine
  }
  if (i0 < i1) {
    const float* pc = a.log_P + jc;
    auto one = [&](int i) {
      const float p = pc[(size_t)i * N];
#pragma unroll
      for (int bb = 0; bb < kBT; ++bb) {
        const float v = dl[bb][i] + p;
        const bool tk = v > best[bb];
        best[bb] = tk ? v : best[bb];
        arg[bb] = tk ? i : arg[bb];
      }
    };
    {  // the slice's first candidate is real: best starts from it (-inf columns keep index i0)
      const float p = pc[(size_t)i0 * N];
#pragma unroll
      for (int bb = 0; bb < kBT; ++bb) {
        best[bb] = dl[bb][i0] + p;
        arg[bb] = i0;
      }
    }
    int i = i0 + 1;
    const int ih = i0 + 4 < i1 ? i0 + 4 : i1;
    for (; i < ih; ++i) one(i);
#pragma unroll 4
    for (; i + 4 <= i1; i += 4) {
      const float* pr = pc + (size_t)i * N;
      const float p[4] = {pr[0], pr[(size_t)N], pr[2 * (size_t)N], pr[3 * (size_t)N]};
#pragma unroll
      for (int bb = 0; bb < kBT; ++bb) {
        const float4 d4 = *reinterpret_cast<const float4*>(&dl[bb][i]);
        const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // strict > in ascending i: the first maximum wins
          const float v = d[k] + p[k];
          const bool tk = v > best[bb];
          best[bb] = tk ? v : best[bb];
          arg[bb] = tk ? i + k : arg[bb];
        }
      }
    }
    for (; i < i1; ++i) one(i);
  }
#pragma unroll
  for (int bb = 0; bb < kBT; ++bb) {
    pv[w][bb][l] = best[bb];
    pi[w][bb][l] = arg[bb];
  }
  __syncthreads();
  if (tid < kBT * kColTile) {
    const int bb = tid >> 6;
    float v = pv[0][bb][l];
    int ix = pi[0][bb][l];
#pragma unroll
    for (int ww = 1; ww < kWaves; ++ww) argmax_combine(v, ix, pv[ww][bb][l], pi[ww][bb][l]);
    const size_t b = b0 + bb;
    if (j < N && b < (size_t)a.B) {
      const size_t off = (b * T + (size_t)t) * N + j;
      a.delta[off] = v + a.lo[off];
      a.psi[off] = (uint16_t)ix;
    }
  }
}

// One workgroup per sequence: first argmax of delta_{T-1} (hmm.py:174), then the T-step walk
// (hmm.py:177-178) by one lane over psi rows staged in LDS, kPsiLds entries at a time.
constexpr int kPsiLds = 16384;

__global__ void __launch_bounds__(256) wide_backtrace_kernel(WVitArgs a, int64_t* __restrict__ states,
                                                             float* __restrict__ final_score) {
  __shared__ __attribute__((aligned(16))) uint16_t ps[kPsiLds];
  __shared__ float rv[4];
  __shared__ int ri[4];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int N = a.N, T = a.T;
  const size_t b = blockIdx.x;
  const float* dl = a.delta + (b * T + (size_t)(T - 1)) * N;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int j = tid; j < N; j += 256) argmax_combine(bv, bi, dl[j], j);
  wave_argmax(bv, bi);
  if (l == 0) {
    rv[w] = bv;
    ri[w] = bi;
  }
  __syncthreads();
  int s = 0;
  if (tid == 0) {
    bv = rv[0];
    bi = ri[0];
    for (int ww = 1; ww < 4; ++ww) argmax_combine(bv, bi, rv[ww], ri[ww]);
    if (final_score) final_score[b] = bv;
    s = bi;
  }
  const int R = kPsiLds / N;  // psi rows per pass (>= 4)
  for (int t_hi = T - 1; t_hi >= 1; t_hi -= R) {
    const int t_lo = t_hi - R + 1 > 1 ? t_hi - R + 1 : 1;
    const size_t cnt = (size_t)(t_hi - t_lo + 1) * N;
    const uint16_t* src = a.psi + (b * T + (size_t)t_lo) * N;
    __syncthreads();  // the previous pass's walk is done with ps
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      const size_t n8 = cnt / 8;
      for (size_t q = tid; q < n8; q += 256) reinterpret_cast<uint4*>(ps)[q] = reinterpret_cast<const uint4*>(src)[q];
      for (size_t q = 8 * n8 + tid; q < cnt; q += 256) ps[q] = src[q];
    } else {
      for (size_t q = tid; q < cnt; q += 256) ps[q] = src[q];
    }
    __syncthreads();
    if (tid == 0) {
      for (int t = t_hi; t >= t_lo; --t) {
        states[b * T + t] = s;
        s = ps[(size_t)(t - t_lo) * N + s];
      }
    }
  }
  if (tid == 0) states[b * T] = s;
}

// --------------------------------------------------------------------- forward-backward
struct WFbArgs {
  const float* obs;  // (B,T,N) emissions, encoding obs_mode
  const float* M;    // (B,T) row maxima of the log-emissions (OBS_LOG), else unused
  const float* A;    // (N,N) exp(log_P)
  const float* AT;   // (N,N) its transpose
  float* U;          // (B,T,N) raw alpha rows
  float* V;          // (B,T,N) raw beta rows
  float* SA;         // (B,T) SA[t] = sum_j U_t[j]
  float* SB;         // (B,T) SB[t] = sum_j e_t[j] V_t[j]
  int B, T, N, obs_mode;
};

// e_t[j]: x + 1e-8 (OBS_PROB, hmm.py:86) or exp(lo - M_t) (OBS_LOG, include/hmm355.h)
__device__ __forceinline__ float wide_emis(const WFbArgs& a, size_t row, int j) {
  const float x = a.obs[row * a.N + j];
  return a.obs_mode == HMM355_OBS_PROB ? x + 1e-8f : expf(x - a.M[row]);
}

// A = exp(log_P) and its transpose
__global__ void __launch_bounds__(256) wide_exp_matrix_kernel(const float* __restrict__ log_P, int N, float* __restrict__ A,
                                                              float* __restrict__ AT) {
  const size_t n = (size_t)N * N;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const size_t i = e / N, j = e % N;
    const float v = expf(log_P[e]);
    A[e] = v;
    AT[j * N + i] = v;
  }
}

// U_0 = exp(log_p0) e_0;  V_{T-1} = 1
__global__ void __launch_bounds__(256) wide_fb_init_kernel(WFbArgs a, const float* __restrict__ log_p0) {
  const size_t n = (size_t)a.B * a.N;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t T = a.T;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const size_t b = e / a.N;
    const int j = (int)(e % a.N);
    a.U[b * T * a.N + j] = expf(log_p0[j]) * wide_emis(a, b * T, j);
    a.V[(b * T + T - 1) * a.N + j] = 1.f;
  }
}

// Launch k = 1..T-1.  blockIdx.z = 0: alpha row k from row k-1,
//   U_k[j] = (sum_i (U_{k-1}[i] / SA_{k-1}) A[i][j]) e_k[j];
// blockIdx.z = 1: beta row T-1-k from row T-k,
//   V_{t-1}[i] = sum_j AT[j][i] (e_t[j] V_t[j] / SB_t),  t = T-k.
__global__ void __launch_bounds__(kStepThreads) wide_fb_step_kernel(WFbArgs a, int k) {
  __shared__ __attribute__((aligned(16))) float xs[kBT][kWideMaxN];
  __shared__ float pa[kWaves][kBT][kColTile];
  __shared__ float wsum[kBT][kWaves];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int N = a.N;
  const size_t T = a.T;
  const int dir = blockIdx.z;
  const size_t tin = dir ? T - (size_t)k : (size_t)k - 1;
  const size_t tout = dir ? tin - 1 : tin + 1;
  const float* in = dir ? a.V : a.U;
  float* out = dir ? a.V : a.U;
  const float* mat = dir ? a.AT : a.A;
  const size_t b0 = (size_t)blockIdx.y * kBT;
  const int j = blockIdx.x * kColTile + l;
  const int jc = j < N ? j : N - 1;
  // stage the input rows and form their sums: per-lane partials in ascending i, the wave's
  // lanes, then the waves in order -- the same operations in every workgroup
  float part[kBT];
#pragma unroll
  for (int bb = 0; bb < kBT; ++bb) {
    const size_t b = b0 + bb < (size_t)a.B ? b0 + bb : (size_t)a.B - 1;
    const size_t row = b * T + tin;
    float s = 0.f;
    for (int i = tid; i < N; i += kStepThreads) {
      float x = in[row * N + i];
      if (dir) x *= wide_emis(a, row, i);
      xs[bb][i] = x;
      s += x;
    }
    part[bb] = wave_sum_dpp(s);
  }
  if (l == 0) {
#pragma unroll
    for (int bb = 0; bb < kBT; ++bb) wsum[bb][w] = part[bb];
  }
  __syncthreads();
#pragma unroll
  for (int bb = 0; bb < kBT; ++bb) {
    float s = wsum[bb][0];
#pragma unroll
    for (int ww = 1; ww < kWaves; ++ww) s += wsum[bb][ww];
    for (int i = tid; i < N; i += kStepThreads) xs[bb][i] = s > 0.f ? xs[bb][i] / s : 0.f;  // (this lane's own entries)
    if (blockIdx.x == 0 && tid == 0 && b0 + bb < (size_t)a.B) (dir ? a.SB : a.SA)[(b0 + bb) * T + tin] = s;
  }
  __syncthreads();
  const int S = wide_slice(N);
  const int i0 = w * S;
  const int i1 = i0 + S < N ? i0 + S : N;
  float acc[kBT];
#pragma unroll
  for (int bb = 0; bb < kBT; ++bb) acc[bb] = 0.f;
  {
    const float* pc = mat + jc;
    int i = i0;
#pragma unroll 4
    for (; i + 4 <= i1; i += 4) {
      const float* pr = pc + (size_t)i * N;
      const float p[4] = {pr[0], pr[(size_t)N], pr[2 * (size_t)N], pr[3 * (size_t)N]};
#pragma unroll
      for (int bb = 0; bb < kBT; ++bb) {
        const float4 d4 = *reinterpret_cast<const float4*>(&xs[bb][i]);
        acc[bb] = fmaf(d4.x, p[0], acc[bb]);
        acc[bb] = fmaf(d4.y, p[1], acc[bb]);
        acc[bb] = fmaf(d4.z, p[2], acc[bb]);
        acc[bb] = fmaf(d4.w, p[3], acc[bb]);
      }
    }
    for (; i < i1; ++i) {
      const float p = pc[(size_t)i * N];
#pragma unroll
      for (int bb = 0; bb < kBT; ++bb) acc[bb] = fmaf(xs[bb][i], p, acc[bb]);
    }
  }
#pragma unroll
  for (int bb = 0; bb < kBT; ++bb) pa[w][bb][l] = acc[bb];
  __syncthreads();
  if (tid < kBT * kColTile) {
    const int bb = tid >> 6;
    const size_t b = b0 + bb;
    if (j < N && b < (size_t)a.B) {
      float v = pa[0][bb][l];
#pragma unroll
      for (int ww = 1; ww < kWaves; ++ww) v += pa[ww][bb][l];  // the slices in ascending order
      const size_t row = b * T + tout;
      if (!dir) v *= wide_emis(a, row, j);
      out[row * N + j] = v;
    }
  }
}

// One workgroup per sequence: the cumulative log-scales in fp64 (T adds per direction),
//   CLA[t] = sum_{k<t} log SA[k] + sum_{k<=t} M_k     log alpha_t = log U_t + CLA[t]
//   CLB[t] = sum_{k>t} (log SB[k] + M_k)               log beta_t  = log V_t + CLB[t]
// and loglik = CLA[T-1] + log sum_j U_{T-1}[j].  The logs are formed by all lanes into LDS,
// 1024 steps at a time; lane 0 adds the alpha terms and lane 64 the beta terms in time order.
constexpr int kScanChunk = 1024;

__global__ void __launch_bounds__(256) wide_scan_kernel(WFbArgs a, double* __restrict__ CLA, double* __restrict__ CLB,
                                                        float* __restrict__ loglik) {
  __shared__ double buf[2][kScanChunk];
  __shared__ float wsum[4];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int N = a.N, T = a.T;
  const size_t r0 = (size_t)blockIdx.x * T;
  const bool shifted = a.obs_mode == HMM355_OBS_LOG;
  float part = 0.f;
  {
    const float* u = a.U + (r0 + (size_t)(T - 1)) * N;
    for (int j = tid; j < N; j += 256) part += u[j];
  }
  part = wave_sum_dpp(part);
  if (l == 0) wsum[w] = part;
  __syncthreads();
  const float s_last = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  double ca = 0.0, cb = 0.0;
  for (int c0 = 0; c0 < T; c0 += kScanChunk) {
    const int n = T - c0 < kScanChunk ? T - c0 : kScanChunk;
    for (int q = tid; q < n; q += 256) {
      const int t = c0 + q;  // alpha term of time t; beta term of time T-1-t
      double va = shifted ? (double)a.M[r0 + t] : 0.0;
      if (t > 0) va += log((double)a.SA[r0 + t - 1]);
      double vb = 0.0;
      if (t > 0) vb = log((double)a.SB[r0 + T - t]) + (shifted ? (double)a.M[r0 + T - t] : 0.0);
      buf[0][q] = va;
      buf[1][q] = vb;
    }
    __syncthreads();
    if (tid == 0) {
      for (int q = 0; q < n; ++q) {
        ca += buf[0][q];
        CLA[r0 + c0 + q] = ca;
      }
    } else if (tid == 64) {
      for (int q = 0; q < n; ++q) {
        cb += buf[1][q];
        CLB[r0 + T - 1 - (c0 + q)] = cb;
      }
    }
    __syncthreads();
  }
  if (tid == 0 && loglik) loglik[blockIdx.x] = clean_loglik((float)(ca + log((double)s_last)));
}

// One wave per (b,t) row, grid-stride: posterior = U V / sum(U V) (scale-invariant; each row
// scaled by its maximum first), forward = exp(log U + CLA), backward = exp(log V + CLB)
// (underflowing to 0 as the reference's do), and for the last row the reference's
// compute_likelihood value logsumexp_j(log(forward_{T-1}[j] + 1e-8)) (hmm.py:206).
__global__ void __launch_bounds__(256) wide_post_kernel(WFbArgs a, const double* __restrict__ CLA,
                                                        const double* __restrict__ CLB, unsigned mask,
                                                        float* __restrict__ posterior, float* __restrict__ forward,
                                                        float* __restrict__ backward, float* __restrict__ lik_ref) {
  const int l = threadIdx.x & 63;
  const int N = a.N;
  const size_t T = a.T;
  // a likelihood-only call (no output bit) visits the last row of each sequence alone
  const size_t visits = mask ? (size_t)a.B * T : (size_t)a.B;
  const size_t nw = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t r = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < visits; r += nw) {
    const size_t row = mask ? r : r * T + T - 1;
    const bool last = row % T == T - 1;
    const float* u = a.U + row * N;
    const float* v = a.V + row * N;
    const double cla = CLA[row], clb = CLB[row];
    if (mask & HMM355_FB_POSTERIOR) {
      float mu = 0.f, mv = 0.f;
      for (int j = l; j < N; j += 64) {
        mu = fmaxf(mu, u[j]);
        mv = fmaxf(mv, v[j]);
      }
      mu = wave_max_dpp2(mu);
      mv = wave_max_dpp2(mv);
      const float iu = rcp_normal(mu), iv = rcp_normal(mv);  // (common.h: a dead row is all zero)
      float s = 0.f;
      for (int j = l; j < N; j += 64) s += (u[j] * iu) * (v[j] * iv);
      s = wave_sum_dpp(s);
      const float is = rcp_normal(s);
      for (int j = l; j < N; j += 64) posterior[row * N + j] = row_value((u[j] * iu) * (v[j] * iv) * is, is);
    }
    if (mask & HMM355_FB_FORWARD)
      for (int j = l; j < N; j += 64) forward[row * N + j] = row_value(__expf((float)((double)__logf(u[j]) + cla)), 1.f);
    if (mask & HMM355_FB_BACKWARD)
      for (int j = l; j < N; j += 64) backward[row * N + j] = row_value(__expf((float)((double)__logf(v[j]) + clb)), 1.f);
    if (last && lik_ref) {
      float m = -INFINITY;
      for (int j = l; j < N; j += 64) m = fmaxf(m, __logf(__expf((float)((double)__logf(u[j]) + cla)) + 1e-8f));
      m = wave_max_dpp2(m);
      float e = 0.f;
      for (int j = l; j < N; j += 64) e += __expf(__logf(__expf((float)((double)__logf(u[j]) + cla)) + 1e-8f) - m);
      e = wave_sum_dpp(e);
      if (l == 0) lik_ref[row / T] = m + __logf(e);
    }
  }
}

inline unsigned stride_blocks(size_t n, size_t cap) {
  size_t blocks = (n + 255) / 256;
  blocks = blocks < cap ? blocks : cap;
  return (unsigned)(blocks > 0 ? blocks : 1);
}

size_t wide_vit_lobuf_bytes(int B, int T, int N, int obs_mode) {
  return obs_mode == HMM355_OBS_PROB ? align_up((size_t)B * T * N * sizeof(float), 256) : 0;
}

// A | AT (N,N) | U | V (B,T,N) | SA | SB | M (B,T) fp32 | CLA | CLB (B,T) fp64, pieces 256-B aligned
struct WFbWs {
  float *A, *AT, *U, *V, *SA, *SB, *M;
  double *CLA, *CLB;
};
size_t wide_fb_layout(int B, int T, int N, char* base, WFbWs* w) {
  const size_t rows = (size_t)B * T;
  Carver c{base};
  w->A = c.take<float>((size_t)N * N);
  w->AT = c.take<float>((size_t)N * N);
  w->U = c.take<float>(rows * N);
  w->V = c.take<float>(rows * N);
  w->SA = c.take<float>(rows);
  w->SB = c.take<float>(rows);
  w->M = c.take<float>(rows);
  w->CLA = c.take<double>(rows);
  w->CLB = c.take<double>(rows);
  return c.bytes();
}

}  // namespace
}  // namespace hmm355

using namespace hmm355;

HMM355_API size_t hmm355_viterbi_wide_workspace_bytes(int B, int T, int N, int obs_mode) {
  if (B < 0 || T < 1 || N < 1 || N > kWideMaxN) return 0;
  if (obs_mode != HMM355_OBS_PROB && obs_mode != HMM355_OBS_LOG) return 0;
  return align_up((size_t)B * T * N * sizeof(uint16_t), 256) + wide_vit_lobuf_bytes(B, T, N, obs_mode);
}

HMM355_API int hmm355_viterbi_wide_f32(const float* obs, int obs_mode, const float* log_P, const float* init, int B,
                                       int T, int N, int64_t* states, float* log_delta, float* final_score,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 0 || N < 0) return HMM355_E_ARG;
  if (N < 1 || N > kWideMaxN) return HMM355_E_STATES;
  if (T < 1) return HMM355_E_SHAPE;
  if (B == 0) return HMM355_OK;
  if (!obs || !log_P || !init || !states || !log_delta || !workspace) return HMM355_E_ARG;
  if (obs_mode != HMM355_OBS_PROB && obs_mode != HMM355_OBS_LOG) return HMM355_E_ARG;
  if ((size_t)B * T > (size_t)1 << 40 || B > 65535 * kBT) return HMM355_E_SHAPE;
  if (workspace_bytes < hmm355_viterbi_wide_workspace_bytes(B, T, N, obs_mode)) return HMM355_E_WORKSPACE;
  hipStream_t sm = static_cast<hipStream_t>(stream);
  uint16_t* psi = static_cast<uint16_t*>(workspace);
  const float* lo = obs;
  if (obs_mode == HMM355_OBS_PROB) {
    float* lobuf = reinterpret_cast<float*>(static_cast<char*>(workspace) +
                                            align_up((size_t)B * T * N * sizeof(uint16_t), 256));
    const size_t n = (size_t)B * T * N;
    HMM355_TRY(launch(wide_log_obs_kernel, dim3(stride_blocks(n, 8192)), dim3(256), 0, sm, obs, lobuf, n));
    lo = lobuf;
  }
  WVitArgs a{lo, log_P, log_delta, psi, B, T, N};
  HMM355_TRY(launch(wide_vit_init_kernel, dim3(stride_blocks((size_t)B * N, 4096)), dim3(256), 0, sm, a, init));
  const dim3 grid((N + kColTile - 1) / kColTile, (B + kBT - 1) / kBT);
  for (int t = 1; t < T; ++t) {
    HMM355_TRY(launch(wide_vit_step_kernel, grid, dim3(kStepThreads), 0, sm, a, t));
  }
  return launch(wide_backtrace_kernel, dim3(B), dim3(256), 0, sm, a, states, final_score);
}

HMM355_API size_t hmm355_fb_wide_workspace_bytes(int B, int T, int N) {
  if (B < 0 || T < 1 || N < 1 || N > kWideMaxN) return 0;
  WFbWs w;
  return wide_fb_layout(B, T, N, nullptr, &w);
}

HMM355_API int hmm355_forward_backward_wide_f32(const float* obs, int obs_mode, const float* log_P,
                                                const float* log_p0, int B, int T, int N, unsigned out_mask,
                                                float* posterior, float* forward, float* backward, float* loglik,
                                                float* lik_ref, void* workspace, size_t workspace_bytes,
                                                void* stream) {
  if (B < 0 || N < 0) return HMM355_E_ARG;
  if (N < 1 || N > kWideMaxN) return HMM355_E_STATES;
  if (T < 1) return HMM355_E_SHAPE;
  if (B == 0) return HMM355_OK;
  if (!obs || !log_P || !log_p0 || !workspace) return HMM355_E_ARG;
  if ((out_mask & HMM355_FB_POSTERIOR) && !posterior) return HMM355_E_ARG;
  if ((out_mask & HMM355_FB_FORWARD) && !forward) return HMM355_E_ARG;
  if ((out_mask & HMM355_FB_BACKWARD) && !backward) return HMM355_E_ARG;
  if (obs_mode != HMM355_OBS_PROB && obs_mode != HMM355_OBS_LOG) return HMM355_E_ARG;
  if ((size_t)B * T > (size_t)1 << 40 || B > 65535 * kBT) return HMM355_E_SHAPE;
  if (workspace_bytes < hmm355_fb_wide_workspace_bytes(B, T, N)) return HMM355_E_WORKSPACE;
  hipStream_t sm = static_cast<hipStream_t>(stream);
  WFbWs w;
  wide_fb_layout(B, T, N, static_cast<char*>(workspace), &w);
  const size_t rows = (size_t)B * T;
  HMM355_TRY(launch(wide_exp_matrix_kernel, dim3(stride_blocks((size_t)N * N, 4096)), dim3(256), 0, sm, log_P, N, w.A,
                    w.AT));
  if (obs_mode == HMM355_OBS_LOG) {
    HMM355_TRY(launch(row_max_kernel<false>, dim3(stride_blocks(rows * 64, 4096)), dim3(256), 0, sm, obs, nullptr, T, N,
                      rows, w.M));
  }
  WFbArgs a{obs, w.M, w.A, w.AT, w.U, w.V, w.SA, w.SB, B, T, N, obs_mode};
  HMM355_TRY(launch(wide_fb_init_kernel, dim3(stride_blocks((size_t)B * N, 4096)), dim3(256), 0, sm, a, log_p0));
  const dim3 grid((N + kColTile - 1) / kColTile, (B + kBT - 1) / kBT, 2);
  for (int k = 1; k < T; ++k) {
    HMM355_TRY(launch(wide_fb_step_kernel, grid, dim3(kStepThreads), 0, sm, a, k));
  }
  HMM355_TRY(launch(wide_scan_kernel, dim3(B), dim3(256), 0, sm, a, w.CLA, w.CLB, loglik));
  const unsigned mask = out_mask & (HMM355_FB_POSTERIOR | HMM355_FB_FORWARD | HMM355_FB_BACKWARD);
  if (mask || lik_ref) {
    const size_t visits = mask ? rows : (size_t)B;
    HMM355_TRY(launch(wide_post_kernel, dim3(stride_blocks(visits * 64, 8192)), dim3(256), 0, sm, a, w.CLA, w.CLB,
                      mask, posterior, forward, backward, lik_ref));
  }
  return HMM355_OK;
}
