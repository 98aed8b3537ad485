// hmm355 — forward-backward and Viterbi over a padded batch with per-sequence lengths on gfx950.
//
// The tuned chains (recur.h, band.h, fbpair.h, follow.h) take one T for the whole batch: their
// 16-step blocks, end rows and publish / follow protocol are built around it.  A padded batch of
// unequal lengths takes this separate form instead, selected from the input alone
// (pytorch_hmm_amd/ops.py: lengths given and unequal), as wide.hip is for N > 256.
//
// One workgroup per sequence and job (alpha chain, beta chain; Viterbi chain): workgroup b reads
// len_b = lengths[b] once and runs exactly len_b steps, so a short sequence ends early and frees
// its CU.  No workgroup waits on another, there are no flags and no floating-point atomics, and
// nothing needs co-residency: two calls on the same inputs return the same bits.
//
// The chain is adjoint.hip's compact one.  NP/32 waves; wave w owns outputs o = 32w + (lane & 31),
// the two half-waves split the inputs (lane >> 5 = input half h), the lane's half-row of the
// matrix lives in VGPRs.  Per step the previous vector (NP floats) is read from LDS by broadcast
// float4 reads, the two halves are joined by v_permlane32_swap, the new row leaves to HBM from
// the half-0 lanes and the next product input goes to the other LDS buffer: one s_barrier per
// step.  The emission loads are issued 8 steps ahead into a register ring, and the emission of
// step q + 1 is staged (x + 1e-8, exp(x - M), or the correctly rounded log) while step q waits at
// its barrier.
//
// Forward-backward: the scaled probability-domain recursion with a DEFERRED normaliser, as
// wide.hip's.  A step stores its raw row; the next step divides by that row's sum, which every
// lane forms alongside its FMAs from the LDS reads it makes anyway (the same operations in every
// lane, hence the same bits, and no second barrier):
//     U_0 = exp(log_p0) e_0;             U_{t+1} = (A^T U_t) e_{t+1} / CA_t,   CA_t = sum_i U_t[i]
//     V_{len-1} = 1 or exp(lbt - max);   V_{t-1} = A (e_t V_t) / CB_t,         CB_t = sum_j e_t[j] V_t[j]
// in the workspace layout of hmm355_fb_workspace_layout (U | V (B,T,NP), LA | LB, .., CA | CB), so
// autograd.py and hmm355_fb_adjoint_f32 read the pieces they read after the tuned chains.  A scan
// kernel sums the log-scales in fp64 (LA_t = sum_{k<t} log CA_k + sum_{k<=t} M_k, LB likewise) and
// forms loglik; a row pass forms posterior / forward / backward / lik_ref.
// Padded frames t >= len_b: U = V = 0, CA = CB = 1, LA = LB = 0, outputs 0; also CA = 1 at
// len_b - 1 and CB = 1 at frame 0, so no later division meets a zero or an unwritten word.
//
// Viterbi: delta_t[j] = fl(max_i fl(delta_{t-1}[i] + log_P[i][j]) + lo_t[j]) (hmm.py:154-184).
// Within an input half candidates are taken in ascending i with strict >, the halves combine by
// argmax_combine (larger value, equal -> lower index), a column that is all -inf gets index 0:
// the trellis and path have the bits of viterbi.hip / wide.hip.  psi is one byte per cell in the
// workspace; the backtrace runs in the chain's own workgroup once it ends: the first argmax of
// delta[len_b - 1], then psi in 64-row chunks staged in LDS with one lane walking.  Padded
// frames: log_delta = -inf, states = -1.
//
// The input in padded frames is never read.
#include "launch.h"
#include "logcr.h"

namespace hmm355 {
namespace {

constexpr int kRagChunk = 64;  // psi rows per backtrace chunk

// the sequence's length clamped to 1 .. T (common.h seq_len less its test for null lengths, which
// the entry points refuse; with the test these kernels compile to other code)
__device__ __forceinline__ int rag_len(const int* lengths, int b, int T) {
  const int n = lengths[b];
  return n < 1 ? 1 : (n > T ? T : n);
}

// -------------------------------------------------------------------- forward-backward
struct RagFbArgs {
  const float* obs;      // (B,T,N) emissions
  const float* log_P;    // (N,N)
  const float* log_p0;   // (N)
  const float* lbt;      // (B,N) log of the terminal backward vector, or null
  const int* lengths;    // (B)
  const float* rmax;     // (B,T) row maxima (OBS_LOG)
  float* U;              // (B,T,NP)
  float* V;              // (B,T,NP)
  float* CA;             // (B,T)
  float* CB;             // (B,T)
  float* bscale;         // (B) log-scale of the terminal backward vector
  int B, T, N;
};

// OBS_LOG: M_t = max_j lo_t[j] of the valid frames (0 for a row without a finite maximum and in
// padded frames, which are not read).  One wave per row, grid-stride.  (common.h's
// row_max_kernel<true> less the test for null lengths.)
__global__ void __launch_bounds__(256) rag_row_max_kernel(const float* __restrict__ lo, const int* __restrict__ lengths,
                                                          int T, int N, size_t rows, float* __restrict__ m) {
  const int l = threadIdx.x & 63;
  const size_t nw = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t row = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; row < rows; row += nw) {
    const int b = (int)(row / T), t = (int)(row % T);
    float v = -INFINITY;
    if (t < rag_len(lengths, b, T)) {
      const float* src = lo + row * N;
      for (int j = l; j < N; j += 64) v = fmaxf(v, src[j]);
      v = wave_max_dpp2(v);
    }
    if (l == 0) m[row] = (v > -INFINITY && v < INFINITY) ? v : 0.f;
  }
}

// CH 0: alpha chain (time ascending), CH 1: beta chain (time descending from len - 1)
template <int NP, int OBS, int CH>
__device__ __forceinline__ void rag_fb_chain(const RagFbArgs& a, int b, float* lds) {
  using G = ChainGeo<NP>;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int o = 32 * w + (l & 31), h = l >> 5;
  const int T = a.T, N = a.N;
  const int len = rag_len(a.lengths, b, T);
  const bool ook = o < N;
  const int oc = ook ? o : 0;
  // matrix slice: alpha: out j = o, inputs i (A[i][o]);  beta: out i = o, inputs j (A[o][j])
  float M[G::HALF];
#pragma unroll
  for (int k = 0; k < G::HALF; ++k) {
    const int i = G::HALF * h + k;
    const bool ok = ook && i < N;
    const float v = a.log_P[ok ? (CH == 0 ? (size_t)i * N + o : (size_t)o * N + i) : 0];
    M[k] = ok ? __expf(v) : 0.f;
  }
  const size_t rb = (size_t)b * T;
  auto tau = [&](int q) { return CH == 0 ? q : len - 1 - q; };  // frame of step q
  float* out = CH == 0 ? a.U : a.V;
  float* cs = CH == 0 ? a.CA : a.CB;
  float rx[G::PD], rm[G::PD];
  auto load = [&](int q, int p) {
    const int qq = q < len ? q : len - 1;  // clamped: the tail re-loads the last valid frame
    const size_t row = rb + tau(qq);
    rx[p] = a.obs[row * N + oc];
    rm[p] = OBS == HMM355_OBS_LOG ? a.rmax[row] : 0.f;
  };
  auto stage = [&](int p) { return OBS == HMM355_OBS_PROB ? rx[p] + 1e-8f : __expf(rx[p] - rm[p]); };
#pragma unroll
  for (int p = 0; p < G::PD; ++p) load(p, p);

  float v0 = 1.f;
  if (CH == 1) {
    float m = 0.f;
    if (a.lbt) {
      // terminal vector exp(lbt - max lbt), its scale into LB (every lane reads the whole row)
      const float* src = a.lbt + (size_t)b * N;
      m = -INFINITY;
      for (int j = 0; j < N; ++j) m = fmaxf(m, src[j]);
      if (!(m > -INFINITY && m < INFINITY)) m = 0.f;  // an all-zero terminal vector: every adjoint is 0
      v0 = __expf(src[oc] - m);
    }
    if (tid == 0) a.bscale[b] = m;
  }
  const float p0 = CH == 0 ? __expf(a.log_p0[oc]) : 0.f;

  float* xb = lds;  // [2][2][XS]
  float e = stage(0);
  load(G::PD, 0);
  {
    const float v = ook ? (CH == 0 ? p0 * e : v0) : 0.f;
    const float x = CH == 0 ? v : e * v;  // beta: the product input is e_t V_t
    if (h == 0) {
      out[(rb + tau(0)) * NP + o] = v;
      xb[(o / G::HALF) * G::XS + (o % G::HALF)] = ook ? x : 0.f;
    }
    // the end that no step divides by: CA at len - 1, CB at frame 0
    if (tid == 0) cs[rb + (CH == 0 ? len - 1 : 0)] = 1.f;
    e = stage(1);
    load(1 + G::PD, 1);
  }
  lds_barrier();
  // one step; PN: the ring slot of step q + 1 (a constant: the ring stays in registers), LOAD:
  // whether the step issues the loads of step q + 1 + PD
  auto step = [&](int q, auto PN, auto LOAD) {
    constexpr int pn = decltype(PN)::value;
    const float* xin = xb + ((q - 1) & 1) * 2 * G::XS + h * G::XS;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int k = 0; k < G::HALF; k += 4) {
      const float4 x4 = *reinterpret_cast<const float4*>(xin + k);
      a0 = fmaf(M[k], x4.x, a0);
      a1 = fmaf(M[k + 1], x4.y, a1);
      a2 = fmaf(M[k + 2], x4.z, a2);
      a3 = fmaf(M[k + 3], x4.w, a3);
      s0 += x4.x;
      s1 += x4.y;
      s2 += x4.z;
      s3 += x4.w;
    }
    float t0 = (a0 + a1) + (a2 + a3), t1 = t0;
    permlane32_swap(t0, t1);
    const float tot = t0 + t1;  // the product over all inputs, in both halves
    float c0 = (s0 + s1) + (s2 + s3), c1 = c0;
    permlane32_swap(c0, c1);
    const float sx = c0 + c1;   // the previous row's sum: this step's normaliser
    const float inv = sx > 0.f ? 1.f / sx : 0.f;
    const int t = tau(q);
    float v, x;
    if (CH == 0) {
      v = (tot * e) * inv;  // U_t = (A^T U_{t-1}) e_t / CA_{t-1}
      x = v;
    } else {
      v = tot * inv;        // V_t = A (e_{t+1} V_{t+1}) / CB_{t+1}
      x = e * v;
    }
    if (h == 0) {
      out[(rb + t) * NP + o] = ook ? v : 0.f;
      xb[(q & 1) * 2 * G::XS + (o / G::HALF) * G::XS + (o % G::HALF)] = ook ? x : 0.f;
    }
    if (tid == 0) cs[rb + (CH == 0 ? t - 1 : t + 1)] = sx;
    e = stage(pn);
    if constexpr (decltype(LOAD)::value) load(q + 1 + G::PD, pn);
    lds_barrier();
  };
  // whole blocks of PD steps without a branch between a load and its use (a conditional step
  // would turn the ring into copies that wait for the load just issued), then the last < PD
  // steps, whose emissions are in the ring already
  int q0 = 1;
  for (; q0 + G::PD <= len; q0 += G::PD)
    static_for<0, G::PD>([&](auto PP) {
      step(q0 + PP.value, std::integral_constant<int, (2 + PP.value) % G::PD>{}, std::true_type{});
    });
  static_for<0, G::PD>([&](auto PP) {
    if (q0 + PP.value < len)
      step(q0 + PP.value, std::integral_constant<int, (2 + PP.value) % G::PD>{}, std::false_type{});
  });
  // padded frames: zero rows, unit normalisers
  {
    float* dst = out + (rb + len) * NP;
    const size_t n = (size_t)(T - len) * NP;
    for (size_t i = tid; i < n; i += G::NT) dst[i] = 0.f;
    for (int t = len + tid; t < T; t += G::NT) cs[rb + t] = 1.f;
  }
}

template <int NP, int OBS>
__global__ void __launch_bounds__(ChainGeo<NP>::NT) rag_fb_kernel(RagFbArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[2 * 2 * ChainGeo<NP>::XS];
  const int b = blockIdx.x >> 1;
  if (blockIdx.x & 1) rag_fb_chain<NP, OBS, 1>(a, b, lds);
  else rag_fb_chain<NP, OBS, 0>(a, b, lds);
}

// One workgroup per sequence: the cumulative log-scales in fp64 (wide.hip's scan),
//   LA[t] = sum_{k<t} log CA[k] + sum_{k<=t} M_k            log alpha_t = log U_t + LA[t]
//   LB[t] = bscale + sum_{t<k<len} (log CB[k] + M_k)         log beta_t  = log V_t + LB[t]
// stored as fp32, and loglik = LA[len-1] + log sum_j U_{len-1}[j] formed in fp64.  The logs are
// formed by all lanes into LDS, 1024 steps at a time; lane 0 adds the alpha terms and lane 64
// the beta terms in time order.
constexpr int kRagScan = 1024;

struct RagPostArgs {
  const float* U;
  const float* V;
  float* LA;
  float* LB;
  const float* CA;
  const float* CB;
  const float* rmax;
  const float* bscale;
  const int* lengths;
  float* posterior;
  float* forward;
  float* backward;
  float* loglik;
  float* lik_ref;
  int B, T, N, NP, obs_mode;
  unsigned mask;
};

__global__ void __launch_bounds__(256) rag_scan_kernel(RagPostArgs a) {
  __shared__ double buf[2][kRagScan];
  __shared__ float wsum[4];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
  const int N = a.N, T = a.T, NP = a.NP;
  const int b = blockIdx.x;
  const int len = rag_len(a.lengths, b, T);
  const size_t r0 = (size_t)b * T;
  const bool shifted = a.obs_mode == HMM355_OBS_LOG;
  float part = 0.f;
  {
    const float* u = a.U + (r0 + (size_t)(len - 1)) * NP;
    for (int j = tid; j < N; j += 256) part += u[j];
  }
  part = wave_sum_dpp(part);
  if (l == 0) wsum[w] = part;
  __syncthreads();
  const float s_last = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  double ca = 0.0, cb = (double)a.bscale[b];
  for (int c0 = 0; c0 < len; c0 += kRagScan) {
    const int n = len - c0 < kRagScan ? len - c0 : kRagScan;
    for (int q = tid; q < n; q += 256) {
      const int t = c0 + q;  // alpha term of frame t; beta term of frame len-1-t
      double va = shifted ? (double)a.rmax[r0 + t] : 0.0;
      if (t > 0) va += log((double)a.CA[r0 + t - 1]);
      double vb = 0.0;
      if (t > 0) vb = log((double)a.CB[r0 + len - t]) + (shifted ? (double)a.rmax[r0 + len - t] : 0.0);
      buf[0][q] = va;
      buf[1][q] = vb;
    }
    __syncthreads();
    if (tid == 0) {
      for (int q = 0; q < n; ++q) {
        ca += buf[0][q];
        a.LA[r0 + c0 + q] = (float)ca;
      }
    } else if (tid == 64) {
      for (int q = 0; q < n; ++q) {
        cb += buf[1][q];
        a.LB[r0 + len - 1 - (c0 + q)] = (float)cb;
      }
    }
    __syncthreads();
  }
  for (int t = len + tid; t < T; t += 256) {
    a.LA[r0 + t] = 0.f;
    a.LB[r0 + t] = 0.f;
  }
  if (tid == 0 && a.loglik) a.loglik[b] = clean_loglik((float)(ca + log((double)s_last)));
}

// One wave per (b,t) row, grid-stride: fb_posterior_kernel's arithmetic (post.h) on rows of
// stride NP, with the sequence's own last row for lik_ref and zeros in padded frames.
template <int NP>
__global__ void __launch_bounds__(256) rag_post_kernel(RagPostArgs a) {
  constexpr int K = NP / 64;
  const int l = threadIdx.x & 63;
  const int N = a.N, T = a.T;
  const size_t rows = (size_t)a.B * T;
  const size_t nw = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t row = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; row < rows; row += nw) {
    const int b = (int)(row / T), t = (int)(row % T);
    const int len = rag_len(a.lengths, b, T);
    if (t >= len) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int j = l + 64 * k;
        if (j < N) {
          const size_t off = row * N + j;
          if (a.mask & HMM355_FB_POSTERIOR) a.posterior[off] = 0.f;
          if (a.mask & HMM355_FB_FORWARD) a.forward[off] = 0.f;
          if (a.mask & HMM355_FB_BACKWARD) a.backward[off] = 0.f;
        }
      }
      continue;
    }
    const bool last = t == len - 1;
    if (!a.mask && !(last && a.lik_ref)) continue;
    float u[K], v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      u[k] = a.U[row * NP + l + 64 * k];
      v[k] = a.V[row * NP + l + 64 * k];
    }
    const float la = a.LA[row], lb = a.LB[row];
    float mu = 0.f, mv = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { mu = fmaxf(mu, u[k]); mv = fmaxf(mv, v[k]); }
    mu = wave_max_dpp2(mu);
    mv = wave_max_dpp2(mv);
    // (common.h: a row whose maxima or sum are not positive normal numbers is a dead row, all zero)
    const float iu = rcp_normal(mu), iv = rcp_normal(mv);
    float p[K], s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { p[k] = (u[k] * iu) * (v[k] * iv); s += p[k]; }
    s = wave_sum_dpp(s);
    const float is = rcp_normal(s);
    float fw[K], bw[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      p[k] = row_value(p[k] * is, is);
      fw[k] = 0.f;
      bw[k] = 0.f;
    }
    if ((a.mask & HMM355_FB_FORWARD) || (last && a.lik_ref)) {
#pragma unroll
      for (int k = 0; k < K; ++k) fw[k] = row_value(__expf(__logf(u[k]) + la), 1.f);
    }
    if (a.mask & HMM355_FB_BACKWARD) {
#pragma unroll
      for (int k = 0; k < K; ++k) bw[k] = row_value(__expf(__logf(v[k]) + lb), 1.f);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int j = l + 64 * k;
      if (j < N) {
        const size_t off = row * N + j;
        if (a.mask & HMM355_FB_POSTERIOR) a.posterior[off] = p[k];
        if (a.mask & HMM355_FB_FORWARD) a.forward[off] = fw[k];
        if (a.mask & HMM355_FB_BACKWARD) a.backward[off] = bw[k];
      }
    }
    if (last && a.lik_ref) {
      // hmm.py:206: logsumexp(log(forward[:, len - 1] + 1e-8))
      float lv[K], m = -INFINITY;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        lv[k] = (l + 64 * k < N) ? __logf(fw[k] + 1e-8f) : -INFINITY;
        m = fmaxf(m, lv[k]);
      }
      m = wave_max(m);
      float ex = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) ex += (l + 64 * k < N) ? __expf(lv[k] - m) : 0.f;
      ex = wave_sum(ex);
      if (l == 0) a.lik_ref[b] = m + __logf(ex);
    }
  }
}

// ------------------------------------------------------------------------------ Viterbi
struct RagVitArgs {
  const float* obs;     // (B,T,N)
  const float* log_P;   // (N,N)
  const float* init;    // (N)
  const int* lengths;   // (B)
  float* delta;         // (B,T,N)
  float* final_score;   // (B) or null
  int64_t* states;      // (B,T)
  uint8_t* psi;         // (B,T,NP) workspace
  int B, T, N;
};

template <int NP, int OBS>
__global__ void __launch_bounds__(ChainGeo<NP>::NT) rag_vit_kernel(RagVitArgs a) {
  using G = ChainGeo<NP>;
  __shared__ __attribute__((aligned(16))) float xb[2 * 2 * G::XS];
  __shared__ __attribute__((aligned(16))) uint8_t ps[kRagChunk][NP];
  __shared__ int st[kRagChunk];
  __shared__ int s_state;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int o = 32 * w + (l & 31), h = l >> 5;
  const int b = blockIdx.x;
  const int T = a.T, N = a.N;
  const int len = rag_len(a.lengths, b, T);
  const bool ook = o < N;
  const int oc = ook ? o : 0;
  // the lane's half-column of log_P: out j = o, inputs i; -inf outside the matrix
  float M[G::HALF];
#pragma unroll
  for (int k = 0; k < G::HALF; ++k) {
    const int i = G::HALF * h + k;
    const bool ok = ook && i < N;
    const float v = a.log_P[ok ? (size_t)i * N + o : 0];
    M[k] = ok ? v : -INFINITY;
  }
  const size_t rb = (size_t)b * T;
  float rx[G::PD];
  auto load = [&](int q, int p) {
    const int qq = q < len ? q : len - 1;
    rx[p] = a.obs[(rb + qq) * N + oc];
  };
  auto stage = [&](int p) { return OBS == HMM355_OBS_PROB ? logcr_fast(rx[p] + 1e-8f, g_logcr_tab) : rx[p]; };
#pragma unroll
  for (int p = 0; p < G::PD; ++p) load(p, p);
  float e = stage(0);
  load(G::PD, 0);
  {
    const float v = a.init[oc] + e;  // delta_0 = init + lo_0
    if (h == 0) {
      if (ook) a.delta[rb * N + o] = v;
      a.psi[rb * NP + o] = 0;
      xb[(o / G::HALF) * G::XS + (o % G::HALF)] = ook ? v : -INFINITY;
    }
    e = stage(1);
    load(1 + G::PD, 1);
  }
  lds_barrier();
  // one step (rag_fb_chain's form: PN the ring slot of step q + 1, LOAD whether it loads ahead)
  auto step = [&](int q, auto PN, auto LOAD) {
    constexpr int pn = decltype(PN)::value;
    const float* xin = xb + ((q - 1) & 1) * 2 * G::XS + h * G::XS;
    float best;
    int arg = 0;  // index within the half: small constants in the selects below
    {  // the half's first candidate is real: best starts from it (a -inf column keeps its index)
      const float4 x4 = *reinterpret_cast<const float4*>(xin);
      best = x4.x + M[0];
      const float d[3] = {x4.y, x4.z, x4.w};
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const float c = d[k - 1] + M[k];
        const bool tk = c > best;
        best = tk ? c : best;
        arg = tk ? k : arg;
      }
    }
#pragma unroll
    for (int k = 4; k < G::HALF; k += 4) {
      const float4 x4 = *reinterpret_cast<const float4*>(xin + k);
      const float d[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {  // strict > in ascending i: the first maximum wins
        const float c = d[kk] + M[k + kk];
        const bool tk = c > best;
        best = tk ? c : best;
        arg = tk ? k + kk : arg;
      }
    }
    arg += G::HALF * h;
    float v0 = best, v1 = best;
    int i0 = arg, i1 = arg;
    permlane32_swap(v0, v1);
    permlane32_swap_i(i0, i1);
    argmax_combine(v0, i0, v1, i1);  // larger value wins, equal goes to the lower index
    const float v = v0 + e;
    if (h == 0) {
      if (ook) a.delta[(rb + q) * N + o] = v;
      a.psi[(rb + q) * NP + o] = (uint8_t)(ook ? i0 : 0);
      xb[(q & 1) * 2 * G::XS + (o / G::HALF) * G::XS + (o % G::HALF)] = ook ? v : -INFINITY;
    }
    e = stage(pn);
    if constexpr (decltype(LOAD)::value) load(q + 1 + G::PD, pn);
    lds_barrier();
  };
  int q0 = 1;
  for (; q0 + G::PD <= len; q0 += G::PD)
    static_for<0, G::PD>([&](auto PP) {
      step(q0 + PP.value, std::integral_constant<int, (2 + PP.value) % G::PD>{}, std::true_type{});
    });
  static_for<0, G::PD>([&](auto PP) {
    if (q0 + PP.value < len)
      step(q0 + PP.value, std::integral_constant<int, (2 + PP.value) % G::PD>{}, std::false_type{});
  });
  __syncthreads();
  // padded frames: log_delta = -inf, states = -1
  {
    float* dst = a.delta + (rb + len) * N;
    const size_t n = (size_t)(T - len) * N;
    for (size_t i = tid; i < n; i += G::NT) dst[i] = -INFINITY;
    for (int t = len + tid; t < T; t += G::NT) a.states[rb + t] = -1;
  }
  // the first argmax of delta[len - 1] (hmm.py:174), from the row still in LDS
  if (w == 0) {
    const float* xl = xb + ((len - 1) & 1) * 2 * G::XS;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < G::K; ++k) {
      const int j = l + 64 * k;
      const float v = xl[(j / G::HALF) * G::XS + (j % G::HALF)];
      if (j < N) argmax_combine(bv, bi, v, j);
    }
    wave_argmax(bv, bi);
    if (l == 0) {
      s_state = bi;
      if (a.final_score) a.final_score[b] = bv;
    }
  }
  // the walk (hmm.py:177-178): psi in 64-row chunks staged in LDS, one lane walking.  The
  // barrier's fence makes this workgroup's psi stores visible to its loads.
  for (int t_hi = len - 1; t_hi >= 0; t_hi -= kRagChunk) {
    const int t_lo = t_hi - kRagChunk + 1 > 0 ? t_hi - kRagChunk + 1 : 0;
    const int rows = t_hi - t_lo + 1;
    __syncthreads();
    const uint8_t* psrc = a.psi + (rb + t_lo) * NP;
    for (int idx = tid; idx < rows * NP / 16; idx += G::NT)
      *reinterpret_cast<uint4*>(&ps[0][0] + idx * 16) = *reinterpret_cast<const uint4*>(psrc + idx * 16);
    __syncthreads();
    if (tid == 0) {
      int s = s_state;
      for (int t = t_hi; t >= t_lo; --t) {
        st[t - t_lo] = s;
        s = ps[t - t_lo][s];  // the state of frame t - 1
      }
      s_state = s;
    }
    __syncthreads();
    for (int i = tid; i < rows; i += G::NT) a.states[rb + t_lo + i] = st[i];
  }
}

size_t rag_vit_ws(int B, int T, int N) { return align_up((size_t)B * T * pad_states(N), 256); }

}  // namespace
}  // namespace hmm355

using namespace hmm355;

// the float pieces of hmm355_fb_workspace_layout that the ragged op uses (offsets 0-3 and 6-9; the
// BandDesc and the terminal vector, 4 and 5, are the dense op's)
struct RagFbWs {
  float *U, *V, *LA, *LB, *bscale, *rmax, *CA, *CB;
};

HMM355_API size_t hmm355_viterbi_ragged_workspace_bytes(int B, int T, int N, int obs_mode) {
  if (B < 0 || T < 1 || N < 1 || N > 256) return 0;
  if (obs_mode != HMM355_OBS_PROB && obs_mode != HMM355_OBS_LOG) return 0;
  if ((size_t)B * T > (size_t)1 << 40) return 0;
  return rag_vit_ws(B, T, N);
}

HMM355_API int hmm355_viterbi_ragged_f32(const float* obs, int obs_mode, const float* log_P, const float* init,
                                         const int* lengths, int B, int T, int N, int64_t* states, float* log_delta,
                                         float* final_score, void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 0 || N < 0) return HMM355_E_ARG;
  if (N < 1 || N > 256) return HMM355_E_STATES;
  if (T < 1) return HMM355_E_SHAPE;
  if (B == 0) return HMM355_OK;
  if (!obs || !log_P || !init || !lengths || !states || !log_delta || !workspace) return HMM355_E_ARG;
  if (obs_mode != HMM355_OBS_PROB && obs_mode != HMM355_OBS_LOG) return HMM355_E_ARG;
  if ((size_t)B * T > (size_t)1 << 40) return HMM355_E_SHAPE;
  if (workspace_bytes < rag_vit_ws(B, T, N)) return HMM355_E_WORKSPACE;
  RagVitArgs a{obs, log_P, init, lengths, log_delta, final_score, states, static_cast<uint8_t*>(workspace), B, T, N};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int NP = pad_states(N);
  const bool prob = obs_mode == HMM355_OBS_PROB;
  return with_np(NP, [&](auto np) {
    return with_flag(prob, [&](auto p) {
      constexpr int OBS = p() ? HMM355_OBS_PROB : HMM355_OBS_LOG;
      return launch(rag_vit_kernel<np(), OBS>, dim3(B), dim3(ChainGeo<np()>::NT), 0, st, a);
    });
  });
}

HMM355_API int hmm355_forward_backward_ragged_f32(const float* obs, int obs_mode, const float* log_P,
                                                  const float* log_p0, const float* log_beta_T, const int* lengths,
                                                  int B, int T, int N, unsigned out_mask, float* posterior,
                                                  float* forward, float* backward, float* loglik, float* lik_ref,
                                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (B < 0 || N < 0) return HMM355_E_ARG;
  if (N < 1 || N > 256) return HMM355_E_STATES;
  if (T < 1) return HMM355_E_SHAPE;
  if (B == 0) return HMM355_OK;
  if (!obs || !log_P || !log_p0 || !lengths || !workspace) return HMM355_E_ARG;
  if (out_mask & ~(HMM355_FB_POSTERIOR | HMM355_FB_FORWARD | HMM355_FB_BACKWARD)) return HMM355_E_ARG;
  if ((out_mask & HMM355_FB_POSTERIOR) && !posterior) return HMM355_E_ARG;
  if ((out_mask & HMM355_FB_FORWARD) && !forward) return HMM355_E_ARG;
  if ((out_mask & HMM355_FB_BACKWARD) && !backward) return HMM355_E_ARG;
  if (obs_mode != HMM355_OBS_PROB && obs_mode != HMM355_OBS_LOG) return HMM355_E_ARG;
  if ((size_t)B * T > (size_t)1 << 40 || B > (1 << 30)) return HMM355_E_SHAPE;
  if (workspace_bytes < hmm355_fb_workspace_bytes(B, T, N)) return HMM355_E_WORKSPACE;
  // the pieces of hmm355_fb_workspace_layout, by name
  size_t off[10];
  const int rc = hmm355_fb_workspace_layout(B, T, N, off);
  if (rc != HMM355_OK) return rc;
  char* base = static_cast<char*>(workspace);
  auto piece = [&](int i) { return reinterpret_cast<float*>(base + off[i]); };
  const RagFbWs w{piece(0), piece(1), piece(2), piece(3), piece(6), piece(7), piece(8), piece(9)};
  const int NP = pad_states(N);
  const size_t rows = (size_t)B * T;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool prob = obs_mode == HMM355_OBS_PROB;
  if (!prob)
    HMM355_TRY(launch(rag_row_max_kernel, dim3(row_grid(rows, 4096)), dim3(256), 0, st, obs, lengths, T, N, rows,
                      w.rmax));
  RagFbArgs fa{obs, log_P, log_p0, log_beta_T, lengths, w.rmax, w.U, w.V, w.CA, w.CB, w.bscale, B, T, N};
  HMM355_TRY(with_np(NP, [&](auto np) {
    return with_flag(prob, [&](auto p) {
      constexpr int OBS = p() ? HMM355_OBS_PROB : HMM355_OBS_LOG;
      return launch(rag_fb_kernel<np(), OBS>, dim3(2 * B), dim3(ChainGeo<np()>::NT), 0, st, fa);
    });
  }));
  RagPostArgs pa{w.U, w.V, w.LA, w.LB, w.CA, w.CB, w.rmax, w.bscale, lengths,
                 posterior, forward, backward, loglik, lik_ref, B, T, N, NP, obs_mode, out_mask};
  HMM355_TRY(launch(rag_scan_kernel, dim3(B), dim3(256), 0, st, pa));
  if (!out_mask && !lik_ref) return HMM355_OK;
  return with_np(NP, [&](auto np) {
    return launch(rag_post_kernel<np()>, dim3(row_grid(rows, 8192)), dim3(256), 0, st, pa);
  });
}
