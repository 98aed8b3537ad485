// hmm355 — HMM recursions over an arc list (a sparse transition matrix) on gfx950.
//
// The model is the dense one whose log_P is -inf off the arcs: N <= 8192 states, E <= 2^20 arcs
// (src, dst, log_w) shared by the batch, OBS_LOG emissions, optional per-sequence lengths.  The
// cost of a step is proportional to the arcs, not to N^2 (include/hmm355.h spells the contract
// out; DESIGN.md §13K has the measurements).
//
// One workgroup per (sequence, job), the jobs being the Viterbi chain with its backtrace, the
// alpha chain and the beta chain; workgroup b runs exactly len_b steps.  No workgroup waits on
// another, there are no flags and no atomics, nothing needs co-residency: two calls on the same
// inputs give the same bits.  This is the launch shape of ragged.hip, forced.hip and nbest.hip.
//
// Geometry.  NT = N rounded up to a wave (at most 1024) threads; thread tid owns the states
// tid + d NT, d < D = ceil(N / NT) <= 8 (a template parameter: 1, 2, 4 or 8).  The previous and
// the current state row live in LDS, double-buffered (2 x 32 KiB at N = 8192): one barrier per
// step.  The host passes the arcs grouped by their owner state (a row-pointer array, the other
// end of every arc, its weight): by destination, source ascending, for Viterbi and alpha; by
// source for beta.  A thread loops over the arcs of each state it owns and reads the other end's
// value from the LDS row.
//   REG: when no state has more than 4 arcs (3 above 4096 states) on the owner side (the host knows: it
//     validates the row pointers), the thread's arcs stay in registers for the whole sequence
//     (empty slots: weight -inf / 0), as forced.hip keeps its weights: no global load on the
//     step's dependency chain but the emission, which is loaded one step ahead.
//   streamed: otherwise the arcs are read through L2 every step.  A state with more than one
//     wave's worth (64) of arcs is not taken by its owner: wave 0 lists those hubs once (ballot
//     compaction, ascending) in LDS and every step the waves take them in turn, lanes striding
//     over the arcs and combining by wave_argmax / a DPP sum -- otherwise a hub sets the step time.
//
// Viterbi: delta_0 = init + e_0, delta_t[j] = fl(max fl(delta_{t-1}[src] + log_w) + e_t[j]),
// candidates in ascending source with strict >, a state whose maximum is -inf gets pointer 0:
// the bits of viterbi.hip / ragged.hip / wide.hip on the densified matrix.  Back-pointers are
// uint16 rows in the workspace; the walk stages as many rows as fit the chain's LDS (at most 64)
// and one lane walks them, as ragged.hip / nbest.hip do.
//
// Sums: ragged.hip's scaled probability-domain recursion with the deferred normaliser,
//     U_0 = exp(log_p0) e_0;  U_t[j] = (sum_in U_{t-1}[src] A_e) e_t[j] / CA_{t-1},  CA_t = sum_i U_t[i]
//     X_{len-1} = e_{len-1};  V_{t-1}[i] = (sum_out A_e X_t[dst]) / sum_j X_t[j],    X_t = e_t V_t
// with e_t = exp(obs_t - M_t), M_t the row maximum, A_e = exp(log_w) formed once per call.  Every
// wave leaves the sum of what it wrote in LDS and after the barrier every thread adds the NW
// partial sums in the same order.  The log-scales are summed in fp64 after the chains
// (sp_scan_kernel); a row pass forms gamma and the two per-frame factors the arc counts need.
// The arc counts are a second call over the stored rows: a thread per arc, the (b, t) rows cut
// into tiles, an fp64 partial sum per (tile, arc) and a second kernel adding them in tile order.
//
// Frames t >= len_b are never read.  An arc's other end is clamped into [0, N) and a row pointer
// into [0, E] as read, so a wrong device array cannot index out of bounds.
#include "launch.h"

namespace hmm355 {
namespace {

constexpr int kSpMaxStates = HMM355_SPARSE_MAX_STATES;
constexpr int kSpMaxArcs = HMM355_SPARSE_MAX_ARCS;
constexpr int kSpHub = 64;      // arcs of one state above which a whole wave takes it
// arcs per state kept in registers: 4, and 3 with 8 states per thread (N > 4096), where a fourth
// slot (8 more sources and 8 more weights) no longer fits 128 VGPRs without scratch
template <int D>
constexpr int kSpReg = D == 8 ? 3 : 4;
constexpr int kSpMaxNT = 1024;  // threads
// unrolling of the streamed arc loop: none with 4 or 8 states per thread (the copies' scalars spill)
template <int D>
constexpr int kSpUnroll = D >= 4 ? 1 : 4;
constexpr int kSpChunk = 64;    // back-pointer rows per backtrace chunk, at most
constexpr int kSpMaxWaves = kSpMaxNT / kWave;

// arcs grouped by owner state: state j owns arcs ptr[j] .. ptr[j + 1] - 1
struct SpGraph {
  const int* ptr;    // (N + 1)
  const int* other;  // (E) the state at the arc's other end
  const float* w;    // (E) log weight (Viterbi) or probability (sums)
};

inline int sp_pad(int N) { return (N + 63) & ~63; }
inline int sp_threads(int N) { return N >= kSpMaxNT ? kSpMaxNT : sp_pad(N); }

// The thread's owned states and their arc ranges; the hubs' list in LDS (streamed form).
template <int D, bool REG>
struct SpOwn {
  int lo[D], hi[D];
  int ro[REG ? D : 1][kSpReg<D>];
  float rw[REG ? D : 1][kSpReg<D>];
};

template <int D, bool REG>
__device__ __forceinline__ void sp_own_init(SpOwn<D, REG>& o, const SpGraph& g, int N, int E, float empty,
                                            uint16_t* hub, int* nhub) {
  const int tid = threadIdx.x, NT = blockDim.x;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const int j = tid + d * NT;
    int lo = 0, hi = 0;
    if (j < N) {
      lo = clamp_int(g.ptr[j], 0, E);
      hi = clamp_int(g.ptr[j + 1], 0, E);
      if (hi < lo) hi = lo;
    }
    if (!REG && hi - lo > kSpHub) hi = lo;  // a hub: the waves take it
    if (REG && hi - lo > kSpReg<D>) hi = lo + kSpReg<D>;
    o.lo[d] = lo;
    o.hi[d] = hi;
    if constexpr (REG) {
#pragma unroll
      for (int r = 0; r < kSpReg<D>; ++r) {
        const bool in = lo + r < hi;
        o.ro[d][r] = in ? clamp_int(g.other[lo + r], 0, N - 1) : 0;
        o.rw[d][r] = in ? g.w[lo + r] : empty;
      }
    }
  }
  if constexpr (!REG) {
    if (tid < kWave) {
      int n = 0;
      for (int j0 = 0; j0 < N; j0 += kWave) {
        const int j = j0 + tid;
        bool h = false;
        if (j < N) h = clamp_int(g.ptr[j + 1], 0, E) - clamp_int(g.ptr[j], 0, E) > kSpHub;
        const unsigned long long m = __ballot(h);
        if (h) hub[n + __popcll(m & ((1ull << tid) - 1ull))] = (uint16_t)j;
        n += __popcll(m);
      }
      if (tid == 0) *nhub = n;
    }
  }
}

// ------------------------------------------------------------------------------ Viterbi
struct SpVitArgs {
  const float* obs;    // (B,T,N) log-emissions
  SpGraph g;           // by destination, source ascending; log weights
  const float* init;   // (N)
  const int* lengths;  // (B) or null
  float* delta;        // (B,T,N)
  float* final_score;  // (B) or null
  int64_t* states;     // (B,T)
  uint16_t* bp;        // (B,T,NB) workspace
  int B, T, N, E, NB, rows_fit;
};

template <int D, bool REG>
__global__ void __launch_bounds__(kSpMaxNT) sp_vit_kernel(SpVitArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sp_smem[];
  __shared__ int st[kSpChunk];
  __shared__ float wv[kSpMaxWaves];
  __shared__ int wi[kSpMaxWaves];
  __shared__ int s_state, s_nhub;
  const int tid = threadIdx.x, NT = blockDim.x, w = tid >> 6, l = tid & 63, NW = NT >> 6;
  const int N = a.N, T = a.T, E = a.E, NB = a.NB, NPAD = (N + 63) & ~63;
  float* row = reinterpret_cast<float*>(sp_smem);  // [2][NPAD]
  uint16_t* hub = reinterpret_cast<uint16_t*>(row + 2 * NPAD);
  const int b = blockIdx.x;
  const int len = seq_len(a.lengths, b, T);
  const size_t rb = (size_t)b * T;
  SpOwn<D, REG> o;
  sp_own_init(o, a.g, N, E, -INFINITY, hub, &s_nhub);
  // hubs are written by their wave, not by the owner
  bool mine[D];
  int jc[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const int j = tid + d * NT;
    jc[d] = j < N ? j : 0;
    mine[d] = j < N;
    if (!REG && j < N) mine[d] = clamp_int(a.g.ptr[j + 1], 0, E) - clamp_int(a.g.ptr[j], 0, E) <= kSpHub;
  }
  float e[D];
  auto load = [&](int q, int d) { return a.obs[(rb + (q < len ? q : len - 1)) * N + jc[d]]; };
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const int j = tid + d * NT;
    if (j < N) {
      const float v = a.init[j] + load(0, d);  // delta_0 = init + e_0
      row[j] = v;
      a.delta[rb * N + j] = v;
    }
    e[d] = load(1, d);
  }
  __syncthreads();
  const int nhub = REG ? 0 : s_nhub;

  for (int t = 1; t < len; ++t) {
    const float* prev = row + ((t - 1) & 1) * NPAD;
    float* cur = row + (t & 1) * NPAD;
    float en[D];
#pragma unroll
    for (int d = 0; d < D; ++d) en[d] = load(t + 1, d);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      float best = -INFINITY;
      int arg = 0;
      if constexpr (REG) {
#pragma unroll
        for (int r = 0; r < kSpReg<D>; ++r) {  // strict > in ascending source: the first maximum wins
          const float c = prev[o.ro[d][r]] + o.rw[d][r];
          const bool tk = c > best;
          best = tk ? c : best;
          arg = tk ? o.ro[d][r] : arg;
        }
      } else {
#pragma unroll kSpUnroll<D>
        for (int k = o.lo[d]; k < o.hi[d]; ++k) {
          const int s = clamp_int(a.g.other[k], 0, N - 1);
          const float c = prev[s] + a.g.w[k];
          const bool tk = c > best;
          best = tk ? c : best;
          arg = tk ? s : arg;
        }
      }
      if (mine[d]) {
        const int j = jc[d];
        const float v = best + e[d];
        cur[j] = v;
        a.delta[(rb + t) * N + j] = v;
        a.bp[(rb + t) * NB + j] = (uint16_t)arg;
      }
      e[d] = en[d];
    }
    // the hubs, a wave each in turn (wave-uniform loop)
    for (int h = w; h < nhub; h += NW) {
      const int j = hub[h];
      const int lo = clamp_int(a.g.ptr[j], 0, E), hi = clamp_int(a.g.ptr[j + 1], 0, E);
      float best = -INFINITY;
      int arg = 0x7fffffff;
      for (int k = lo + l; k < hi; k += kWave) {
        const int s = clamp_int(a.g.other[k], 0, N - 1);
        const float c = prev[s] + a.g.w[k];
        const bool tk = c > best;
        best = tk ? c : best;
        arg = tk ? s : arg;
      }
      wave_argmax(best, arg);  // larger value, equal -> lower source
      if (l == 0) {
        const float v = best + a.obs[(rb + t) * N + j];
        cur[j] = v;
        a.delta[(rb + t) * N + j] = v;
        a.bp[(rb + t) * NB + j] = (uint16_t)(best > -INFINITY ? arg : 0);
      }
    }
    lds_barrier();
  }
  // padded frames: log_delta = -inf, states = -1
  {
    float* dst = a.delta + (rb + len) * N;
    const size_t n = (size_t)(T - len) * N;
    for (size_t i = tid; i < n; i += NT) dst[i] = -INFINITY;
    for (int t = len + tid; t < T; t += NT) a.states[rb + t] = -1;
  }
  // the first argmax of delta[len - 1], from the row still in LDS
  {
    const float* last = row + ((len - 1) & 1) * NPAD;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int j = tid + d * NT;
      if (j < N) argmax_combine(bv, bi, last[j], j);
    }
    wave_argmax(bv, bi);
    if (l == 0) {
      wv[w] = bv;
      wi[w] = bi;
    }
    __syncthreads();
    if (tid == 0) {
      for (int k = 1; k < NW; ++k) argmax_combine(bv, bi, wv[k], wi[k]);
      s_state = bi < N ? bi : 0;
      if (a.final_score) a.final_score[b] = bv;
    }
  }
  // the walk: pointer rows t_lo .. t_hi staged in LDS over the dead state rows (the barrier's
  // fence makes this workgroup's pointer stores visible to its loads), one lane walking
  const int R = a.rows_fit < kSpChunk ? a.rows_fit : kSpChunk;
  uint16_t* stg = reinterpret_cast<uint16_t*>(sp_smem);
  if (len == 1) {
    __syncthreads();
    if (tid == 0) a.states[rb] = s_state;
  }
  for (int t_hi = len - 1; t_hi >= 1; t_hi -= R) {
    const int t_lo = t_hi - R + 1 > 1 ? t_hi - R + 1 : 1;
    const int rows = t_hi - t_lo + 1;
    __syncthreads();
    const uint4* src = reinterpret_cast<const uint4*>(a.bp + (rb + t_lo) * NB);
    const int n16 = rows * (NB / 8);
    for (int idx = tid; idx < n16; idx += NT) reinterpret_cast<uint4*>(stg)[idx] = src[idx];
    __syncthreads();
    if (tid == 0) {
      int s = s_state;
      for (int t = t_hi; t >= t_lo; --t) {
        st[t - t_lo] = s;
        s = stg[(size_t)(t - t_lo) * NB + s];  // the state of frame t - 1
        s = s < N ? s : 0;
      }
      s_state = s;
      if (t_lo == 1) a.states[rb] = s;
    }
    __syncthreads();
    for (int i = tid; i < rows; i += NT) a.states[rb + t_lo + i] = st[i];
  }
}

// -------------------------------------------------------------------------------- sums
// A_e = exp(log_w) in both arc orders, once per call
__global__ void __launch_bounds__(256) sp_exp_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                     float* __restrict__ oa, float* __restrict__ ob, int E) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < E) {
    oa[i] = expf(a[i]);
    ob[i] = expf(b[i]);
  }
}

struct SpFbArgs {
  const float* obs;     // (B,T,N)
  SpGraph gin;          // by destination; probabilities
  SpGraph gout;         // by source; probabilities
  const float* log_p0;  // (N)
  const int* lengths;   // (B) or null
  const float* rmax;    // (B,T)
  float* U;             // (B,T,N)
  float* V;             // (B,T,N)
  float* CA;            // (B,T)
  int B, T, N, E;
};

// CH 0: alpha chain (time ascending), CH 1: beta chain (time descending from len - 1)
template <int D, bool REG, int CH>
__device__ __forceinline__ void sp_fb_chain(const SpFbArgs& a, int b, float* row, uint16_t* hub, float* wsum,
                                            int* s_nhub) {
  const int tid = threadIdx.x, NT = blockDim.x, w = tid >> 6, l = tid & 63, NW = NT >> 6;
  const int N = a.N, T = a.T, E = a.E, NPAD = (N + 63) & ~63;
  const SpGraph& g = CH == 0 ? a.gin : a.gout;
  const int len = seq_len(a.lengths, b, T);
  const size_t rb = (size_t)b * T;
  SpOwn<D, REG> o;
  sp_own_init(o, g, N, E, 0.f, hub, s_nhub);
  bool mine[D];
  int jc[D];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const int j = tid + d * NT;
    jc[d] = j < N ? j : 0;
    mine[d] = j < N;
    if (!REG && j < N) mine[d] = clamp_int(g.ptr[j + 1], 0, E) - clamp_int(g.ptr[j], 0, E) <= kSpHub;
  }
  auto tau = [&](int q) { return CH == 0 ? q : len - 1 - q; };  // frame of step q
  auto emis = [&](int q, int j) {
    const size_t r = rb + tau(q < len ? q : len - 1);
    return expf(a.obs[r * N + j] - a.rmax[r]);
  };
  float* out = CH == 0 ? a.U : a.V;
  float e[D];
  float ps = 0.f;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const int j = tid + d * NT;
    if (j < N) {
      const float e0 = emis(0, j);
      const float v = CH == 0 ? expf(a.log_p0[j]) * e0 : 1.f;
      const float x = CH == 0 ? v : e0;  // beta: the next step's input is e_t V_t
      out[(rb + tau(0)) * N + j] = v;
      row[j] = x;
      ps += x;
    }
    e[d] = emis(1, jc[d]);
  }
  ps = wave_sum_dpp(ps);
  if (l == 0) wsum[w] = ps;
  __syncthreads();
  const int nhub = REG ? 0 : *s_nhub;

  for (int q = 1; q < len; ++q) {
    const float* prev = row + ((q - 1) & 1) * NPAD;
    float* cur = row + (q & 1) * NPAD;
    const float* wp = wsum + ((q - 1) & 1) * kSpMaxWaves;
    const int t = tau(q);
    float en[D];
#pragma unroll
    for (int d = 0; d < D; ++d) en[d] = emis(q + 1, jc[d]);
    // the previous row's sum, the same additions in every thread: this step's normaliser
    float sx = wp[0];
    for (int k = 1; k < NW; ++k) sx += wp[k];
    const float inv = sx > 0.f ? 1.f / sx : 0.f;
    if (CH == 0 && tid == 0) a.CA[rb + t - 1] = sx;
    ps = 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
      float acc = 0.f;
      if constexpr (REG) {
#pragma unroll
        for (int r = 0; r < kSpReg<D>; ++r) acc = fmaf(prev[o.ro[d][r]], o.rw[d][r], acc);
      } else {
#pragma unroll kSpUnroll<D>
        for (int k = o.lo[d]; k < o.hi[d]; ++k) acc = fmaf(prev[clamp_int(g.other[k], 0, N - 1)], g.w[k], acc);
      }
      if (mine[d]) {
        const int j = jc[d];
        float v, x;
        if (CH == 0) {
          v = (acc * e[d]) * inv;
          x = v;
        } else {
          v = acc * inv;
          x = e[d] * v;
        }
        out[(rb + t) * N + j] = v;
        cur[j] = x;
        ps += x;
      }
      e[d] = en[d];
    }
    for (int h = w; h < nhub; h += NW) {
      const int j = hub[h];
      const int lo = clamp_int(g.ptr[j], 0, E), hi = clamp_int(g.ptr[j + 1], 0, E);
      float acc = 0.f;
      for (int k = lo + l; k < hi; k += kWave) acc = fmaf(prev[clamp_int(g.other[k], 0, N - 1)], g.w[k], acc);
      acc = wave_sum_dpp(acc);
      if (l == 0) {
        const size_t r = rb + t;
        const float ej = expf(a.obs[r * N + j] - a.rmax[r]);
        float v, x;
        if (CH == 0) {
          v = (acc * ej) * inv;
          x = v;
        } else {
          v = acc * inv;
          x = ej * v;
        }
        out[r * N + j] = v;
        cur[j] = x;
        ps += x;
      }
    }
    ps = wave_sum_dpp(ps);
    if (l == 0) wsum[(q & 1) * kSpMaxWaves + w] = ps;
    lds_barrier();
  }
  // padded frames: zero rows, unit normalisers; CA at len - 1, which no step divides by
  {
    float* dst = out + (rb + len) * N;
    const size_t n = (size_t)(T - len) * N;
    for (size_t i = tid; i < n; i += NT) dst[i] = 0.f;
    if (CH == 0)
      for (int t = len - 1 + tid; t < T; t += NT) a.CA[rb + t] = 1.f;
  }
}

template <int D, bool REG_IN, bool REG_OUT>
__global__ void __launch_bounds__(kSpMaxNT) sp_fb_kernel(SpFbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sp_smem[];
  __shared__ float wsum[2 * kSpMaxWaves];
  __shared__ int s_nhub;
  const int NPAD = (a.N + 63) & ~63;
  float* row = reinterpret_cast<float*>(sp_smem);
  uint16_t* hub = reinterpret_cast<uint16_t*>(row + 2 * NPAD);
  const int b = blockIdx.x >> 1;
  if (blockIdx.x & 1) sp_fb_chain<D, REG_OUT, 1>(a, b, row, hub, wsum, &s_nhub);
  else sp_fb_chain<D, REG_IN, 0>(a, b, row, hub, wsum, &s_nhub);
}

// One workgroup per sequence: loglik = sum_t M_t + sum_{t<len-1} log CA_t + log sum_j U_{len-1}[j],
// the terms in fp64, each thread its own in time order and the 256 partial sums in thread order.
__global__ void __launch_bounds__(256) sp_scan_kernel(const float* __restrict__ U, const float* __restrict__ CA,
                                                      const float* __restrict__ rmax, const int* __restrict__ lengths,
                                                      int T, int N, float* __restrict__ loglik) {
  __shared__ double part[256];
  __shared__ double last[256];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int len = seq_len(lengths, b, T);
  const size_t r0 = (size_t)b * T;
  double s = 0.0, u = 0.0;
  for (int t = tid; t < len; t += 256) {
    s += (double)rmax[r0 + t];
    if (t < len - 1) s += log((double)CA[r0 + t]);
  }
  const float* ul = U + (r0 + len - 1) * N;
  for (int j = tid; j < N; j += 256) u += (double)ul[j];
  part[tid] = s;
  last[tid] = u;
  __syncthreads();
  if (tid == 0) {
    double ts = 0.0, tu = 0.0;
    for (int k = 0; k < 256; ++k) {
      ts += part[k];
      tu += last[k];
    }
    loglik[b] = clean_loglik((float)(ts + log(tu)));
  }
}

// One wave per (b,t) row, grid-stride: gamma = (U / max U)(V / max V) / s, and the two factors
// the arc counts use, Q1 = 1 / (max U * s) and Q2 = 1 / max V; zeros in padded frames and in a
// frame without probability.
__global__ void __launch_bounds__(256) sp_post_kernel(const float* __restrict__ U, const float* __restrict__ V,
                                                      const int* __restrict__ lengths, int B, int T, int N,
                                                      float* __restrict__ Q1, float* __restrict__ Q2,
                                                      float* __restrict__ posterior) {
  const int l = threadIdx.x & 63;
  const size_t rows = (size_t)B * T;
  const size_t nw = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t row = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; row < rows; row += nw) {
    const int b = (int)(row / T), t = (int)(row % T);
    const float* u = U + row * N;
    const float* v = V + row * N;
    float iu = 0.f, iv = 0.f, is = 0.f;
    if (t < seq_len(lengths, b, T)) {
      float mu = 0.f, mv = 0.f;
      for (int j = l; j < N; j += 64) {
        mu = fmaxf(mu, u[j]);
        mv = fmaxf(mv, v[j]);
      }
      mu = wave_max_dpp2(mu);
      mv = wave_max_dpp2(mv);
      // (common.h: a row whose maxima or sum are not positive normal numbers is a dead row: zeros,
      // and zero factors for the arc counts)
      iu = rcp_normal(mu);
      iv = rcp_normal(mv);
      float s = 0.f;
      for (int j = l; j < N; j += 64) s += (u[j] * iu) * (v[j] * iv);
      s = wave_sum_dpp(s);
      is = rcp_normal(s);
    }
    if (l == 0) {
      Q1[row] = row_value(iu * is, is);
      Q2[row] = row_value(iv, is);
    }
    if (posterior) {
      float* p = posterior + row * N;
      if (__float_as_uint(is) != 0u) {
        for (int j = l; j < N; j += 64) p[j] = row_value(((u[j] * iu) * (v[j] * iv)) * is, is);
      } else {
        for (int j = l; j < N; j += 64) p[j] = 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------------------- arc counts
struct SpCntArgs {
  const float* obs;
  const int* src;
  const int* dst;
  const float* log_w;
  const float* g;      // (B) or null
  const int* lengths;  // (B) or null
  const float* U;
  const float* V;
  const float* CA;
  const float* rmax;
  const float* Q1;
  const float* Q2;
  double* part;  // (tiles, E)
  int B, T, N, E;
  long long rows_per_tile;
};

// xi_t[e] = U_{t-1}[src] A_e e_t[dst] V_t[dst] / (CA_{t-1} S_t) with S_t = sum_j U_t[j] V_t[j]
// (= 1 / (Q1 Q2) of frame t): a thread per arc, its tile's rows in order, the sum in fp64
__global__ void __launch_bounds__(256) sp_count_kernel(SpCntArgs a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.E) return;
  const int N = a.N, T = a.T;
  const int s = a.src[e], d = a.dst[e];
  const bool ok = s >= 0 && s < N && d >= 0 && d < N;
  const float A = ok ? expf(a.log_w[e]) : 0.f;
  const int sc = ok ? s : 0, dc = ok ? d : 0;
  const long long total = (long long)a.B * T;
  const long long r0 = (long long)blockIdx.y * a.rows_per_tile;
  const long long r1 = r0 + a.rows_per_tile < total ? r0 + a.rows_per_tile : total;
  double acc = 0.0;
  for (long long r = r0; r < r1; ++r) {
    const int b = (int)(r / T), t = (int)(r % T);
    if (t < 1 || t >= seq_len(a.lengths, b, T)) continue;
    const float ca = a.CA[r - 1];
    const float ica = rcp_normal(ca);
    const float left = (a.U[(size_t)(r - 1) * N + sc] * ica) * A;
    const float right = (expf(a.obs[(size_t)r * N + dc] - a.rmax[r]) * a.V[(size_t)r * N + dc]) * a.Q2[r];
    const float x = row_value((left * right) * a.Q1[r], a.Q1[r]);  // (a dead frame has Q1 = 0: counts 0)
    const float gb = a.g ? a.g[b] : 1.f;
    acc += (double)x * (double)gb;
  }
  a.part[(size_t)blockIdx.y * a.E + e] = A > 0.f ? acc : 0.0;
}

__global__ void __launch_bounds__(256) sp_count_sum_kernel(const double* __restrict__ part, int tiles, int E,
                                                           double* __restrict__ xi) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  double s = 0.0;
  for (int k = 0; k < tiles; ++k) s += part[(size_t)k * E + e];  // tile order
  xi[e] = s;
}

// ------------------------------------------------------------------------------- host
int sp_check_shape(int B, int T, int N, int E) {
  if (B < 0) return HMM355_E_ARG;
  if (N < 1 || N > kSpMaxStates) return HMM355_E_STATES;
  if (E < 1 || E > kSpMaxArcs || T < 1) return HMM355_E_SHAPE;
  if ((size_t)B * T > (size_t)1 << 40 || (size_t)B * T * N > (size_t)1 << 44) return HMM355_E_SHAPE;
  return HMM355_OK;
}

// a host row-pointer array: non-decreasing from 0 to E; its largest difference into *maxdeg
int sp_check_ptr(const int* p, int N, int E, int* maxdeg) {
  if (p[0] != 0 || p[N] != E) return HMM355_E_ARG;
  int m = 0;
  for (int j = 0; j < N; ++j) {
    const int d = p[j + 1] - p[j];
    if (d < 0) return HMM355_E_ARG;
    m = d > m ? d : m;
  }
  *maxdeg = m;
  return HMM355_OK;
}

size_t sp_rows_lds(int N) { return (size_t)sp_pad(N) * 10; }  // two fp32 rows and the uint16 hub list
int sp_bp_stride(int N) { return (N + 7) & ~7; }
size_t sp_vit_lds(int N) {
  const size_t want = (size_t)kSpChunk * sp_bp_stride(N) * 2;
  const size_t stage = want < 65536 ? want : 65536;
  return sp_rows_lds(N) > stage ? sp_rows_lds(N) : stage;
}
size_t sp_vit_ws(int B, int T, int N) { return align_up((size_t)B * T * sp_bp_stride(N) * 2, 256); }

// the forward-backward workspace: U, V (B,T,N); CA, rmax, Q1, Q2 (B,T); A by destination, A by source (E)
struct SpFbWs {
  float *U, *V, *CA, *rmax, *Q1, *Q2, *Ain, *Aout;
};
size_t sp_fb_layout(int B, int T, int N, int E, char* base, SpFbWs* w) {
  const size_t rows = (size_t)B * T;
  Carver c{base};
  w->U = c.take<float>(rows * N);
  w->V = c.take<float>(rows * N);
  w->CA = c.take<float>(rows);
  w->rmax = c.take<float>(rows);
  w->Q1 = c.take<float>(rows);
  w->Q2 = c.take<float>(rows);
  w->Ain = c.take<float>(E);
  w->Aout = c.take<float>(E);
  return c.bytes();
}

int sp_count_tiles(int B, int T, int E) {
  const size_t rows = (size_t)B * T;
  size_t tiles = (rows + 255) / 256;
  size_t cap = ((size_t)64 << 20) / ((size_t)E * 8);
  cap = cap < 1 ? 1 : (cap > 256 ? 256 : cap);
  tiles = tiles < 1 ? 1 : (tiles > cap ? cap : tiles);
  return (int)tiles;
}

template <int D, bool REG>
hipError_t sp_vit_launch(const SpVitArgs& a, hipStream_t st) {
  const size_t lds = sp_vit_lds(a.N);
  return launch(sp_vit_kernel<D, REG>, dim3(a.B), dim3(sp_threads(a.N)), lds, st, a);
}

template <int D>
hipError_t sp_fb_launch(const SpFbArgs& a, bool rin, bool rout, hipStream_t st) {
  const size_t lds = sp_rows_lds(a.N);
  const dim3 grid(2 * a.B), block(sp_threads(a.N));
  return with_flag(rin, [&](auto ri) {
    return with_flag(rout, [&](auto ro) { return launch(sp_fb_kernel<D, ri(), ro()>, grid, block, lds, st, a); });
  });
}

int sp_slots(int N) {
  const int d = (N + kSpMaxNT - 1) / kSpMaxNT;
  return d <= 1 ? 1 : (d <= 2 ? 2 : (d <= 4 ? 4 : 8));
}

int sp_reg_budget(int N) { return sp_slots(N) == 8 ? kSpReg<8> : kSpReg<1>; }

}  // namespace
}  // namespace hmm355

using namespace hmm355;

HMM355_API size_t hmm355_sparse_viterbi_workspace_bytes(int B, int T, int N, int E) {
  if (sp_check_shape(B, T, N, E) != HMM355_OK) return 0;
  return sp_vit_ws(B, T, N);
}

HMM355_API int hmm355_sparse_viterbi_f32(const float* log_obs, const int* in_ptr_host, const int* in_ptr,
                                         const int* in_src, const float* in_log_w, const float* init,
                                         const int* lengths, int B, int T, int N, int E, int64_t* states,
                                         float* log_delta, float* final_score, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  int rc = sp_check_shape(B, T, N, E);
  if (rc != HMM355_OK) return rc;
  if (B == 0) return HMM355_OK;
  if (!log_obs || !in_ptr_host || !in_ptr || !in_src || !in_log_w || !init || !states || !log_delta || !workspace)
    return HMM355_E_ARG;
  int maxdeg = 0;
  rc = sp_check_ptr(in_ptr_host, N, E, &maxdeg);
  if (rc != HMM355_OK) return rc;
  if (workspace_bytes < sp_vit_ws(B, T, N)) return HMM355_E_WORKSPACE;
  const int NB = sp_bp_stride(N);
  SpVitArgs a{log_obs, {in_ptr, in_src, in_log_w}, init, lengths, log_delta, final_score, states,
              static_cast<uint16_t*>(workspace), B, T, N, E, NB, (int)(sp_vit_lds(N) / ((size_t)NB * 2))};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool reg = maxdeg <= sp_reg_budget(N);
  switch (sp_slots(N)) {
    case 1: return reg ? sp_vit_launch<1, true>(a, st) : sp_vit_launch<1, false>(a, st);
    case 2: return reg ? sp_vit_launch<2, true>(a, st) : sp_vit_launch<2, false>(a, st);
    case 4: return reg ? sp_vit_launch<4, true>(a, st) : sp_vit_launch<4, false>(a, st);
    default: return reg ? sp_vit_launch<8, true>(a, st) : sp_vit_launch<8, false>(a, st);
  }
}

HMM355_API size_t hmm355_sparse_forward_backward_workspace_bytes(int B, int T, int N, int E) {
  if (sp_check_shape(B, T, N, E) != HMM355_OK) return 0;
  SpFbWs w;
  return sp_fb_layout(B, T, N, E, nullptr, &w);
}

HMM355_API int hmm355_sparse_forward_backward_f32(const float* log_obs, const int* in_ptr_host, const int* in_ptr,
                                                  const int* in_src, const float* in_log_w,
                                                  const int* out_ptr_host, const int* out_ptr, const int* out_dst,
                                                  const float* out_log_w, const float* log_p0, const int* lengths,
                                                  int B, int T, int N, int E, float* loglik, float* posterior,
                                                  void* workspace, size_t workspace_bytes, void* stream) {
  int rc = sp_check_shape(B, T, N, E);
  if (rc != HMM355_OK) return rc;
  if (B == 0) return HMM355_OK;
  if (!log_obs || !in_ptr_host || !in_ptr || !in_src || !in_log_w || !out_ptr_host || !out_ptr || !out_dst ||
      !out_log_w || !log_p0 || !loglik || !workspace)
    return HMM355_E_ARG;
  int din = 0, dout = 0;
  rc = sp_check_ptr(in_ptr_host, N, E, &din);
  if (rc != HMM355_OK) return rc;
  rc = sp_check_ptr(out_ptr_host, N, E, &dout);
  if (rc != HMM355_OK) return rc;
  SpFbWs w;
  if (workspace_bytes < sp_fb_layout(B, T, N, E, static_cast<char*>(workspace), &w)) return HMM355_E_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t rows = (size_t)B * T;
  HMM355_TRY(launch(row_max_kernel<true>, dim3(row_grid(rows, 4096)), dim3(256), 0, st, log_obs, lengths, T, N, rows,
                    w.rmax));
  HMM355_TRY(launch(sp_exp_kernel, dim3((E + 255) / 256), dim3(256), 0, st, in_log_w, out_log_w, w.Ain, w.Aout, E));
  SpFbArgs a{log_obs, {in_ptr, in_src, w.Ain}, {out_ptr, out_dst, w.Aout}, log_p0, lengths,
             w.rmax, w.U, w.V, w.CA, B, T, N, E};
  const bool rin = din <= sp_reg_budget(N), rout = dout <= sp_reg_budget(N);
  switch (sp_slots(N)) {
    case 1: HMM355_TRY(sp_fb_launch<1>(a, rin, rout, st)); break;
    case 2: HMM355_TRY(sp_fb_launch<2>(a, rin, rout, st)); break;
    case 4: HMM355_TRY(sp_fb_launch<4>(a, rin, rout, st)); break;
    default: HMM355_TRY(sp_fb_launch<8>(a, rin, rout, st)); break;
  }
  HMM355_TRY(launch(sp_scan_kernel, dim3(B), dim3(256), 0, st, w.U, w.CA, w.rmax, lengths, T, N, loglik));
  return launch(sp_post_kernel, dim3(row_grid(rows, 8192)), dim3(256), 0, st, w.U, w.V, lengths, B, T, N, w.Q1, w.Q2,
                posterior);
}

HMM355_API size_t hmm355_sparse_arc_counts_workspace_bytes(int B, int T, int N, int E) {
  if (sp_check_shape(B, T, N, E) != HMM355_OK) return 0;
  return align_up((size_t)sp_count_tiles(B, T, E) * E * 8, 256);
}

HMM355_API int hmm355_sparse_arc_counts_f32(const float* log_obs, const int* src, const int* dst, const float* log_w,
                                            const float* weight, const int* lengths, int B, int T, int N, int E,
                                            const void* fb_workspace, size_t fb_workspace_bytes, double* xi,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = sp_check_shape(B, T, N, E);
  if (rc != HMM355_OK) return rc;
  if (!xi) return HMM355_E_ARG;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (B == 0) return HMM355_OK;
  if (!log_obs || !src || !dst || !log_w || !fb_workspace || !workspace) return HMM355_E_ARG;
  SpFbWs w;  // (read only here)
  char* fb = const_cast<char*>(static_cast<const char*>(fb_workspace));
  if (fb_workspace_bytes < sp_fb_layout(B, T, N, E, fb, &w)) return HMM355_E_WORKSPACE;
  const int tiles = sp_count_tiles(B, T, E);
  if (workspace_bytes < align_up((size_t)tiles * E * 8, 256)) return HMM355_E_WORKSPACE;
  const long long rows = (long long)B * T;
  SpCntArgs a{log_obs, src, dst, log_w, weight, lengths, w.U, w.V, w.CA, w.rmax, w.Q1, w.Q2,
              static_cast<double*>(workspace), B, T, N, E, (rows + tiles - 1) / tiles};
  HMM355_TRY(launch(sp_count_kernel, dim3((E + 255) / 256, tiles), dim3(256), 0, st, a));
  return launch(sp_count_sum_kernel, dim3((E + 255) / 256), dim3(256), 0, st, a.part, tiles, E, xi);
}
