// hmm355 — N-best (list) Viterbi on gfx950: the K most probable state paths of every sequence.
//
// The recursion keeps K values and K back-pointers per state instead of one (include/hmm355.h
// spells the contract out):
//     d_0[j][0] = init[j] + lo_0[j],  d_0[j][k >= 1] = -inf
//     d_t[j][k] = fl(c_k + lo_t[j]),  c_k the k-th of the N*K candidates fl(d_{t-1}[i][r] + log_P[i][j])
// ordered by value descending, then i ascending, then r ascending; the pointer of (t, j, k) is
// that candidate's (i, r).  The K best of d_{len-1}[j][k] in the same order (value, j, k) are
// ranks 0 .. K-1 and each path is read back through the pointers.
//
// One workgroup per sequence, running exactly len_b steps, then its own final selection and
// backtrace: no workgroup waits on another, nothing is atomic, two calls give the same bits.
//
// Geometry.  S * NP threads, S = 4 source parts per state (2 at NP = 256): thread (s, j) owns
// destination state j and part s of the sources, i in [s * NP/S, (s + 1) * NP/S), whose part of
// column j of log_P lives in NP/S VGPRs; s is uniform in a wave, so d_{t-1}[i][r] (LDS, [i][KB],
// double-buffered) is read by broadcast.  The thread keeps its KB best (value, 16 i + r) in
// registers with static indexing (KB, the K bucket, is 1, 4, 8 or 16; ranks K .. KB-1 are
// computed and not reported: rank k depends on the ranks <= k of the step before only).  It
// takes the sources in ascending i.  A source's list is descending, so it matters only if its
// first candidate beats the thread's last entry (a wave-uniform skip otherwise); then its KB
// candidates are merged in by a fixed network (nb_merge: half-cleaner + bitonic merge) under
// the order (value descending, pointer ascending), which is the contract's tie order and costs
// the same in every lane -- an insertion per candidate, tried first, ran whenever any lane of
// the wave needed it and was 3x slower at K = 16.  Parts 1 .. S-1 pass their lists through LDS
// ([s][k][j], conflict-free) and part 0 merges them in ascending s the same way, adds lo_t[j],
// writes the new row to the other buffer and the pointers as uint16 to the workspace, j
// fastest.  Two LDS barriers per step.
//
// Emissions: part s >= 1 holds one load in flight, for the step S - 1 ahead, and every (S-1)-th
// step one of them stages its value (the correctly rounded log for OBS_PROB) into LDS while
// part 0 merges: the load and the log stay off the step's dependency chain without a register
// ring (the step body is too long to unroll for one).
//
// The final selection (the K best of d_{len-1}[j][k] by value, then j, then k) is one lane's
// insertion scan over the row in LDS, once per sequence.  Then K lanes walk the K paths
// concurrently through pointer rows staged in LDS, up to 64 rows at a time (as many as fit in
// the chain's LDS: 7 at NP = 256, K = 16).
//
// Padded states: init = -inf and log_P = -inf, so they never enter a rank.  Frames t >= len_b are
// never read.
#include "launch.h"
#include "logcr.h"

namespace hmm355 {
namespace {

// source parts per destination state: quarters, halves at NP = 256 (a quarter there would mean
// 1024 threads with 128 VGPRs each, which the column part and the list do not fit)
template <int NP>
constexpr int kNbSlices = NP == 256 ? 2 : 4;
constexpr int kNbMaxK = 16;    // ranks (a pointer is 16 i + r in a uint16)
constexpr int kNbChunk = 64;   // pointer rows per backtrace chunk, at most

template <int NP, int KB>
struct NbGeo {
  static constexpr int S = kNbSlices<NP>;
  static constexpr int D = S - 1;                        // parts that stage emissions: steps of load-ahead
  static constexpr int SL = NP / S;                      // sources per thread
  static constexpr int NT = S * NP;                      // threads
  static constexpr int BS = NP == 256 ? 4 : 8;                           // sources whose first values are read ahead
  static constexpr int D_FLOATS = 2 * NP * KB;           // d[2][NP][KB]
  static constexpr int M_CELLS = (S - 1) * KB * NP;      // merge lists [S-1][KB][NP]: float + uint16
  static constexpr size_t LDS = (size_t)(D_FLOATS + M_CELLS) * 4 + (size_t)M_CELLS * 2;
};

struct NbArgs {
  const float* obs;     // (B,T,N)
  const float* log_P;   // (N,N)
  const float* init;    // (N)
  const int* lengths;   // (B) or null
  int64_t* paths;       // (B,K,T)
  float* scores;        // (B,K)
  int* count;           // (B) or null
  uint16_t* ptr;        // (B,T,K,NP) workspace
  int B, T, N, K, prob;
};

// (c, q) into the descending list (v, p) behind every entry >= c: strict >, so an equal value
// that came earlier stays ahead
template <int KB>
__device__ __forceinline__ void nb_insert(float (&v)[KB], int (&p)[KB], float c, int q) {
#pragma unroll
  for (int k = KB - 1; k >= 1; --k) {
    const bool up = c > v[k - 1];
    const bool here = c > v[k];
    v[k] = up ? v[k - 1] : (here ? c : v[k]);
    p[k] = up ? p[k - 1] : (here ? q : p[k]);
  }
  const bool h0 = c > v[0];
  v[0] = h0 ? c : v[0];
  p[0] = h0 ? q : p[0];
}

// The KB largest of two descending lists, (v, p) and (c, q), into (v, p), descending by value
// and, among equal values, by pointer ascending.  Needs every pointer of (c, q) above every
// pointer of (v, p) with an equal value: (c, q) comes from a later source.  A half-cleaner
// against the reversed list (strict >: the earlier entry keeps an equal value's place) leaves a
// bitonic list of the KB largest, which a bitonic merge under the full order sorts: a fixed
// network with static indexing, the same work in every lane.
template <int KB>
__device__ __forceinline__ void nb_merge(float (&v)[KB], int (&p)[KB], const float (&c)[KB], const int (&q)[KB]) {
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const bool take = c[KB - 1 - k] > v[k];
    v[k] = take ? c[KB - 1 - k] : v[k];
    p[k] = take ? q[KB - 1 - k] : p[k];
  }
#pragma unroll
  for (int st = KB / 2; st >= 1; st >>= 1) {
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      if ((k & st) == 0) {
        const float va = v[k], vb = v[k + st];
        const int pa = p[k], pb = p[k + st];
        const bool sw = (vb > va) | ((vb == va) & (pb < pa));
        v[k] = sw ? vb : va;
        v[k + st] = sw ? va : vb;
        p[k] = sw ? pb : pa;
        p[k + st] = sw ? pa : pb;
      }
    }
  }
}

template <int NP, int KB>
__global__ void __launch_bounds__(kNbSlices<NP> * NP) nbest_kernel(NbArgs a) {
  using G = NbGeo<NP, KB>;
  extern __shared__ __attribute__((aligned(16))) unsigned char nb_smem[];
  __shared__ float lo_s[2][NP];
  __shared__ float fin_v[kNbMaxK];
  __shared__ int fin_p[kNbMaxK];
  float* d = reinterpret_cast<float*>(nb_smem);
  float* mv = d + G::D_FLOATS;
  uint16_t* mp = reinterpret_cast<uint16_t*>(mv + G::M_CELLS);
  const int tid = threadIdx.x, s = tid / NP, j = tid % NP;
  const int b = blockIdx.x;
  const int T = a.T, N = a.N, K = a.K;
  int len = T;
  if (a.lengths) {
    const int n = a.lengths[b];
    len = n < 1 ? 1 : (n > T ? T : n);
  }
  const bool jok = j < N;
  const int jc = jok ? j : 0;
  // the thread's part of column j of log_P; -inf outside the matrix
  float M[G::SL];
#pragma unroll
  for (int k = 0; k < G::SL; ++k) {
    const int i = G::SL * s + k;
    const bool ok = jok && i < N;
    const float x = a.log_P[ok ? (size_t)i * N + j : 0];
    M[k] = ok ? x : -INFINITY;
  }
  const size_t rb = (size_t)b * T;
  auto load = [&](int q) { return a.obs[(rb + (q < len ? q : len - 1)) * N + jc]; };
  auto stage = [&](float x) { return a.prob ? logcr_fast(x + 1e-8f, g_logcr_tab) : x; };
  // part g >= 1 stages the steps q with q % D + 1 == g: its first one is g - 1, or D for g = 1
  float rx = 0.f;
  if (s > 0) rx = load(s == 1 ? G::D : s - 1);
  if (s == 0) {
    const float x = jok ? a.init[jc] + stage(load(0)) : -INFINITY;  // d_0 = init + lo_0
    d[j * KB] = x;
#pragma unroll
    for (int k = 1; k < KB; ++k) d[j * KB + k] = -INFINITY;
    if (!jok) {
      lo_s[0][j] = 0.f;
      lo_s[1][j] = 0.f;
    }
  } else if (s == 1 % G::D + 1) {
    if (jok) lo_s[1][j] = stage(rx);
    rx = load(1 + G::D);
  }
  lds_barrier();

  for (int t = 1; t < len; ++t) {
    // opaque per step: otherwise every source's LDS address and pointer base is hoisted out of
    // the time loop into a register of its own
    int sbase = G::SL * s;
    keep(sbase);
    const float* din = d + ((t - 1) & 1) * NP * KB + sbase * KB;
    const int pbase = sbase * 16;
    float v[KB];
    int p[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      v[k] = -INFINITY;
      p[k] = 0;
    }
    // static_for, not a pragma: the body is long and the column part must stay in registers
    static_for<0, G::SL / G::BS>([&](auto BLK) {
      constexpr int k0 = decltype(BLK)::value * G::BS;
      float x[G::BS];
#pragma unroll
      for (int u = 0; u < G::BS; ++u) x[u] = din[(k0 + u) * KB];
#pragma unroll
      for (int u = 0; u < G::BS; ++u) {
        const float Pk = M[k0 + u];
        const int q = pbase + (k0 + u) * 16;
        const float c0 = x[u] + Pk;
        if constexpr (KB == 1) {
          nb_insert(v, p, c0, q);
        } else {
          // the source's list is descending: it matters only if its first candidate enters
          if (c0 > v[KB - 1]) {
            float c[KB];
            int qq[KB];
#pragma unroll
            for (int r = 0; r < KB; r += 4) {
              const float4 x4 = *reinterpret_cast<const float4*>(din + (k0 + u) * KB + r);
              c[r] = x4.x + Pk;
              c[r + 1] = x4.y + Pk;
              c[r + 2] = x4.z + Pk;
              c[r + 3] = x4.w + Pk;
            }
#pragma unroll
            for (int r = 0; r < KB; ++r) qq[r] = q + r;
            nb_merge(v, p, c, qq);
          }
        }
      }
      // keeps the reads of later blocks from piling up in registers
      asm volatile("" ::: "memory");
    });
    if (s > 0) {
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        mv[((s - 1) * KB + k) * NP + j] = v[k];
        mp[((s - 1) * KB + k) * NP + j] = (uint16_t)p[k];
      }
    }
    lds_barrier();
    if (s == 0) {
      // the other parts' lists in ascending s
#pragma unroll
      for (int s2 = 0; s2 < G::S - 1; ++s2) {
        float c[KB];
        int qq[KB];
#pragma unroll
        for (int r = 0; r < KB; ++r) {
          c[r] = mv[(s2 * KB + r) * NP + j];
          qq[r] = mp[(s2 * KB + r) * NP + j];
        }
        if constexpr (KB == 1) nb_insert(v, p, c[0], qq[0]);
        else nb_merge(v, p, c, qq);
      }
      {
        const float e = lo_s[t & 1][j];
        float* dout = d + (t & 1) * NP * KB + j * KB;
        if constexpr (KB >= 4) {
#pragma unroll
          for (int k = 0; k < KB; k += 4)
            *reinterpret_cast<float4*>(dout + k) = make_float4(v[k] + e, v[k + 1] + e, v[k + 2] + e, v[k + 3] + e);
        } else {
          dout[0] = v[0] + e;
        }
        uint16_t* pr = a.ptr + (rb + t) * K * NP + j;
        // one running address (kept opaque), not KB hoisted ones
#pragma unroll
        for (int k = 0; k < KB; ++k) {
          if (k < K) *pr = (uint16_t)p[k];
          pr += NP;
          keep(pr);
        }
      }
    } else if (s == (t + 1) % G::D + 1) {
      // lo of step t + 1 into LDS, the load of step t + 1 + D into flight
      if (jok) lo_s[(t + 1) & 1][j] = stage(rx);
      rx = load(t + 1 + G::D);
    }
    lds_barrier();
  }
  // the final selection: the K best of d_{len-1}[j][k] by value, then j, then k -- the same scan
  // with (j, k) as the source, by one lane (once per sequence: N dependent LDS reads)
  if (tid == 0) {
    const float* dl = d + ((len - 1) & 1) * NP * KB;
    float v[KB];
    int p[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      v[k] = -INFINITY;
      p[k] = 0;
    }
    for (int i = 0; i < N; ++i) {
      float c = dl[i * KB];
      int r = 0;
#pragma nounroll
      while (c > v[KB - 1]) {
        nb_insert(v, p, c, i * 16 + r);
        if (++r == KB) break;
        c = dl[i * KB + r];
      }
    }
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      fin_v[k] = v[k];
      fin_p[k] = p[k];
    }
  }
  __syncthreads();

  // ranks 0 .. K-1: lane k of wave 0 takes rank k
  int st = 0, sl = 0;
  bool exist = false;
  if (tid < kWave) {
    const float sc = tid < K ? fin_v[tid] : -INFINITY;
    const int pk = tid < K ? fin_p[tid] : 0;
    const int cnt = __popcll(__ballot(tid < K && sc > -INFINITY));
    exist = tid < K && tid < (cnt > 1 ? cnt : 1);
    if (tid < K) a.scores[(size_t)b * K + tid] = exist ? sc : -INFINITY;
    if (tid == 0 && a.count) a.count[b] = cnt;
    st = pk >> 4;
    sl = pk & 15;
  }
  // padded frames: state -1 in every rank
  {
    const int pad = T - len;
    for (int idx = tid; idx < K * pad; idx += G::NT)
      a.paths[((size_t)b * K + idx / pad) * T + len + idx % pad] = -1;
  }
  // the walks: pointer rows t_lo .. t_hi staged in LDS (the barrier's fence makes this
  // workgroup's pointer stores visible to its loads), K lanes walking; a rank that does not
  // exist gets -1
  const size_t row_bytes = (size_t)K * NP * 2;
  const int fit = (int)(G::LDS / row_bytes);
  const int R = fit < kNbChunk ? fit : kNbChunk;
  uint16_t* stg = reinterpret_cast<uint16_t*>(nb_smem);
  int64_t* out = a.paths + ((size_t)b * K + (tid < K ? tid : 0)) * T;
  for (int t_hi = len - 1; t_hi >= 1; t_hi -= R) {
    const int t_lo = t_hi - R + 1 > 1 ? t_hi - R + 1 : 1;
    const int rows = t_hi - t_lo + 1;
    __syncthreads();
    const uint4* src = reinterpret_cast<const uint4*>(a.ptr + (rb + t_lo) * K * NP);
    const int n16 = rows * K * (NP / 8);
    for (int idx = tid; idx < n16; idx += G::NT) reinterpret_cast<uint4*>(stg)[idx] = src[idx];
    __syncthreads();
    if (tid < K) {
      for (int t = t_hi; t >= t_lo; --t) {
        if (exist) {
          out[t] = st;
          const int pk = stg[((t - t_lo) * K + sl) * NP + st];  // (state, rank) of frame t - 1
          st = pk >> 4;
          sl = pk & 15;
        } else {
          out[t] = -1;
        }
      }
    }
  }
  if (tid < K) out[0] = exist ? st : -1;
}

size_t nb_ws(int B, int T, int N, int K) { return align_up((size_t)B * T * K * pad_states(N) * 2, 256); }

int nb_check_shape(int B, int T, int N, int K, int obs_mode) {
  if (B < 0 || N < 0) return HMM355_E_ARG;
  if (obs_mode != HMM355_OBS_PROB && obs_mode != HMM355_OBS_LOG) return HMM355_E_ARG;
  if (N < 1 || N > 256 || K > kNbMaxK) return HMM355_E_STATES;
  if (T < 1 || K < 1) return HMM355_E_SHAPE;
  if ((size_t)B * T > (size_t)1 << 40) return HMM355_E_SHAPE;
  return HMM355_OK;
}

template <int NP, int KB>
hipError_t nb_launch(const NbArgs& a, hipStream_t st) {
  using G = NbGeo<NP, KB>;
  return launch(nbest_kernel<NP, KB>, dim3(a.B), dim3(G::NT), G::LDS, st, a);
}

template <int NP>
hipError_t nb_launch_k(const NbArgs& a, hipStream_t st) {
  if (a.K == 1) return nb_launch<NP, 1>(a, st);
  if (a.K <= 4) return nb_launch<NP, 4>(a, st);
  if (a.K <= 8) return nb_launch<NP, 8>(a, st);
  return nb_launch<NP, 16>(a, st);
}

}  // namespace
}  // namespace hmm355

using namespace hmm355;

HMM355_API size_t hmm355_viterbi_nbest_workspace_bytes(int B, int T, int N, int K, int obs_mode) {
  if (nb_check_shape(B, T, N, K, obs_mode) != HMM355_OK) return 0;
  return nb_ws(B, T, N, K);
}

HMM355_API int hmm355_viterbi_nbest_f32(const float* obs, int obs_mode, const float* log_P, const float* init,
                                        const int* lengths, int B, int T, int N, int K, int64_t* paths,
                                        float* scores, int* count, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  const int rc = nb_check_shape(B, T, N, K, obs_mode);
  if (rc != HMM355_OK) return rc;
  if (B == 0) return HMM355_OK;
  if (!obs || !log_P || !init || !paths || !scores || !workspace) return HMM355_E_ARG;
  if (workspace_bytes < nb_ws(B, T, N, K)) return HMM355_E_WORKSPACE;
  NbArgs a{obs, log_P, init, lengths, paths, scores, count, static_cast<uint16_t*>(workspace),
           B, T, N, K, obs_mode == HMM355_OBS_PROB};
  hipStream_t st = static_cast<hipStream_t>(stream);
  return with_np(pad_states(N), [&](auto np) { return nb_launch_k<np()>(a, st); });
}
