// hmm355 — DurationConstrainedHMM: Viterbi with a run-length counter per cell and soft duration
// penalties (the reference's DurationConstrainedHMM._constrained_viterbi, hsmm.py:520-590).
//
// Semantics (include/hmm355.h has them in full).  Per cell (b, s): delta, psi, dur.  t = 0:
// delta = e - fl32(log S), dur = 1.  Each later step first takes, per state, the largest and the
// smallest dur of the previous row over a *group* of sequences (the reference: over the whole
// batch), forms from them pen_self[s] (dmax + 1 > max_duration) and pen_from[p] (dmin <
// min_duration), each ONE rounded fp32 product, and then per cell the first strict maximum over
// p = 0 .. S-1 of
//   p == s:  (delta[p] + e) + pen_self[s]                 new dur = dur[s] + 1, lT[s,s] never read
//   p != s:  ((delta[p] + lT[p,s]) + e) + pen_from[p]     new dur = 1
// every add rounded once, in that order.  A cell without a finite candidate keeps delta = -inf,
// psi = 0, dur = 0.
//
// One workgroup per group, the groups being consecutive runs of `group` sequences; no workgroup
// waits on another (no flags, no atomics on memory).  The previous and the current delta / dur rows of the
// group are in LDS (two buffers each, [state][sequence] so that the R sequences a thread owns
// are one broadcast read per candidate), and so are the step's two penalty vectors.  The threads
// that write a row also leave its largest and smallest dur per state in LDS (integer max / min
// atomics of the workgroup: the result does not depend on their order), and the first S threads
// form the next step's penalties from those before the cells are computed: the products are
// rounded there, once, and the cells only add (nothing for hipcc to contract into an FMA).
// An absent penalty is stored as -0.0f: x + -0.0f == x for every x, -0.0f and -inf included, so
// adding it is the same as skipping the add.
// A thread owns one state s and R sequences (dc_seqs_per_thread: 1, 2 or 4) and walks p in
// ascending order with a strict >, so the first index wins a tie with no cross-lane step.  A
// group of at most 256 cells (a sequence decoded alone, a small batch) gives each cell
// kDcSplit lanes instead, each walking a quarter of p, and combines them by shuffles.
// The transition column lT[p, s] is read from an LDS copy whose diagonal is -inf (the
// p == s candidate of the walk then never wins) while S*S floats fit beside the rows, else as
// coalesced rows from memory with the diagonal masked; the self-loop candidate is combined last
// by "larger value wins, equal values go to the smaller index" (argmax_combine), which gives the
// same winner as the reference's ascending scan.  The emissions of step t + 1 are loaded before
// the candidates of step t are walked.  Two workgroup barriers per step.
//
// psi goes to the workspace as one byte per cell, (B,T,Sp) with Sp = S rounded up to 4.  After
// the last step the same workgroup walks it back: it stages windows of as many time steps as its
// LDS holds (4-byte loads) and one lane per sequence follows its path inside the window.  One
// launch per call.
#include "launch.h"

#include <climits>
#include <cmath>

namespace hmm355 {
namespace {

constexpr int kDcMaxStates = HMM355_DCHMM_MAX_STATES;
constexpr int kDcMaxCells = HMM355_DCHMM_MAX_CELLS;
constexpr int kDcMaxThreads = 1024;
constexpr int kDcPasses = 2;           // work items (a state and R sequences) per thread, at most
constexpr int kDcSplit = 4;            // lanes that share a cell's range of p in a small group
constexpr size_t kDcMinLds = 32768;    // never less LDS than this: the walk's window

struct DcArgs {
  const float* e;        // (B,T,S)
  const float* lT;       // (S,S)
  long long* states;     // (B,T)
  float* score;          // (B)
  float* delta;          // (B,T,S) or NULL
  int* dur;              // (B,T,S) or NULL
  unsigned char* psi;    // (B,T,Sp)
  int B, T, S, G, Sp;
  int mind, maxd;
  float negw, logS;
  int lds_bytes;
};

// sequences per thread: the fewest of 1, 2, 4 with which a state and R sequences per thread
// cover the group in one pass of the largest workgroup (more waves hide the LDS latency of the
// walk over p; more sequences per thread share the lT and penalty reads once the CU is full)
inline int dc_seqs_per_thread(int G, int S) {
  for (int R = 1; R < 4; R *= 2)
    if ((long long)S * ((G + R - 1) / R) <= kDcMaxThreads) return R;
  return 4;
}

__host__ __device__ inline size_t dc_align16(size_t x) { return (x + 15) & ~(size_t)15; }
__host__ __device__ inline int dc_rows(int G, int R) { return (G + R - 1) / R * R; }

// bytes of LDS: the walk's states, two delta and two dur rows, the penalty vectors, and lT
size_t dc_lds_bytes(int G, int S, int R, bool lt_lds) {
  size_t n = dc_align16(sizeof(int) * (size_t)G) + (size_t)16 * dc_rows(G, R) * S + (size_t)16 * S;
  if (lt_lds) n += (size_t)4 * S * S;
  return n < kDcMinLds ? kDcMinLds : n;
}

// SPLIT (1 or kDcSplit, the latter with R = 1 only): lanes per cell.  Lane l of a wave has cell
// l % (64 / SPLIT) of the wave's 64 / SPLIT cells and the part l / (64 / SPLIT) of the range of p,
// consecutive p per part, so the parts combine in ascending order of p.
template <int R, bool LTL, int SPLIT>
__global__ void __launch_bounds__(kDcMaxThreads) dchmm_kernel(DcArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dc_smem[];
  static_assert(SPLIT == 1 || R == 1, "the range of p is split with one sequence per thread only");
  constexpr int K = kDcPasses;
  constexpr int CW = kWave / SPLIT;  // cells per wave
  const float NINF = -INFINITY;
  const int tid = threadIdx.x, NT = blockDim.x;
  const int S = a.S, T = a.T, Sp = a.Sp;
  const int b0 = blockIdx.x * a.G;
  const int Gk = a.B - b0 < a.G ? a.B - b0 : a.G;  // sequences of this group
  const int Gq = (Gk + R - 1) / R, Gp = Gq * R;    // ... in R-blocks, and padded
  const int nitems = S * Gq;
  const int row = S * Gp;

  int* wstate = reinterpret_cast<int*>(dc_smem);
  const size_t off_rows = dc_align16(sizeof(int) * (size_t)Gk);
  float* dl = reinterpret_cast<float*>(dc_smem + off_rows);  // [2][S][Gp]
  int* ul = reinterpret_cast<int*>(dl + 2 * row);            // [2][S][Gp]
  float* penf = reinterpret_cast<float*>(ul + 2 * row);      // [S] pen_from
  float* pens = penf + S;                                    // [S] pen_self
  int* dmx = reinterpret_cast<int*>(pens + S);               // [S] the row's largest dur per state
  int* dmn = dmx + S;                                        // [S] ... and its smallest
  float* ltl = reinterpret_cast<float*>(dmn + S);            // [S][S], diagonal -inf (LTL only)

  int is[K], iq[K];
  bool iv[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int slot = tid + k * NT;
    const int item = SPLIT == 1 ? slot : slot / kWave * CW + slot % CW;
    iv[k] = item < nitems;
    is[k] = iv[k] ? item % S : 0;
    iq[k] = iv[k] ? item / S : 0;
  }
  const int part = SPLIT == 1 ? 0 : (tid % kWave) / CW;
  const int chunk = (S + SPLIT - 1) / SPLIT;
  const int p0 = part * chunk < S ? part * chunk : S;
  const int p1 = p0 + chunk < S ? p0 + chunk : S;
  const bool writer = part == 0;  // the lane of a cell that stores its results
  auto cell = [&](int k, int r, int t) {  // index of (b, t, s) in the (B,T,S) tensors
    return ((size_t)(b0 + iq[k] * R + r) * T + t) * S + is[k];
  };
  auto load_e = [&](int t, float (&ev)[K][R]) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int r = 0; r < R; ++r) ev[k][r] = (iv[k] && iq[k] * R + r < Gk) ? a.e[cell(k, r, t)] : 0.f;
  };

  float en[K][R];
  load_e(0, en);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if (!iv[k] || !writer) continue;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool ok = iq[k] * R + r < Gk;
      const float d = ok ? en[k][r] - a.logS : NINF;
      dl[is[k] * Gp + iq[k] * R + r] = d;
      ul[is[k] * Gp + iq[k] * R + r] = ok ? 1 : 0;
      if (ok && a.delta) a.delta[cell(k, r, 0)] = d;
      if (ok && a.dur) a.dur[cell(k, r, 0)] = 1;
    }
  }
  for (int s = tid; s < S; s += NT) dmx[s] = dmn[s] = 1;  // the first row counts 1 everywhere
  if (LTL)
    for (int i = tid; i < S * S; i += NT) ltl[i] = (i / S == i % S) ? NINF : a.lT[i];
  if (T > 1) load_e(1, en);
  lds_barrier();

  for (int t = 1; t < T; ++t) {
    const float* dprev = dl + ((t - 1) & 1) * row;
    const int* uprev = ul + ((t - 1) & 1) * row;
    float* dcur = dl + (t & 1) * row;
    int* ucur = ul + (t & 1) * row;

    // the step's penalty vectors from the previous row's largest and smallest dur per state,
    // which the threads of that row left in dmx / dmn (LDS integer max / min: any order gives
    // the same result); both are reset for the row this step writes
    for (int s = tid; s < S; s += NT) {
      const int over = dmx[s] + 1 - a.maxd, under = a.mind - dmn[s];
      pens[s] = over > 0 ? __fmul_rn(a.negw, (float)over) : -0.f;
      penf[s] = under > 0 ? __fmul_rn(a.negw, (float)under) : -0.f;
      dmx[s] = 0;  // dur >= 0
      dmn[s] = INT_MAX;
    }
    lds_barrier();

    float ec[K][R];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int r = 0; r < R; ++r) ec[k][r] = en[k][r];
    if (t + 1 < T) load_e(t + 1, en);

#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (!iv[k]) continue;
      const int s = is[k], q = iq[k];
      float best[R];
      int arg[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        best[r] = NINF;
        arg[r] = 0;
      }
#pragma unroll 4
      for (int p = p0; p < p1; ++p) {
        float l;
        if (LTL) {
          l = ltl[p * S + s];
        } else {
          l = a.lT[p * S + s];
          l = p == s ? NINF : l;
        }
        const float pf = penf[p];
        float dp[R];
        if constexpr (R == 4) {
          const float4 v = *reinterpret_cast<const float4*>(dprev + p * Gp + q * 4);
          dp[0] = v.x, dp[1] = v.y, dp[2] = v.z, dp[3] = v.w;
        } else if constexpr (R == 2) {
          const float2 v = *reinterpret_cast<const float2*>(dprev + p * Gp + q * 2);
          dp[0] = v.x, dp[1] = v.y;
        } else {
          dp[0] = dprev[p * Gp + q];
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          float x = __fadd_rn(dp[r], l);
          x = __fadd_rn(x, ec[k][r]);
          x = __fadd_rn(x, pf);
          const bool take = x > best[r];
          best[r] = take ? x : best[r];
          arg[r] = take ? p : arg[r];
        }
      }
      if constexpr (SPLIT > 1) {
        // the parts of a cell sit CW lanes apart; a later part holds larger p, so "larger value
        // wins, equal values go to the smaller index" keeps the first maximum (and index 0 when
        // every part is -inf)
#pragma unroll
        for (int off = CW; off < kWave; off *= 2) {
          const float v2 = __shfl_xor(best[0], off);
          const int i2 = __shfl_xor(arg[0], off);
          argmax_combine(best[0], arg[0], v2, i2);
        }
        if (!writer) continue;
      }
      const float ps = pens[s];
      int umax = 0, umin = INT_MAX;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int c = s * Gp + q * R + r;
        float x = __fadd_rn(dprev[c], ec[k][r]);
        x = __fadd_rn(x, ps);
        argmax_combine(best[r], arg[r], x, s);
        const int u = best[r] == NINF ? 0 : (arg[r] == s ? uprev[c] + 1 : 1);
        dcur[c] = best[r];
        ucur[c] = u;
        if (q * R + r < Gk) {
          umax = u > umax ? u : umax;
          umin = u < umin ? u : umin;
          a.psi[((size_t)(b0 + q * R + r) * T + t) * Sp + s] = (unsigned char)arg[r];
          if (a.delta) a.delta[cell(k, r, t)] = best[r];
          if (a.dur) a.dur[cell(k, r, t)] = u;
        }
      }
      atomicMax(&dmx[s], umax);  // every block of R has at least one sequence of the group
      atomicMin(&dmn[s], umin);
    }
    lds_barrier();
  }

  // the last row's first maximum: the path's end and its score
  const float* dlast = dl + ((T - 1) & 1) * row;
  int endstate[4];  // Gk <= kDcMaxCells = 4 * kDcMaxThreads: at most four sequences per lane
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int b = tid + j * NT;
    endstate[j] = 0;
    if (b < Gk) {
      float best = dlast[b];
      int arg = 0;
      for (int s = 1; s < S; ++s) {
        const float v = dlast[s * Gp + b];
        const bool take = v > best;
        best = take ? v : best;
        arg = take ? s : arg;
      }
      endstate[j] = arg;
      a.score[b0 + b] = best;
      a.states[(size_t)(b0 + b) * T + T - 1] = arg;
    }
  }
  if (T == 1) return;
  global_barrier();  // every thread's psi bytes are in memory, and the rows in LDS are dead
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (tid + j * NT < Gk) wstate[tid + j * NT] = endstate[j];

  // ---- the walk: windows of psi staged in LDS, one lane per sequence inside a window
  unsigned char* win = dc_smem + off_rows;
  const int W0 = (int)(((size_t)a.lds_bytes - off_rows) / ((size_t)Gk * Sp));
  const int W = W0 < T - 1 ? W0 : T - 1;  // time steps per window (>= 1: dc_lds_bytes)
  const int wpb = W * Sp / 4;             // 4-byte words of a sequence's part of the window
  for (int thi = T - 1; thi >= 1; thi -= W) {
    const int tlo = thi - W + 1 > 1 ? thi - W + 1 : 1;
    const int nw = (thi - tlo + 1) * Sp / 4;
    __syncthreads();
    for (int i = tid; i < Gk * nw; i += NT) {
      const int b = i / nw, w = i % nw;
      const unsigned* src = reinterpret_cast<const unsigned*>(a.psi + ((size_t)(b0 + b) * T + tlo) * Sp);
      reinterpret_cast<unsigned*>(win)[(size_t)b * wpb + w] = src[w];
    }
    __syncthreads();
    for (int b = tid; b < Gk; b += NT) {
      int s = wstate[b];
      const unsigned char* wb = win + (size_t)b * wpb * 4;
      long long* out = a.states + (size_t)(b0 + b) * T;
      for (int t = thi; t >= tlo; --t) {
        s = wb[(t - tlo) * Sp + s];
        out[t - 1] = s;
      }
      wstate[b] = s;
    }
  }
}

int dc_shape_check(int B, int T, int S, int group) {
  if (B < 1) return HMM355_E_ARG;
  if (S < 1 || S > kDcMaxStates) return HMM355_E_STATES;
  if (T < 1) return HMM355_E_SHAPE;
  if (group < 1 || group > B) return HMM355_E_ARG;
  if ((long long)group * S > kDcMaxCells) return HMM355_E_STATES;
  const size_t lim = (size_t)1 << 46;
  size_t n, m;
  if (__builtin_mul_overflow((size_t)B, (size_t)T, &n) || n > lim) return HMM355_E_SHAPE;
  if (__builtin_mul_overflow(n, (size_t)S + 3, &m) || m > lim) return HMM355_E_SHAPE;
  return HMM355_OK;
}

size_t dc_ws_bytes(int B, int T, int S) { return align_up((size_t)B * T * align_up((size_t)S, 4), 256) + 256; }

template <int R, bool LTL, int SPLIT = 1>
hipError_t dc_launch(const DcArgs& a, int threads, size_t lds, hipStream_t st) {
  return launch(dchmm_kernel<R, LTL, SPLIT>, dim3((a.B + a.G - 1) / a.G), dim3(threads), lds, st, a);
}

}  // namespace
}  // namespace hmm355

using namespace hmm355;

HMM355_API size_t hmm355_dchmm_workspace_bytes(int B, int T, int S) {
  if (dc_shape_check(B, T, S, 1) != HMM355_OK) return 0;
  return dc_ws_bytes(B, T, S);
}

HMM355_API int hmm355_dchmm_viterbi_f32(const float* emis, const float* log_T, int B, int T, int S, int group,
                                        int min_duration, int max_duration, float penalty_weight, int64_t* states,
                                        float* final_score, float* log_delta, int32_t* durations, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  const int rc = dc_shape_check(B, T, S, group);
  if (rc != HMM355_OK) return rc;
  if (!emis || !log_T || !states || !final_score || !workspace) return HMM355_E_ARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return HMM355_E_ARG;
  if (workspace_bytes < dc_ws_bytes(B, T, S)) return HMM355_E_WORKSPACE;
  const int R = dc_seqs_per_thread(group, S);
  const bool lt_lds = dc_lds_bytes(group, S, R, true) <= kExclusiveLds;
  const size_t lds = dc_lds_bytes(group, S, R, lt_lds);
  const int nitems = S * ((group + R - 1) / R);
  // a group of few cells (a sequence alone, say) would leave the CU to one or two waves, each
  // walking all of p: kDcSplit lanes per cell then share the walk
  const bool split = R == 1 && nitems * kDcSplit <= kDcMaxThreads;
  const int slots = split ? (nitems + kWave / kDcSplit - 1) / (kWave / kDcSplit) * kWave : nitems;
  const int threads = slots >= kDcMaxThreads ? kDcMaxThreads : (slots + kWave - 1) / kWave * kWave;
  if (slots > kDcPasses * threads || lds > kExclusiveLds) return HMM355_E_STATES;  // not reached inside the limits
  DcArgs a{};
  a.e = emis;
  a.lT = log_T;
  a.states = reinterpret_cast<long long*>(states);
  a.score = final_score;
  a.delta = log_delta;
  a.dur = durations;
  a.psi = static_cast<unsigned char*>(workspace);
  a.B = B;
  a.T = T;
  a.S = S;
  a.G = group;
  a.Sp = (S + 3) / 4 * 4;
  a.mind = min_duration;
  a.maxd = max_duration;
  a.negw = -penalty_weight;
  a.logS = (float)std::log((double)S);
  a.lds_bytes = (int)lds;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return with_flag(lt_lds, [&](auto ltl) {
    if (R == 4) return dc_launch<4, ltl()>(a, threads, lds, st);
    if (R == 2) return dc_launch<2, ltl()>(a, threads, lds, st);
    if (split) return dc_launch<1, ltl(), kDcSplit>(a, threads, lds, st);
    return dc_launch<1, ltl()>(a, threads, lds, st);
  });
}
