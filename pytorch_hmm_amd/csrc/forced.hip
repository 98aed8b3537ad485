// hmm355 — transcript forced alignment: a left-to-right chain per utterance.  Forward sum (alpha,
// log-likelihood), backward sum (beta), Viterbi with its walk and durations, and the occupancy /
// gradient kernel.
//
// Sequence b has S_b positions in transcript order; position s emits class id_s = state_ids[b,s]
// (or s itself without ids: the monotonic-alignment-search form, log_probs already (B,T,S)) and
// stays (weight log_stay[b,s]), advances to s + 1 (log_next[b,s]) or skips to s + 2
// (log_skip[b,s]); weights are indexed by the source position.  A path starts in position 0 and
// ends in S_b - 1.  Absent weights are 0, 0 and -inf (no skips).
//
// One launch per call, the whole batch in it: one workgroup per (sequence, job), the jobs being
// the forward sum (always: it gives loglik), the backward sum (HMM355_FORCED_BETA) and the
// max-plus forward with its walk (HMM355_FORCED_VITERBI).  No workgroup waits on another; no
// flags, no atomics.  The layout is ctc.hip's.
//
// How lanes own positions.  A thread owns P consecutive positions u = k P .. k P + P - 1 and keeps
// their values in registers for the whole sequence, with the three weights and the class of each
// (loaded once).  The backward job runs the same body on the mirrored lattice (u = S_b - 1 - s,
// time T_b - 1 - i): "take from s + 1, s + 2" becomes "take from u - 1, u - 2", and the weights
// of a cell's candidates are its own next / skip instead of its neighbours'.  Per step a thread
// needs the last two values of the thread to its left.  They travel as one float2 through LDS,
// double-buffered by step parity, so a step costs one barrier; in one wave (Smax <= 64) they come
// by lane shuffles, no LDS and no barrier.  P is chosen per call from Smax, the smallest that
// covers it: 1 in one wave (<= 64), 1 (<= 256), kForcedPosLow (<= 512), kForcedPos (<= 1024),
// kForcedPosMid (<= 2048), kForcedPosWide (<= 4096 = HMM355_FORCED_MAX_POSITIONS).
// Emissions lp[b, t, id_s] are a gather; a thread issues the loads of step i + kForcedAhead while
// it computes step i, into a register ring, so their latency is not on the dependent chain.  A
// class outside [0, C) is never read: its emission is -inf.
// The plain form (no ids, no weights: PLAIN) has no weight adds, two candidates per cell and
// reads its emissions as P consecutive floats of a row at constant offsets from one address.
//
// The sum jobs carry c[u] = the value including the step's emission: every candidate is
// c + weight (one rounding), r = LSE of the candidates (or the start value 0 at u = 0 on the
// first step; -0 in the forward jobs, so that alpha[0,0] = e[0,0] even when that is -0),
// c = r + e.  The forward job stores c (alpha); the backward job stores r: beta excludes the
// emission of its own frame, the convention of the CTC tables.  -inf candidates drop out of the
// LSE.  Without HMM355_FORCED_ALPHA the forward job stores no table at all.
// Viterbi: max in place of LSE; candidates in the order stay, u - 1, u - 2 with strict >, so the
// first wins a tie; the end is S_b - 1.  The choice is kept as 2 bits per cell in the workspace,
// and lane 0 walks it afterwards through windows of the table staged in LDS; the path is monotone,
// so the same walk counts the run of every position (durations) in a register.
//
// Gradient (forced_grad_kernel, one workgroup per sequence and tile of kForcedGradRows frames):
// gamma[b,t,s] = exp(alpha + beta - loglik), d loglik / d lp[b,t,c] = sum over {s: id_s = c} of
// gamma, and d loglik / d log_stay[b,s] = sum over t >= 1 of exp(alpha[t-1,s] + stay[s] + e[t,s]
// + beta[t,s] - loglik), likewise next and skip with their target positions.  Every exponent is
// formed in fp64 from the fp32 tables and normalised by its frame's own LSE_s(alpha + beta -
// loglik), which is 0 in exact arithmetic: alpha and beta of a long utterance are large numbers
// whose accumulated rounding is mostly common to the positions of a frame, and it cancels there
// (each frame's gamma sums to 1 to fp32 rounding however long the utterance).  A transition's
// term is taken as gamma of its target times the transition's share among the candidates into
// that target (the same number in exact arithmetic): a ratio of neighbouring alphas, exactly 1
// for a lone candidate, and no emission is read.
// No floating-point atomics: the positions of a class are grouped once per workgroup ("next
// position of the same class" links, formed in LDS) and one lane sums a class's chain in position
// order; a frame's normaliser is a fixed shuffle tree; the sums over t are taken by a thread per
// position over its tile's frames in frame order (fp64), stored per tile in the workspace, and
// forced_grad_combine_kernel adds the tiles in tile order.  Two runs give the same bits.
#include "launch.h"

namespace hmm355 {
namespace {

constexpr int kForcedThreads = 256;   // threads per workgroup of the LDS forms
constexpr int kForcedPosLow = 2;      // positions per thread: Smax <= 512 (1 up to Smax = 256)
constexpr int kForcedPos = 4;         // Smax <= 1024
constexpr int kForcedPosMid = 8;      // Smax <= 2048
constexpr int kForcedPosWide = 16;    // Smax <= 4096
constexpr int kForcedAhead = 4;       // steps between an emission gather and its use
constexpr int kForcedWalkRows = 64;   // backtrace window: frames
constexpr int kForcedWalkBytes = 136; // ... and bytes of a frame's choices (2 * 63 + 1 positions)
constexpr int kForcedGradRows = 32;   // frames per occupancy workgroup of the gradient kernel
constexpr int kForcedMax = HMM355_FORCED_MAX_POSITIONS;
static_assert(kForcedThreads * kForcedPosWide >= kForcedMax, "the widest form covers the ABI's limit");

constexpr int kJobForward = 0, kJobBackward = 1, kJobViterbi = 2;

struct ForcedArgs {
  const float* lp;        // (B,T,C)
  const int* ids;         // (B,Smax) or NULL
  const int* in_len;      // (B)
  const int* st_len;      // (B)
  const float* w_stay;    // (B,Smax) or NULL
  const float* w_next;
  const float* w_skip;
  float* alpha;           // (B,T,Smax) or NULL
  float* beta;            // (B,T,Smax) or NULL
  float* loglik;          // (B)
  int* path;              // (B,T)
  float* score;           // (B)
  int* dur;               // (B,Smax)
  unsigned char* bp;      // (B,T,row_bytes) the Viterbi choices
  int B, T, C, Smax;
  int jobs[3];
};

struct ForcedShared {
  float2 xch[2][kForcedThreads + 2];  // slot k + 2: thread k's last two values
  unsigned char win[kForcedWalkRows][kForcedWalkBytes];
  float fin;
  int wpos[2];
};

template <int P, int NT, bool VIT, bool PLAIN>
__device__ __forceinline__ void forced_run(const ForcedArgs& a, const int job, ForcedShared& sh) {
  constexpr int AH = kForcedAhead;
  constexpr int PB = (P + 3) / 4;  // bytes of choices per thread and step
  constexpr int RB = NT * PB;      // ... per frame
  const float NINF = -INFINITY;
  const int k = threadIdx.x;
  const int b = blockIdx.x;
  const int T = a.T, C = a.C, Sm = a.Smax;
  const int Tb = clamp_int(a.in_len[b], 1, T);
  const int Sb = clamp_int(a.st_len[b], 1, Sm);
  const bool back = job == kJobBackward;
  float* tab = VIT ? nullptr : (back ? a.beta : a.alpha);
  if (tab) tab += (size_t)b * T * Sm;
  unsigned char* bp = VIT ? a.bp + (size_t)b * T * RB : nullptr;

  // cells no step writes: frames >= T_b and positions >= S_b
  if (tab) {
    const size_t lo = (size_t)Tb * Sm, hi = (size_t)T * Sm;
    for (size_t e = lo + k; e < hi; e += NT) tab[e] = NINF;
    if (Sb < Sm) {
      const int w = Sm - Sb;
      for (size_t e = k; e < (size_t)Tb * w; e += NT) tab[(e / w) * Sm + Sb + (e % w)] = NINF;
    }
  }

  // once per sequence: the class and the candidate weights of each owned position
  int cls[P];
  float w0[P], w1[P], w2[P];
  unsigned valid = 0;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int u = k * P + j;
    const int s = back ? Sb - 1 - u : u;
    cls[j] = -1;
    w0[j] = 0.f;
    w1[j] = w2[j] = NINF;
    if (u < Sb) {
      valid |= 1u << j;
      if (!PLAIN) {
        const size_t row = (size_t)b * Sm;
        const int c = a.ids ? a.ids[row + s] : s;
        if (c >= 0 && c < C) cls[j] = c;
        if (a.w_stay) w0[j] = a.w_stay[row + s];
        // forward: the weights of the sources s - 1, s - 2; mirrored: this position's own
        const int s1 = back ? s : s - 1, s2 = back ? s : s - 2;
        if (u >= 1) w1[j] = a.w_next ? a.w_next[row + s1] : 0.f;
        if (u >= 2 && a.w_skip) w2[j] = a.w_skip[row + s2];
      }
    }
  }

  const float* lpb = a.lp + (size_t)b * T * C;
  auto gather = [&](int i, float (&e)[P]) __attribute__((always_inline)) {
    const int t = back ? Tb - 1 - i : i;
    const float* row = lpb + (size_t)t * C;
    if (PLAIN) {
      // class = position: P consecutive floats, descending for the mirrored job
      if (back) {
        const float* p = row + (Sb - 1 - k * P - (P - 1));
#pragma unroll
        for (int j = 0; j < P; ++j) e[j] = ((valid >> j) & 1u) ? p[P - 1 - j] : 0.f;
      } else {
        const float* p = row + k * P;
#pragma unroll
        for (int j = 0; j < P; ++j) e[j] = ((valid >> j) & 1u) ? p[j] : 0.f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < P; ++j) e[j] = cls[j] >= 0 ? row[cls[j]] : (((valid >> j) & 1u) ? NINF : 0.f);
    }
  };

  float c[P];
#pragma unroll
  for (int j = 0; j < P; ++j) c[j] = NINF;
  float ring[AH][P];
  static_for<0, AH>([&](auto ph) {
    if (ph.value < Tb) gather(ph.value, ring[ph.value]);
  });
  constexpr bool LDS = NT > 64;  // the exchange goes through LDS (else: one wave, lane shuffles)
  if (LDS && k == 0) {
    sh.xch[0][0] = sh.xch[0][1] = make_float2(NINF, NINF);
    sh.xch[1][0] = sh.xch[1][1] = make_float2(NINF, NINF);
  }

  auto step = [&](int i, float (&e)[P]) __attribute__((always_inline)) {
    const int t = back ? Tb - 1 - i : i;
    float in1, in2 = NINF;  // the values of u0 - 1 and u0 - 2
    if (!LDS) {
      in1 = __shfl_up(c[0], 1);
      if (k < 1) in1 = NINF;
      if (!PLAIN) {
        in2 = __shfl_up(c[0], 2);
        if (k < 2) in2 = NINF;
      }
    } else if (P == 1) {
      in1 = sh.xch[i & 1][k + 1].y;
      if (!PLAIN) in2 = sh.xch[i & 1][k].y;
    } else {
      const float2 v = sh.xch[i & 1][k + 1];
      in2 = v.x;
      in1 = v.y;
    }
    float n[P];
    unsigned bits[PB];
#pragma unroll
    for (int q = 0; q < PB; ++q) bits[q] = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int u = k * P + j;
      float stay = c[j];
      float p1 = j >= 1 ? c[j >= 1 ? j - 1 : 0] : in1;
      float p2 = NINF;
      if (!PLAIN) {
        stay += w0[j];
        p1 += w1[j];
        p2 = (j >= 2 ? c[j >= 2 ? j - 2 : 0] : (j == 1 ? in1 : in2)) + w2[j];
      }
      float r;
      if (VIT) {
        unsigned d = 0;
        r = stay;
        if (p1 > r) {
          r = p1;
          d = 1;
        }
        if (!PLAIN && p2 > r) {
          r = p2;
          d = 2;
        }
        bits[j >> 2] |= d << (2 * (j & 3));
      } else {
        r = PLAIN ? lse2(stay, p1) : lse3(stay, p1, p2);
      }
      // the start: beta's 0, and -0 for the forward jobs so that alpha[0,0] is e[0,0] to the bit
      if (i == 0) r = u == 0 ? (back ? 0.f : -0.f) : NINF;
      const bool ok = (valid >> j) & 1u;
      if (!ok) r = NINF;
      const float val = r + e[j];
      if (tab && ok) tab[(size_t)t * Sm + (back ? Sb - 1 - u : u)] = back ? r : val;
      n[j] = val;
    }
#pragma unroll
    for (int j = 0; j < P; ++j) c[j] = n[j];
    if (LDS) sh.xch[(i + 1) & 1][k + 2] = make_float2(c[P >= 2 ? P - 2 : 0], c[P - 1]);
    if (VIT && i > 0 && k * P < Sb) {
#pragma unroll
      for (int q = 0; q < PB; ++q) bp[(size_t)t * RB + k * PB + q] = (unsigned char)bits[q];
    }
    if (i + AH < Tb) gather(i + AH, e);
    if (LDS) lds_barrier();
  };

  for (int i0 = 0; i0 < Tb; i0 += AH)
    static_for<0, AH>([&](auto ph) {
      if (i0 + ph.value < Tb) step(i0 + ph.value, ring[ph.value]);
    });

  if (back) return;

  // the last frame's end position
#pragma unroll
  for (int j = 0; j < P; ++j)
    if (k * P + j == Sb - 1) sh.fin = c[j];
  __syncthreads();
  const float best = sh.fin;
  if (!VIT) {
    if (k == 0) a.loglik[b] = best;
    return;
  }

  // ---- the walk: lane 0 follows the choices back through windows staged in LDS
  int* path = a.path + (size_t)b * T;
  int* dur = a.dur + (size_t)b * Sm;
  if (k == 0) a.score[b] = best;
  const bool feasible = best > NINF;
  for (int t = (feasible ? Tb : 0) + k; t < T; t += NT) path[t] = -1;
  for (int s = k; s < Sm; s += NT) dur[s] = 0;
  if (!feasible) return;
  auto byte_of = [&](int u) { return (u / P) * PB + ((u % P) >> 2); };
  if (k == 0) {
    sh.wpos[0] = Tb - 1;
    sh.wpos[1] = Sb - 1;
  }
  global_barrier();  // every thread's choices and the zeroed durations are in memory
  int last = -1, run = 0;   // lane 0: the position of the frames walked last and how many they are
  for (;;) {
    __syncthreads();
    int t = sh.wpos[0], s = sh.wpos[1];
    if (t <= 0) break;
    const int tlo = t - (kForcedWalkRows - 1) > 1 ? t - (kForcedWalkRows - 1) : 1;
    const int slo = s - 2 * (t - tlo) > 0 ? s - 2 * (t - tlo) : 0;
    const int blo = byte_of(slo);
    const int nb = byte_of(s) - blo + 1, nr = t - tlo + 1;
    for (int e = k; e < nr * kForcedWalkBytes; e += NT) {
      const int r = e / kForcedWalkBytes, cc = e % kForcedWalkBytes;
      if (cc < nb) sh.win[r][cc] = bp[(size_t)(tlo + r) * RB + blo + cc];
    }
    __syncthreads();
    if (k == 0) {
      while (t >= tlo) {
        path[t] = s;
        if (s == last) {
          ++run;
        } else {
          if (last >= 0) dur[last] = run;
          last = s;
          run = 1;
        }
        const unsigned d = (sh.win[t - tlo][byte_of(s) - blo] >> (2 * ((s % P) & 3))) & 3u;
        s -= (int)d;
        --t;
      }
      sh.wpos[0] = t;
      sh.wpos[1] = s;
    }
  }
  if (k == 0) {
    const int s = sh.wpos[1];
    path[0] = s;
    if (s == last) {
      dur[s] = run + 1;
    } else {
      if (last >= 0) dur[last] = run;
      dur[s] = 1;
    }
  }
}

template <int P, int NT, bool PLAIN>
__global__ void __launch_bounds__(NT) forced_kernel(ForcedArgs a) {
  __shared__ ForcedShared sh;
  const int job = a.jobs[blockIdx.y];
  if (job == kJobViterbi)
    forced_run<P, NT, true, PLAIN>(a, job, sh);
  else
    forced_run<P, NT, false, PLAIN>(a, job, sh);
}

// ------------------------------------------------- occupancy, class and transition gradients
struct ForcedGradArgs {
  const float* alpha;   // (B,T,Smax)
  const float* beta;    // (B,T,Smax)
  const float* loglik;  // (B)
  const int* ids;       // (B,Smax) or NULL
  const int* in_len;
  const int* st_len;
  const float* w_stay;  // (B,Smax) or NULL
  const float* w_next;
  const float* w_skip;
  float* gamma;         // (B,T,Smax) or NULL
  float* grad;          // (B,T,C) or NULL
  float* g_stay;        // (B,Smax) or NULL
  float* g_next;
  float* g_skip;
  int B, T, C, Smax;
  double* part;         // (B,tiles,3,Smax): the tiles' transition sums, or NULL
  int tiles;            // workgroups per sequence: kForcedGradRows frames each
};

__global__ void __launch_bounds__(kForcedThreads) forced_grad_kernel(ForcedGradArgs a) {
  constexpr int NT = kForcedThreads;
  constexpr int NW = NT / 64;
  __shared__ int lab[kForcedMax];
  __shared__ short nxt[kForcedMax];
  __shared__ unsigned char has_prev[kForcedMax];
  __shared__ float nrm[kForcedGradRows];  // the frames' normalisers, relative to loglik
  const int k = threadIdx.x;
  const int lane = k & 63, w = k >> 6;
  const int b = blockIdx.x;
  const int T = a.T, C = a.C, Sm = a.Smax;
  const int Tb = clamp_int(a.in_len[b], 1, T);
  const int Sb = clamp_int(a.st_len[b], 1, Sm);
  const float ll = a.loglik[b];
  const float NINF = -INFINITY;
  const bool live = ll > NINF;
  const int* ids = a.ids ? a.ids + (size_t)b * Sm : nullptr;
  const float* al = a.alpha + (size_t)b * T * Sm;
  const float* be = a.beta + (size_t)b * T * Sm;

  // ---- occupancy and class gradient of kForcedGradRows frames
  const int t0 = blockIdx.y * kForcedGradRows;
  const int t1 = t0 + kForcedGradRows < T ? t0 + kForcedGradRows : T;
  // this workgroup's frames start as zero: classes that are not in the chain, frames >= T_b,
  // an infeasible pair
  if (a.grad) {
    float* g = a.grad + ((size_t)b * T + t0) * C;
    for (size_t e = k; e < (size_t)(t1 - t0) * C; e += NT) g[e] = 0.f;
  }
  if (a.gamma) {
    float* g = a.gamma + ((size_t)b * T + t0) * Sm;
    for (size_t e = k; e < (size_t)(t1 - t0) * Sm; e += NT) g[e] = 0.f;
  }
  const int tend = t1 < Tb ? t1 : Tb;
  double* pt = a.part ? a.part + ((size_t)b * a.tiles + blockIdx.y) * 3 * Sm : nullptr;
  if (!live || t0 >= tend) {
    if (pt)
      for (int e = k; e < 3 * Sm; e += NT) pt[e] = 0.0;
    return;
  }

  const bool chains = a.grad && ids;  // else a position is its own class, or no class sum is wanted
  if (chains) {
    // group the positions by class: nxt[i] is the next position of the class of position i
    for (int i = k; i < Sb; i += NT) {
      lab[i] = ids[i];
      has_prev[i] = 0;
    }
    __syncthreads();
    for (int i = k; i < Sb; i += NT) {
      const int v = lab[i];
      int j = i + 1;
      while (j < Sb && lab[j] != v) ++j;
      nxt[i] = (short)(j < Sb ? j : -1);
    }
    __syncthreads();
    for (int i = k; i < Sb; i += NT)
      if (nxt[i] >= 0) has_prev[nxt[i]] = 1;
  }
  global_barrier();  // the zeros are in memory before any sum is stored over them

  for (int t = t0 + w; t < tend; t += NW) {
    const float* ar = al + (size_t)t * Sm;
    const float* br = be + (size_t)t * Sm;
    float* gr = a.grad ? a.grad + ((size_t)b * T + t) * C : nullptr;
    float* gm = a.gamma ? a.gamma + ((size_t)b * T + t) * Sm : nullptr;
    // y = alpha + beta - loglik, formed in fp64: small whatever the size of the three
    auto rel = [&](int s) {
      const float av = ar[s], bv = br[s];
      const float y = (float)((double)av + (double)bv - (double)ll);
      return (av > NINF && bv > NINF) ? y : NINF;
    };
    // the frame's own normaliser LSE_s(y): 0 in exact arithmetic; in fp32 it carries the rounding
    // the frame's alpha and beta have in common, which then cancels in y - normaliser
    float m = NINF;
    for (int s = lane; s < Sb; s += 64) m = fmaxf(m, rel(s));
    m = wave_max(m);
    const float ms = m > NINF ? m : 0.f;
    float z = 0.f;
    for (int s = lane; s < Sb; s += 64) z += expf(rel(s) - ms);
    z = wave_sum(z);
    const float nt = m > NINF ? ms + logf(z) : 0.f;
    if (lane == 0) nrm[t - t0] = nt;
    auto occ = [&](int s) {
      const float g = expf(rel(s) - nt);  // exp(-inf) = 0
      if (gm) gm[s] = g;
      return g;
    };
    if (!chains) {
      for (int s = lane; s < Sb; s += 64) {
        const float g = occ(s);
        if (gr && s < C) gr[s] = g;
      }
    } else {
      for (int i = lane; i < Sb; i += 64) {
        if (has_prev[i]) continue;
        float sum = 0.f;
        for (int j = i; j >= 0; j = nxt[j]) sum += occ(j);
        const int c = lab[i];
        if (c >= 0 && c < C) gr[c] = sum;
      }
    }
  }
  if (!pt) return;

  // ---- the transition sums of this tile's frames: a thread per source position, frames in order
  __syncthreads();  // the frames' normalisers
  const int tb = t0 > 1 ? t0 : 1;
  for (int s = k; s < Sm; s += NT) {
    double acc[3] = {0.0, 0.0, 0.0};
    if (s < Sb) {
      // The transition s -> s + d at frame t has the posterior gamma[t, s + d] times its share
      // among the (up to three) candidates into s + d: exp(alpha[t-1,s] + w_d[s] - R), R their
      // LSE.  R + e[t,s+d] is alpha[t,s+d] in exact arithmetic, so this is exp(alpha[t-1,s] +
      // w_d[s] + e + beta - loglik); formed this way the share is a ratio of nearby numbers (a
      // lone candidate's is exactly 1) and no emission is read.
      // wq[d][j]: the weight of the candidate from s + d - j into s + d (j = 0 stay, 1 next, 2 skip)
      const size_t row = (size_t)b * Sm;
      float wq[3][3];
#pragma unroll
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int src = s + d - j;
          const float* wp = j == 0 ? a.w_stay : (j == 1 ? a.w_next : a.w_skip);
          wq[d][j] = (s + d < Sb && src >= 0) ? (wp ? wp[row + src] : (j == 2 ? NINF : 0.f)) : NINF;
        }
      for (int t = tb; t < tend; ++t) {
        const float* ap = al + (size_t)(t - 1) * Sm;
        const float* ar = al + (size_t)t * Sm;
        const float* br = be + (size_t)t * Sm;
        const float nt = nrm[t - t0];
        float av[5];  // alpha[t-1, s-2 .. s+2]
#pragma unroll
        for (int q = 0; q < 5; ++q) av[q] = (s + q - 2 >= 0 && s + q - 2 < Sb) ? ap[s + q - 2] : NINF;
        if (!(av[2] > NINF)) continue;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          if (s + d >= Sb || !(wq[d][d] > NINF)) continue;
          const float a1 = ar[s + d], b1 = br[s + d];
          if (!(a1 > NINF && b1 > NINF)) continue;
          const float g = expf((float)((double)a1 + (double)b1 - (double)ll) - nt);
          double cd[3], mx = -INFINITY;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            cd[j] = (double)av[2 + d - j] + (double)wq[d][j];  // -inf where there is no candidate
            mx = cd[j] > mx ? cd[j] : mx;
          }
          float p[3];
#pragma unroll
          for (int j = 0; j < 3; ++j) p[j] = expf((float)(cd[j] - mx));
          acc[d] += (double)(g * (p[d] / (p[0] + p[1] + p[2])));
        }
      }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) pt[(size_t)d * Sm + s] = acc[d];
  }
}

// the tiles' transition sums, added in tile order
__global__ void __launch_bounds__(kForcedThreads) forced_grad_combine_kernel(ForcedGradArgs a) {
  const int b = blockIdx.x, Sm = a.Smax;
  const int s = blockIdx.y * kForcedThreads + threadIdx.x;
  if (s >= Sm) return;
  double sum[3] = {0.0, 0.0, 0.0};
  for (int tile = 0; tile < a.tiles; ++tile) {
    const double* pt = a.part + ((size_t)b * a.tiles + tile) * 3 * Sm;
#pragma unroll
    for (int d = 0; d < 3; ++d) sum[d] += pt[(size_t)d * Sm + s];
  }
  const size_t o = (size_t)b * Sm + s;
  if (a.g_stay) a.g_stay[o] = (float)sum[0];
  if (a.g_next) a.g_next[o] = (float)sum[1];
  if (a.g_skip) a.g_skip[o] = (float)sum[2];
}

// the 2-bit choices of the Viterbi job, (B,T,row_bytes)
int forced_row_bytes(int Sm) {
  if (Sm <= 64) return 64;
  if (Sm <= kForcedThreads * kForcedPos) return kForcedThreads;  // P = 1, 2, 4: one byte per thread
  if (Sm <= kForcedThreads * kForcedPosMid) return kForcedThreads * ((kForcedPosMid + 3) / 4);
  return kForcedThreads * ((kForcedPosWide + 3) / 4);
}

int forced_shape_check(int B, int T, int C, int Smax) {
  if (T < 1 || B < 1 || C < 1) return HMM355_E_ARG;
  if (Smax < 1 || Smax > kForcedMax) return HMM355_E_STATES;
  const size_t lim = (size_t)1 << 46;
  size_t n;
  if (__builtin_mul_overflow((size_t)T, (size_t)B, &n) || n > lim) return HMM355_E_SHAPE;
  size_t m;
  if (__builtin_mul_overflow(n, (size_t)Smax, &m) || m > lim) return HMM355_E_SHAPE;
  if (__builtin_mul_overflow(n, (size_t)C, &m) || m > lim) return HMM355_E_SHAPE;
  return HMM355_OK;
}

constexpr unsigned kForcedFlags = HMM355_FORCED_ALPHA | HMM355_FORCED_BETA | HMM355_FORCED_VITERBI;

// 256 bytes without the Viterbi job, so that 0 always means a rejected shape
size_t forced_ws_bytes(int B, int T, int Smax, unsigned flags) {
  if (!(flags & HMM355_FORCED_VITERBI)) return 256;
  return align_up((size_t)B * T * forced_row_bytes(Smax), 256) + 256;
}

inline int forced_grad_tiles(int T) { return (T + kForcedGradRows - 1) / kForcedGradRows; }

// the gradient call's transition sums per frame tile, fp64 (B,tiles,3,Smax)
size_t forced_grad_ws_bytes(int B, int T, int Smax) {
  return align_up((size_t)B * forced_grad_tiles(T) * 3 * Smax * sizeof(double), 256) + 256;
}

template <bool PLAIN>
hipError_t forced_launch(const ForcedArgs& a, dim3 grid, hipStream_t sm) {
  constexpr int NT = kForcedThreads;
  const int S = a.Smax;
  if (S <= 64) return launch(forced_kernel<1, 64, PLAIN>, grid, dim3(64), 0, sm, a);
  if (S <= NT) return launch(forced_kernel<1, NT, PLAIN>, grid, dim3(NT), 0, sm, a);
  if (S <= NT * kForcedPosLow) return launch(forced_kernel<kForcedPosLow, NT, PLAIN>, grid, dim3(NT), 0, sm, a);
  if (S <= NT * kForcedPos) return launch(forced_kernel<kForcedPos, NT, PLAIN>, grid, dim3(NT), 0, sm, a);
  if (S <= NT * kForcedPosMid) return launch(forced_kernel<kForcedPosMid, NT, PLAIN>, grid, dim3(NT), 0, sm, a);
  return launch(forced_kernel<kForcedPosWide, NT, PLAIN>, grid, dim3(NT), 0, sm, a);
}

}  // namespace
}  // namespace hmm355

using namespace hmm355;

HMM355_API size_t hmm355_forced_workspace_bytes(int B, int T, int Smax, unsigned flags) {
  if (forced_shape_check(B, T, 1, Smax) != HMM355_OK) return 0;
  if (flags & ~(kForcedFlags | HMM355_FORCED_GRAD)) return 0;
  const size_t run = forced_ws_bytes(B, T, Smax, flags & kForcedFlags);
  const size_t grad = (flags & HMM355_FORCED_GRAD) ? forced_grad_ws_bytes(B, T, Smax) : 0;
  return run > grad ? run : grad;
}

HMM355_API int hmm355_forced_f32(const float* log_probs, const int* state_ids, const int* input_lengths,
                                 const int* state_lengths, const float* log_stay, const float* log_next,
                                 const float* log_skip, int B, int T, int C, int Smax, unsigned flags, float* alpha,
                                 float* beta, float* loglik, int* path, float* score, int* durations, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  const int rc = forced_shape_check(B, T, C, Smax);
  if (rc != HMM355_OK) return rc;
  if (!state_ids && C < Smax) return HMM355_E_ARG;
  if (flags & ~kForcedFlags) return HMM355_E_ARG;
  if (!log_probs || !input_lengths || !state_lengths || !loglik || !workspace) return HMM355_E_ARG;
  if ((flags & HMM355_FORCED_ALPHA) && !alpha) return HMM355_E_ARG;
  if ((flags & HMM355_FORCED_BETA) && !beta) return HMM355_E_ARG;
  if ((flags & HMM355_FORCED_VITERBI) && (!path || !score || !durations)) return HMM355_E_ARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return HMM355_E_ARG;
  if (workspace_bytes < forced_ws_bytes(B, T, Smax, flags)) return HMM355_E_WORKSPACE;
  ForcedArgs a{};
  a.lp = log_probs;
  a.ids = state_ids;
  a.in_len = input_lengths;
  a.st_len = state_lengths;
  a.w_stay = log_stay;
  a.w_next = log_next;
  a.w_skip = log_skip;
  a.alpha = (flags & HMM355_FORCED_ALPHA) ? alpha : nullptr;
  a.beta = (flags & HMM355_FORCED_BETA) ? beta : nullptr;
  a.loglik = loglik;
  a.path = path;
  a.score = score;
  a.dur = durations;
  a.bp = static_cast<unsigned char*>(workspace);
  a.B = B;
  a.T = T;
  a.C = C;
  a.Smax = Smax;
  int nj = 0;
  a.jobs[nj++] = kJobForward;
  if (flags & HMM355_FORCED_BETA) a.jobs[nj++] = kJobBackward;
  if (flags & HMM355_FORCED_VITERBI) a.jobs[nj++] = kJobViterbi;
  hipStream_t sm = static_cast<hipStream_t>(stream);
  const dim3 grid(B, nj);
  const bool plain = !state_ids && !log_stay && !log_next && !log_skip;
  return with_flag(plain, [&](auto p) { return forced_launch<p()>(a, grid, sm); });
}

HMM355_API int hmm355_forced_grad_f32(const float* alpha, const float* beta, const float* loglik,
                                      const int* state_ids, const int* input_lengths, const int* state_lengths,
                                      const float* log_stay, const float* log_next, const float* log_skip, int B,
                                      int T, int C, int Smax, float* gamma, float* grad_log_probs, float* grad_stay,
                                      float* grad_next, float* grad_skip, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  const int rc = forced_shape_check(B, T, C, Smax);
  if (rc != HMM355_OK) return rc;
  if (!state_ids && C < Smax) return HMM355_E_ARG;
  if (!alpha || !beta || !loglik || !input_lengths || !state_lengths) return HMM355_E_ARG;
  const bool trans = grad_stay || grad_next || grad_skip;
  if (!gamma && !grad_log_probs && !trans) return HMM355_E_ARG;
  if (forced_grad_tiles(T) > 65535) return HMM355_E_SHAPE;  // grid.y
  if (trans) {
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return HMM355_E_ARG;
    if (workspace_bytes < forced_grad_ws_bytes(B, T, Smax)) return HMM355_E_WORKSPACE;
  }
  ForcedGradArgs a{};
  a.alpha = alpha;
  a.beta = beta;
  a.loglik = loglik;
  a.ids = state_ids;
  a.in_len = input_lengths;
  a.st_len = state_lengths;
  a.w_stay = log_stay;
  a.w_next = log_next;
  a.w_skip = log_skip;
  a.gamma = gamma;
  a.grad = grad_log_probs;
  a.g_stay = grad_stay;
  a.g_next = grad_next;
  a.g_skip = grad_skip;
  a.B = B;
  a.T = T;
  a.C = C;
  a.Smax = Smax;
  a.part = trans ? static_cast<double*>(workspace) : nullptr;
  a.tiles = forced_grad_tiles(T);
  hipStream_t sm = static_cast<hipStream_t>(stream);
  HMM355_TRY(launch(forced_grad_kernel, dim3(B, a.tiles), dim3(kForcedThreads), 0, sm, a));
  if (!trans) return HMM355_OK;
  const dim3 grid(B, (Smax + kForcedThreads - 1) / kForcedThreads);
  return launch(forced_grad_combine_kernel, grid, dim3(kForcedThreads), 0, sm, a);
}
