// hmm355 — HSMM forward-backward on gfx950: the sum-product side of the explicit-duration model
// whose max-plus side is hsmm.hip / hsmm_wide.hip.  Log-likelihood, state posteriors and the
// expected duration / transition / initial counts, which are the derivatives of the
// log-likelihood with respect to lp, dur_lp, log_T and log_init (autograd.HsmmLogLik).
//
// The model (include/hmm355.h): a segmentation (s_1,d_1)..(s_K,d_K) with sum d_k = T exactly,
// 1 <= d_k <= Dmax and s_k != s_k+1 scores sum_k dur_lp[s_k,d_k-1] + (its frames' lp) +
// (k = 1 ? log_init[s_1] : log_T[s_k-1,s_k]); loglik = log sum over segmentations of exp(score).
// With O(a..t,s) the sum of lp over frames a..t:
//   begin_0(s) = log_init(s)
//   F_t(s)     = LSE_{d <= min(Dmax,t+1)} begin_{t-d+1}(s) + O(t-d+1..t,s) + dur_lp[s,d-1]
//   begin_t+1(s) = LSE_{s' != s} F_t(s') + log_T[s',s]           loglik = LSE_s F_{T-1}(s)
//   Bend_{T-1}(s) = 0;  Bend_t(s) = LSE_{s' != s} log_T[s,s'] + Bbeg_t+1(s')
//   Bbeg_t(s)  = LSE_{d <= min(Dmax,T-t)} dur_lp[s,d-1] + O(t..t+d-1,s) + Bend_{t+d-1}(s)
//
// Frame shift.  Every segmentation covers every frame once, so x_t(s) = lp_t(s) - M_t with
// M_t = max_s lp_t(s) (0 where the row has no finite maximum) changes every score by the same
// sum of M_t: the recursions run on x, the posteriors need no correction, and loglik gets the sum
// back in fp64.  Unshifted Gaussian scores (-100 .. -300 per frame) would put the fp32 tables at
// 1e5 by T = 2000.
//
// Launches of one call (each holds the whole batch; no workgroup waits on another, no flags, no
// atomics):
//   hsmm_fb_prep_kernel   M (B,T) and the two orientations of log_T with -inf diagonals.
//   hsmm_fb_chain_kernel  one workgroup per (sequence, job).  The forward and backward jobs are one
//     body: the backward recursion is the forward one on reversed time with Bend in the place of
//     begin, Bbeg in the place of F and log_T's rows in the place of its columns.  SUB lanes (a
//     power of two, inside one wave) share a state.  The Dmax open segments of a state (begin +
//     emissions so far) are a ring in LDS indexed by start time mod Dmax; a lane owns the slots
//     k = sub, sub + SUB, ..  Per step: every slot takes the frame's score (the slot of the segment
//     starting now is first set to begin), the slots are closed against dur_lp by a two-pass LSE
//     (the state's own maximum, then the sum) into F_t, ONE barrier, and begin_t+1 is the LSE over
//     predecessors with every target state's own maximum: exact whatever the spread of F_t, so a
//     dead-end state that leads by hundreds of nats costs the others nothing.  -inf candidates
//     drop out of an LSE and a cell without a finite candidate stays -inf; no NaN is formed.
//     log_T's orientation and dur_lp sit in LDS when they fit beside the ring (160 KiB), else they
//     are read from memory.  Emissions are loaded four steps ahead into a register ring.  The
//     third job (only with dur_counts) forms the fp64 prefix sums of x and the running count of
//     -inf frames per state, from which the counts kernel takes O(a..t,s) without cancellation.
//   hsmm_fb_gamma_kernel  gamma_t(s) = sum_{a<=t} P(begin a) - sum_{e<t} P(end e) as an fp64 running
//     sum of fp64 exponentials, time cut into 16 chunks per workgroup: chunk totals first, then each
//     chunk again from its offset.  Also init_post.
//   hsmm_fb_dur_kernel / hsmm_fb_trans_kernel + hsmm_fb_reduce_kernel  one thread per (s,d) or
//     (i,j) and time chunk sums its terms in time order in fp64; the chunk partials are added in
//     chunk order.  Two runs give the same bits.
#include <algorithm>

#include "launch.h"

namespace hmm355 {
namespace {

constexpr int kHfMaxStates = HMM355_HSMM_FB_MAX_STATES;
constexpr int kHfMaxDur = HMM355_HSMM_FB_MAX_DURATION;
constexpr int kHfMaxCells = HMM355_HSMM_FB_MAX_CELLS;  // S * Dmax: the ring is 64 KiB of LDS
constexpr int kHfMaxBatch = HMM355_HSMM_FB_MAX_BATCH;
constexpr int kHfAhead = 4;         // steps between an emission load and its use
constexpr int kHfGammaChunks = 16;  // waves (time chunks) per workgroup of the gamma kernel
constexpr int kHfPartCells = 16384; // counts kernels: cells x time chunks per sequence, about
constexpr int kHfMaxChunks = 32;
constexpr size_t kHfLdsBudget = 159 * 1024;
constexpr int kHfSlotBatch = 4;    // slots / predecessors a lane loads before it uses the first
constexpr int kHfPredBatch = 8;

constexpr int kJobForward = 0, kJobBackward = 1, kJobPrefix = 2;
constexpr unsigned kHfOutputs =
    HMM355_HSMM_FB_GAMMA | HMM355_HSMM_FB_DUR | HMM355_HSMM_FB_TRANS | HMM355_HSMM_FB_INIT;
constexpr unsigned kHfFlags = kHfOutputs | HMM355_FORM_GENERAL;

struct HfArgs {
  const float* lp;        // (B,T,S)
  const float* dur;       // (S,Dm)
  const float* logT;      // (S,S)
  const float* log_init;  // (S) or NULL
  float* ltF;             // (S,S): ltF[s][s'] = log_T[s'][s], -inf at s' == s
  float* ltB;             // (S,S): ltB[s][s'] = log_T[s][s'], -inf at s' == s
  float* M;               // (B,T)
  float* lls;             // (B): the log-likelihood of the shifted scores
  float* loglik;          // (B)
  float* begin;           // (B,T,S) tables, or NULL (likelihood only)
  float* F;
  float* Bend;
  float* Bbeg;
  double* P;              // (B,T,S) prefix sums of the finite x, or NULL
  int* Cinf;              // (B,T,S) -inf frames so far
  int B, T, S, Dm;
  int SUB, NT, lt_stride;
  int jobs[3];
};

__global__ void __launch_bounds__(256) hsmm_fb_prep_kernel(HfArgs a, int row_blocks) {
  const int tid = threadIdx.x;
  const float NINF = -INFINITY;
  if ((int)blockIdx.x < row_blocks) {
    const size_t row = (size_t)blockIdx.x * 4 + (tid >> 6);
    if (row >= (size_t)a.B * a.T) return;
    const float* r = a.lp + row * a.S;
    float m = NINF;
    for (int s = tid & 63; s < a.S; s += 64) m = fmaxf(m, r[s]);
    m = wave_max(m);
    if ((tid & 63) == 0) a.M[row] = (m > NINF && m < INFINITY) ? m : 0.f;
    return;
  }
  const int S = a.S;
  const int idx = ((int)blockIdx.x - row_blocks) * 256 + tid;
  if (idx >= S * S) return;
  const int i = idx / S, j = idx % S;
  a.ltB[idx] = i == j ? NINF : a.logT[idx];
  a.ltF[idx] = i == j ? NINF : a.logT[(size_t)j * S + i];
}

// fp64 prefix sums of x = lp - M over the finite frames of every state, and the count of its
// -inf frames: O(a..t,s) = P_t - P_a-1 when the counts agree, else -inf
__device__ void hf_prefix_run(const HfArgs& a) {
  const int s = threadIdx.x, b = blockIdx.x, T = a.T, S = a.S;
  if (s >= S) return;
  const float* lp = a.lp + (size_t)b * T * S;
  const float* Mb = a.M + (size_t)b * T;
  double* P = a.P + (size_t)b * T * S;
  int* C = a.Cinf + (size_t)b * T * S;
  double p = 0.0;
  int c = 0;
#pragma unroll 8
  for (int t = 0; t < T; ++t) {
    const float x = lp[(size_t)t * S + s];
    const float m = Mb[t];
    if (x == -INFINITY)
      ++c;
    else
      p += (double)x - (double)m;
    P[(size_t)t * S + s] = p;
    C[(size_t)t * S + s] = c;
  }
}

template <bool LT_LDS, bool DUR_LDS>
__device__ __forceinline__ void hf_chain_run(const HfArgs& a, const int job, float* sm) {
  constexpr int AH = kHfAhead;
  const float NINF = -INFINITY;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int T = a.T, S = a.S, Dm = a.Dm, SUB = a.SUB, NT = a.NT;
  const bool back = job == kJobBackward;
  const int s = tid / SUB, sub = tid & (SUB - 1);
  const bool live = s < S;
  const int sc = live ? s : 0;

  float* vals = sm;              // (S,Dm): the open segments, slot = start step mod Dm
  float* Fl = vals + S * Dm;     // (2,S): this step's closed values, by step parity
  float* lt_l = Fl + 2 * S;      // (S,lt_stride) when LT_LDS
  float* du_l = lt_l + (LT_LDS ? S * a.lt_stride : 0);  // (S,Dm) when DUR_LDS
  const float* ltg = back ? a.ltB : a.ltF;
  for (int e = tid; e < S * Dm; e += NT) vals[e] = NINF;
  if constexpr (LT_LDS)
    for (int e = tid; e < S * S; e += NT) lt_l[(e / S) * a.lt_stride + e % S] = ltg[e];
  if constexpr (DUR_LDS)
    for (int e = tid; e < S * Dm; e += NT) du_l[e] = a.dur[e];
  __syncthreads();
  const int lts = LT_LDS ? a.lt_stride : S;
  auto lt_at = [&](int sp) -> float { return LT_LDS ? lt_l[sc * lts + sp] : ltg[(size_t)sc * S + sp]; };
  auto du_at = [&](int di) -> float { return DUR_LDS ? du_l[sc * Dm + di] : a.dur[(size_t)sc * Dm + di]; };

  const float* lpb = a.lp + (size_t)b * T * S;
  const float* Mb = a.M + (size_t)b * T;
  float* tab_in = back ? a.Bend : a.begin;   // the value a segment opens with at this step
  float* tab_out = back ? a.Bbeg : a.F;      // the step's closed value
  if (tab_in) {
    tab_in += (size_t)b * T * S;
    tab_out += (size_t)b * T * S;
  }
  float beg = back ? 0.f : (a.log_init ? a.log_init[sc] : 0.f);
  if (!live) beg = NINF;
  double sum_m = 0.0;
  float* vrow = vals + sc * Dm;

  float xl[AH], xm[AH];
  auto load = [&](int u, float& l, float& m) __attribute__((always_inline)) {
    const int t = back ? T - 1 - u : u;
    l = lpb[(size_t)t * S + sc];
    m = Mb[t];
  };
  static_for<0, AH>([&](auto ph) {
    if (ph.value < T) load(ph.value, xl[ph.value], xm[ph.value]);
  });

  int kf = 0;  // u mod Dm: the slot of the segment that opens at this step
  auto step = [&](int u, float& l, float& m) __attribute__((always_inline)) {
    const int t = back ? T - 1 - u : u;
    const float x = l - m;
    sum_m += (double)m;
    if (u + AH < T) load(u + AH, l, m);
    const bool lead = live && sub == 0;
    if (tab_in && lead) tab_in[(size_t)t * S + s] = beg;
    // Every open segment takes the frame; the candidates' maximum.  Slots and predecessors go in
    // whole batches whose loads all come before the first store or use, then one at a time: a
    // plain loop waits a whole LDS (or L2) round trip per slot, because the compiler must keep a
    // slot's store ahead of the next slot's loads.
    auto dur_of = [&](int k) {  // duration - 1 of the segment in slot k
      const int di = kf - k;
      return di + (di < 0 ? Dm : 0);
    };
    constexpr int SB = kHfSlotBatch, PB = kHfPredBatch;
    float mx = NINF;
    if (live) {
      int k0 = sub;
      for (; k0 + (SB - 1) * SUB < Dm; k0 += SB * SUB) {
        float v[SB], dd[SB];
#pragma unroll
        for (int j = 0; j < SB; ++j) {
          const int k = k0 + j * SUB;
          v[j] = vrow[k];
          v[j] = k == kf ? beg : v[j];
          dd[j] = du_at(dur_of(k));
        }
#pragma unroll
        for (int j = 0; j < SB; ++j) {
          v[j] += x;
          vrow[k0 + j * SUB] = v[j];
          mx = fmaxf(mx, v[j] + dd[j]);
        }
      }
      for (int k = k0; k < Dm; k += SUB) {
        float v = k == kf ? beg : vrow[k];
        v += x;
        vrow[k] = v;
        mx = fmaxf(mx, v + du_at(dur_of(k)));
      }
    }
    mx = grp_max_rt(mx, SUB);
    const float ms = mx == NINF ? 0.f : mx;
    float sum = 0.f;
    if (live) {
      int k0 = sub;
      for (; k0 + (SB - 1) * SUB < Dm; k0 += SB * SUB) {
        float c[SB];
#pragma unroll
        for (int j = 0; j < SB; ++j) c[j] = vrow[k0 + j * SUB] + du_at(dur_of(k0 + j * SUB));
#pragma unroll
        for (int j = 0; j < SB; ++j) sum += expf(c[j] - ms);
      }
      for (int k = k0; k < Dm; k += SUB) sum += expf(vrow[k] + du_at(dur_of(k)) - ms);
    }
    sum = grp_sum_rt(sum, SUB);
    const float Fv = mx == NINF ? NINF : ms + logf(sum);
    if (lead) {
      Fl[(u & 1) * S + s] = Fv;
      if (tab_out) tab_out[(size_t)t * S + s] = Fv;
    }
    lds_barrier();
    kf = kf + 1 == Dm ? 0 : kf + 1;
    if (u + 1 < T) {
      // the next step's opening value: LSE over the other states with this state's own maximum
      const float* Fr = Fl + (u & 1) * S;
      float m2 = NINF, s2 = 0.f;
      if (live) {
        int p0 = sub;
        for (; p0 + (PB - 1) * SUB < S; p0 += PB * SUB) {
          float c[PB];
#pragma unroll
          for (int j = 0; j < PB; ++j) c[j] = Fr[p0 + j * SUB] + lt_at(p0 + j * SUB);
#pragma unroll
          for (int j = 0; j < PB; ++j) m2 = fmaxf(m2, c[j]);
        }
        for (int sp = p0; sp < S; sp += SUB) m2 = fmaxf(m2, Fr[sp] + lt_at(sp));
      }
      m2 = grp_max_rt(m2, SUB);
      const float ms2 = m2 == NINF ? 0.f : m2;
      if (live) {
        int p0 = sub;
        for (; p0 + (PB - 1) * SUB < S; p0 += PB * SUB) {
          float c[PB];
#pragma unroll
          for (int j = 0; j < PB; ++j) c[j] = Fr[p0 + j * SUB] + lt_at(p0 + j * SUB);
#pragma unroll
          for (int j = 0; j < PB; ++j) s2 += expf(c[j] - ms2);
        }
        for (int sp = p0; sp < S; sp += SUB) s2 += expf(Fr[sp] + lt_at(sp) - ms2);
      }
      s2 = grp_sum_rt(s2, SUB);
      beg = (m2 == NINF || !live) ? NINF : ms2 + logf(s2);
    }
  };

  for (int u0 = 0; u0 < T; u0 += AH)
    static_for<0, AH>([&](auto ph) {
      if (u0 + ph.value < T) step(u0 + ph.value, xl[ph.value], xm[ph.value]);
    });

  if (back || tid >= 64) return;
  // loglik = LSE_s F_{T-1}(s) + sum of M (the last step's barrier published the row)
  const float* Fr = Fl + ((T - 1) & 1) * S;
  float m = NINF;
  for (int sp = tid; sp < S; sp += 64) m = fmaxf(m, Fr[sp]);
  m = wave_max(m);
  const float ms = m == NINF ? 0.f : m;
  float sum = 0.f;
  for (int sp = tid; sp < S; sp += 64) sum += expf(Fr[sp] - ms);
  sum = wave_sum(sum);
  if (tid == 0) {
    const float ll = m == NINF ? NINF : ms + logf(sum);
    a.lls[b] = ll;
    a.loglik[b] = m == NINF ? NINF : (float)((double)ll + sum_m);
  }
}

template <bool LT_LDS, bool DUR_LDS>
__global__ void __launch_bounds__(1024) hsmm_fb_chain_kernel(HfArgs a) {
  extern __shared__ __attribute__((aligned(16))) float hf_sm[];
  const int job = a.jobs[blockIdx.y];
  if (job == kJobPrefix)
    hf_prefix_run(a);
  else
    hf_chain_run<LT_LDS, DUR_LDS>(a, job, hf_sm);
}

// ------------------------------------------------------------------ posteriors and counts
struct HfCountArgs {
  const float* begin;   // (B,T,S)
  const float* F;
  const float* Bend;
  const float* Bbeg;
  const float* lls;     // (B)
  const float* dur;     // (S,Dm)
  const float* ltB;     // (S,S), -inf diagonal
  const float* log_init;
  const double* P;
  const int* Cinf;
  float* gamma;         // (B,T,S) or NULL
  float* init_post;     // (B,S) or NULL
  double* part;         // (B,chunks,cells) partial sums of the counts kernel in flight
  int B, T, S, Dm, chunks;
};

__global__ void __launch_bounds__(64 * kHfGammaChunks) hsmm_fb_gamma_kernel(HfCountArgs a) {
  __shared__ double tot[kHfGammaChunks][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.y, T = a.T, S = a.S;
  const float NINF = -INFINITY;
  const float llf = a.lls[b];
  const bool feasible = llf > NINF;
  const double ll = feasible ? (double)llf : 0.0;
  const size_t off = (size_t)b * T * S;
  if (a.init_post && blockIdx.x == 0 && tid < S) {
    const float li = a.log_init ? a.log_init[tid] : 0.f;
    const float bb = a.Bbeg[off + tid];
    a.init_post[(size_t)b * S + tid] =
        (feasible && li > NINF && bb > NINF) ? (float)exp((double)li + (double)bb - ll) : 0.f;
  }
  if (!a.gamma) return;
  const int s = blockIdx.x * 64 + lane;
  const bool live = s < S;
  const int sc = live ? s : S - 1;
  const float* bg = a.begin + off + sc;
  const float* bb = a.Bbeg + off + sc;
  const float* fe = a.F + off + sc;
  const float* be = a.Bend + off + sc;
  float* g = a.gamma + off + sc;
  const int C = (T + kHfGammaChunks - 1) / kHfGammaChunks;
  const int t0 = w * C, t1 = t0 + C < T ? t0 + C : T;
  if (!feasible) {
    if (live)
      for (int t = t0; t < t1; ++t) g[(size_t)t * S] = 0.f;
    return;
  }
  // P(a segment of s begins at t) - P(a segment of s ended at t - 1)
  auto delta = [&](int t) -> double {
    const float x0 = bg[(size_t)t * S], x1 = bb[(size_t)t * S];
    double d = (x0 > NINF && x1 > NINF) ? exp((double)x0 + (double)x1 - ll) : 0.0;
    if (t > 0) {
      const float y0 = fe[(size_t)(t - 1) * S], y1 = be[(size_t)(t - 1) * S];
      if (y0 > NINF && y1 > NINF) d -= exp((double)y0 + (double)y1 - ll);
    }
    return d;
  };
  double acc = 0.0;
  for (int t = t0; t < t1; ++t) acc += delta(t);
  tot[w][lane] = acc;
  __syncthreads();
  double run = 0.0;
  for (int k = 0; k < w; ++k) run += tot[k][lane];
  for (int t = t0; t < t1; ++t) {
    run += delta(t);
    if (live) g[(size_t)t * S] = (float)run;
  }
}

// expected number of (s,d) segments: one thread per (s,d) and time chunk, ends t ascending
__global__ void __launch_bounds__(256) hsmm_fb_dur_kernel(HfCountArgs a) {
  const int T = a.T, S = a.S, Dm = a.Dm, b = blockIdx.z, c = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;  // d * S + s: a wave reads along s
  if (idx >= S * Dm) return;
  const float NINF = -INFINITY;
  const int s = idx % S, d = idx / S;  // duration d + 1
  const float llf = a.lls[b];
  const float du = a.dur[(size_t)s * Dm + d];
  const int TC = (T + a.chunks - 1) / a.chunks;
  int t0 = c * TC;
  const int t1 = t0 + TC < T ? t0 + TC : T;
  if (t0 < d) t0 = d;
  double acc = 0.0;
  if (llf > NINF && du > NINF) {
    const size_t off = (size_t)b * T * S + s;
    const double base = (double)du - (double)llf;
    for (int t = t0; t < t1; ++t) {
      const int st = t - d;
      const float x0 = a.begin[off + (size_t)st * S], x1 = a.Bend[off + (size_t)t * S];
      const double pt = a.P[off + (size_t)t * S];
      const int ct = a.Cinf[off + (size_t)t * S];
      const double pa = st > 0 ? a.P[off + (size_t)(st - 1) * S] : 0.0;
      const int ca = st > 0 ? a.Cinf[off + (size_t)(st - 1) * S] : 0;
      if (x0 > NINF && x1 > NINF && ct == ca)
        acc += (double)expf((float)((double)x0 + (pt - pa) + (double)x1 + base));
    }
  }
  a.part[((size_t)b * a.chunks + c) * S * Dm + idx] = acc;
}

// expected number of i -> j transitions: one thread per (i,j) and time chunk
__global__ void __launch_bounds__(256) hsmm_fb_trans_kernel(HfCountArgs a) {
  const int T = a.T, S = a.S, b = blockIdx.z, c = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= S * S) return;
  const float NINF = -INFINITY;
  const int i = idx / S, j = idx % S;
  const float llf = a.lls[b];
  const float lt = a.ltB[idx];
  const int TC = (T - 1 + a.chunks - 1) / a.chunks;
  const int t0 = c * TC;
  const int t1 = t0 + TC < T - 1 ? t0 + TC : T - 1;
  double acc = 0.0;
  if (llf > NINF && lt > NINF) {
    const size_t off = (size_t)b * T * S;
    const double base = (double)lt - (double)llf;
    for (int t = t0; t < t1; ++t) {
      const float x0 = a.F[off + (size_t)t * S + i], x1 = a.Bbeg[off + (size_t)(t + 1) * S + j];
      if (x0 > NINF && x1 > NINF) acc += (double)expf((float)((double)x0 + (double)x1 + base));
    }
  }
  a.part[((size_t)b * a.chunks + c) * S * S + idx] = acc;
}

// out[b][cell] = the chunk partials in chunk order; cols > 0: the partials are (rows, cols) with
// the output transposed to (cols, rows)
__global__ void __launch_bounds__(256) hsmm_fb_reduce_kernel(const double* part, float* out, int cells, int chunks,
                                                           int cols) {
  const int idx = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (idx >= cells) return;
  double acc = 0.0;
  for (int c = 0; c < chunks; ++c) acc += part[((size_t)b * chunks + c) * cells + idx];
  const int o = cols > 0 ? (idx % cols) * (cells / cols) + idx / cols : idx;
  out[(size_t)b * cells + o] = (float)acc;
}

// ------------------------------------------------------------------ host side
int hf_chunks(int cells, int T) {
  int c = (kHfPartCells + cells - 1) / cells;
  c = c < kHfMaxChunks ? c : kHfMaxChunks;
  const int by_t = (T + 15) / 16;  // at least 16 frames a chunk
  c = c < by_t ? c : by_t;
  return c < 1 ? 1 : c;
}

int hf_shape_check(int B, int T, int S, int Dm) {
  if (B < 0 || S < 0 || Dm < 0) return HMM355_E_ARG;
  if (S < 1 || S > kHfMaxStates) return HMM355_E_STATES;
  if (Dm < 1 || Dm > kHfMaxDur || S * Dm > kHfMaxCells) return HMM355_E_DURATION;
  if (T < 1) return HMM355_E_SHAPE;
  // a sequence is a grid row of the counts kernels (gridDim.y / .z stop at 65535) and B * T rows
  // are counted in an int by the prep launch
  if (B > kHfMaxBatch) return HMM355_E_SHAPE;
  size_t n, m;
  if (__builtin_mul_overflow((size_t)(B > 0 ? B : 1), (size_t)T, &n) || n > ((size_t)1 << 31)) return HMM355_E_SHAPE;
  if (__builtin_mul_overflow(n, (size_t)S, &m) || m > ((size_t)1 << 40)) return HMM355_E_SHAPE;
  if ((size_t)T * S > ((size_t)1 << 30)) return HMM355_E_SHAPE;  // per-sequence offsets are ints in places
  return HMM355_OK;
}

// (pieces an output flag does not ask for are not carved and stay null; 256 bytes of slack end it)
struct HfLayout {
  float *ltF, *ltB, *M, *lls, *tab[4];
  double* P;
  int* Cinf;
  double* part;
  size_t total;
  int cd, ct;
};

HfLayout hf_layout(int B, int T, int S, int Dm, unsigned flags, char* base) {
  HfLayout L{};
  Carver c{base};
  const size_t n = (size_t)B * T * S;
  L.ltF = c.take<float>((size_t)S * S);
  L.ltB = c.take<float>((size_t)S * S);
  L.M = c.take<float>((size_t)B * T);
  L.lls = c.take<float>(B);
  if (flags & kHfOutputs)
    for (int k = 0; k < 4; ++k) L.tab[k] = c.take<float>(n);
  L.cd = hf_chunks(S * Dm, T);
  L.ct = hf_chunks(S * S, T);
  if (flags & HMM355_HSMM_FB_DUR) {
    L.P = c.take<double>(n);
    L.Cinf = c.take<int>(n);
  }
  size_t part = 0;  // (doubles)
  if (flags & HMM355_HSMM_FB_DUR) part = (size_t)B * L.cd * S * Dm;
  if (flags & HMM355_HSMM_FB_TRANS) part = std::max(part, (size_t)B * L.ct * S * S);
  L.part = c.take<double>(part);
  L.total = c.bytes() + 256;
  return L;
}

}  // namespace
}  // namespace hmm355

using namespace hmm355;

HMM355_API size_t hmm355_hsmm_fb_workspace_bytes(int B, int T, int S, int Dmax, unsigned flags) {
  if (hf_shape_check(B, T, S, Dmax) != HMM355_OK || (flags & ~kHfFlags)) return 0;
  return hf_layout(B, T, S, Dmax, flags, nullptr).total;
}

HMM355_API int hmm355_hsmm_fb_f32(const float* lp, const float* dur_lp, const float* log_T, const float* log_init,
                                  int B, int T, int S, int Dmax, unsigned flags, float* loglik, float* gamma,
                                  float* dur_counts, float* trans_counts, float* init_post, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (flags & ~kHfFlags) return HMM355_E_ARG;
  const int rc = hf_shape_check(B, T, S, Dmax);
  if (rc != HMM355_OK) return rc;
  if (B == 0) return HMM355_OK;
  if (!lp || !dur_lp || !log_T || !loglik || !workspace) return HMM355_E_ARG;
  if ((flags & HMM355_HSMM_FB_GAMMA) && !gamma) return HMM355_E_ARG;
  if ((flags & HMM355_HSMM_FB_DUR) && !dur_counts) return HMM355_E_ARG;
  if ((flags & HMM355_HSMM_FB_TRANS) && !trans_counts) return HMM355_E_ARG;
  if ((flags & HMM355_HSMM_FB_INIT) && !init_post) return HMM355_E_ARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return HMM355_E_ARG;
  const HfLayout L = hf_layout(B, T, S, Dmax, flags, static_cast<char*>(workspace));
  if (workspace_bytes < L.total) return HMM355_E_WORKSPACE;

  const bool tables = flags & kHfOutputs;
  HfArgs a{};
  a.lp = lp;
  a.dur = dur_lp;
  a.logT = log_T;
  a.log_init = log_init;
  a.ltF = L.ltF;
  a.ltB = L.ltB;
  a.M = L.M;
  a.lls = L.lls;
  a.loglik = loglik;
  a.begin = L.tab[0];
  a.F = L.tab[1];
  a.Bend = L.tab[2];
  a.Bbeg = L.tab[3];
  a.P = L.P;
  a.Cinf = L.Cinf;
  a.B = B;
  a.T = T;
  a.S = S;
  a.Dm = Dmax;
  // lanes per state: a power of two inside one wave, as many as 1024 threads hold and the longer
  // of a state's two loops (Dmax slots, S predecessors) has work for.  A step is a chain of LDS
  // round trips, exponentials and reductions, not throughput: at S = 64, Dmax = 40, T = 2000,
  // B = 16 the forward sum took 29.2 / 16.4 / 8.7 / 5.4 / 4.5 ms with 1 / 2 / 4 / 8 / 16 lanes.
  int sub = 64;
  while (sub > 1 && S * sub > 1024) sub >>= 1;
  while (sub > 1 && (sub >> 1) >= std::max(S, Dmax)) sub >>= 1;
  a.SUB = sub;
  a.NT = (S * sub + 63) / 64 * 64;
  a.lt_stride = S + sub;
  int nj = 0;
  a.jobs[nj++] = kJobForward;
  if (tables) a.jobs[nj++] = kJobBackward;
  if (flags & HMM355_HSMM_FB_DUR) a.jobs[nj++] = kJobPrefix;

  hipStream_t st = static_cast<hipStream_t>(stream);
  const int row_blocks = (int)(((size_t)B * T + 3) / 4);
  HMM355_TRY(launch(hsmm_fb_prep_kernel, dim3(row_blocks + (S * S + 255) / 256), dim3(256), 0, st, a, row_blocks));

  size_t lds = ((size_t)S * Dmax + 2 * (size_t)S) * 4;
  const size_t lt_bytes = (size_t)S * a.lt_stride * 4, du_bytes = (size_t)S * Dmax * 4;
  const bool lt_lds = lds + lt_bytes <= kHfLdsBudget;
  if (lt_lds) lds += lt_bytes;
  // without log_T the ring and dur_lp always fit (2 * 64 KiB + 2 KiB): three placements
  const bool du_lds = lds + du_bytes <= kHfLdsBudget;
  if (du_lds) lds += du_bytes;
  static_assert(2 * (size_t)kHfMaxCells * 4 + 2 * (size_t)kHfMaxStates * 4 <= kHfLdsBudget, "ring + dur_lp fit");
  const dim3 grid(B, nj), block(a.NT);
  if (lt_lds && du_lds)
    HMM355_TRY(launch(hsmm_fb_chain_kernel<true, true>, grid, block, lds, st, a));
  else if (lt_lds)
    HMM355_TRY(launch(hsmm_fb_chain_kernel<true, false>, grid, block, lds, st, a));
  else
    HMM355_TRY(launch(hsmm_fb_chain_kernel<false, true>, grid, block, lds, st, a));
  if (!tables) return HMM355_OK;

  HfCountArgs c{};
  c.begin = a.begin;
  c.F = a.F;
  c.Bend = a.Bend;
  c.Bbeg = a.Bbeg;
  c.lls = a.lls;
  c.dur = dur_lp;
  c.ltB = a.ltB;
  c.log_init = log_init;
  c.P = a.P;
  c.Cinf = a.Cinf;
  c.gamma = (flags & HMM355_HSMM_FB_GAMMA) ? gamma : nullptr;
  c.init_post = (flags & HMM355_HSMM_FB_INIT) ? init_post : nullptr;
  c.part = L.part;
  c.B = B;
  c.T = T;
  c.S = S;
  c.Dm = Dmax;
  if (c.gamma || c.init_post) {
    const int gx = c.gamma ? (S + 63) / 64 : 1;
    HMM355_TRY(launch(hsmm_fb_gamma_kernel, dim3(gx, B), dim3(64 * kHfGammaChunks), 0, st, c));
  }
  if (flags & HMM355_HSMM_FB_DUR) {
    const int cells = S * Dmax;
    c.chunks = L.cd;
    HMM355_TRY(launch(hsmm_fb_dur_kernel, dim3((cells + 255) / 256, L.cd, B), dim3(256), 0, st, c));
    HMM355_TRY(launch(hsmm_fb_reduce_kernel, dim3((cells + 255) / 256, B), dim3(256), 0, st, c.part, dur_counts,
                      cells, L.cd, S));
  }
  if (flags & HMM355_HSMM_FB_TRANS) {
    const int cells = S * S;
    c.chunks = L.ct;
    HMM355_TRY(launch(hsmm_fb_trans_kernel, dim3((cells + 255) / 256, L.ct, B), dim3(256), 0, st, c));
    HMM355_TRY(launch(hsmm_fb_reduce_kernel, dim3((cells + 255) / 256, B), dim3(256), 0, st, c.part, trans_counts,
                      cells, L.ct, 0));
  }
  return HMM355_OK;
}
