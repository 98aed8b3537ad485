// hmm355 — explicit-duration forced alignment: an utterance against its own transcript chain,
// every position with its own duration distribution.  Forward sum (log-likelihood), backward sum,
// max-plus forward with its walk (best segmentation), posteriors, expected duration counts and the
// emission gradient.
//
// The model (include/hmm355.h).  Sequence b has T_b frames and L_b positions in transcript order;
// position l emits class id_l = state_ids[b,l] (or l itself without ids) and lasts d_l frames,
// 1 <= d_l <= Dmax, scored dur_lp[b,l,d_l-1]; every position is visited once, in order, and
// sum d_l = T_b exactly.  With O(a..t,l) the sum of position l's emissions over frames a..t:
//   begin_0(0) = 0, begin_0(l>0) = -inf, begin_t(0) = -inf for t > 0
//   F_t(l)     = OP_{d <= min(Dmax,t+1)} begin_{t-d+1}(l) + O(t-d+1..t,l) + dur_lp[l,d-1]
//   begin_t+1(l+1) = F_t(l)                      result = F_{T_b-1}(L_b-1)
//   Bend_{T_b-1}(L_b-1) = 0;  Bend_t(l) = Bbeg_t+1(l+1)
//   Bbeg_t(l)  = LSE_d dur_lp[l,d-1] + O(t..t+d-1,l) + Bend_{t+d-1}(l)
// OP is LSE for the sums and max for Viterbi (the smaller d wins a tie).
//
// Frame shift.  Every segmentation covers every frame once, so x_t(l) = lp_t(l) - M_t with M_t the
// maximum over the chain's positions at frame t (0 where there is no finite one) changes every
// score by the same sum of M_t: the recursions run on x, the posteriors need no correction, and
// loglik / score get the sum back in fp64.
//
// durforced_chain_kernel: one launch per call, the whole batch in it, one workgroup per (sequence,
// job): forward sum (always), backward sum (HMM355_DURFORCED_TABLES), max-plus forward with its
// walk (HMM355_DURFORCED_VITERBI).  No workgroup waits on another; no flags, no atomics.  The
// backward job is the forward body on reversed time and reversed positions (p = L_b - 1 - l), with
// Bend in the place of begin and Bbeg in the place of F.  A workgroup first forms its own M_t (a
// wave per frame), then runs the chain:
//   SUB lanes (a power of two, inside one wave) own a position.  Its up-to-Dmax open segments
//   (begin + emissions so far) are a ring in LDS indexed by start step mod Dmax; a lane owns the
//   slots sub, sub + SUB, .. and no other lane touches them.  Per step every slot takes the frame's
//   score (the slot of the segment starting now is first set to begin), the slots are closed
//   against dur_lp (in LDS beside the ring; both with a row stride that keeps a half wave's 32
//   words in 32 banks, df_row_stride) into F_t(l): a two-pass LSE with the position's own
//   maximum (the candidates of a lane's first kDfKeep batches of slots stay in registers between
//   the passes, the rest are read again), or a max / first-argmax; ONE barrier; and begin_t+1 is
//   the left neighbour's F_t, through LDS double-buffered by step parity, or by lane shuffles (no
//   barrier at all) when the chain sits in one wave.  There is no predecessor reduction.
//   Emissions are a gather lp[b,t,id_l], issued kDfAhead steps ahead into a register ring with
//   the frame's M_t.  A class outside [0, C) reads as -inf and is never dereferenced.  -inf
//   candidates drop out of an LSE and a cell without a finite candidate stays -inf; no NaN.
//   Viterbi keeps the chosen d - 1 as one byte per cell in the workspace; lane 0 walks it back from
//   (T_b-1, L_b-1) through windows of kDfWalkRows x kDfWalkCols cells staged in LDS and writes
//   durations and path.
// Gradient (three launches; the tables are those of one forward call):
//   durforced_gamma_kernel  gamma_t(l) = sum_{a<=t} P(begin a) - sum_{e<t} P(end e) as an fp64
//     running sum of fp64 exponentials of the fp32 tables, time cut into 16 chunks per workgroup:
//     chunk totals first, then each chunk again from its offset.  Further workgroups of the same
//     launch form the fp64 prefix sums of x and the running count of -inf frames per position, from
//     which the counts kernel takes O(a..t,l) without cancellation.
//   durforced_count_kernel  one thread per (l,d) and time chunk sums exp(begin + O + dur_lp + Bend
//     - loglik) over its ends t in time order (fp64).
//   durforced_reduce_kernel adds the chunk partials in chunk order, and (further workgroups) forms
//     d loglik / d log_probs: the positions of a class are grouped once per workgroup ("next
//     position of the same class" links in LDS) and one lane sums a class's chain of gammas in
//     position order.  No atomics anywhere: two runs give the same bits.
#include "launch.h"

namespace hmm355 {
namespace {

constexpr int kDfMaxPos = HMM355_DURFORCED_MAX_POSITIONS;
constexpr int kDfMaxDur = HMM355_DURFORCED_MAX_DURATION;
constexpr int kDfMaxCells = HMM355_DURFORCED_MAX_CELLS;  // Lmax * Dmax: the ring is 64 KiB of LDS (unpadded)
constexpr int kDfMaxThreads = 1024;
constexpr int kDfAhead = 4;          // steps between an emission gather and its use
constexpr int kDfSlotBatch = 4;      // slots a lane loads before it uses the first
constexpr int kDfKeep = 4;           // batches of a lane whose candidates stay in registers between the passes
constexpr int kDfWalkRows = 64;      // backtrace window: frames
constexpr int kDfWalkCols = 64;      // ... and positions
constexpr int kDfGammaChunks = 16;   // waves (time chunks) per workgroup of the gamma kernel
constexpr int kDfPartCells = 16384;  // counts kernel: cells x time chunks per sequence, about
constexpr int kDfMaxChunks = 32;
constexpr int kDfClassRows = 32;     // frames per class-sum workgroup of the reduce launch
constexpr size_t kDfLdsBudget = 159 * 1024;
static_assert(kDfMaxDur <= 256, "a cell's choice is one byte");
static_assert(kDfMaxPos <= kDfMaxThreads, "a position has at least one lane");

constexpr int kJobForward = 0, kJobBackward = 1, kJobViterbi = 2;
constexpr unsigned kDfFlags = HMM355_DURFORCED_TABLES | HMM355_DURFORCED_VITERBI;

struct DfArgs {
  const float* lp;      // (B,T,C)
  const int* ids;       // (B,Lm) or NULL
  const int* in_len;    // (B)
  const int* st_len;    // (B)
  const float* dur;     // (B,Lm,Dm)
  float* begin;         // (B,T,Lm) tables, or NULL (likelihood only)
  float* F;
  float* Bend;
  float* Bbeg;
  float* shift;         // (B,T): M_t, with the tables
  float* lls;           // (B): the log-likelihood of the shifted scores, with the tables
  float* loglik;        // (B)
  int* path;            // (B,T)
  float* score;         // (B)
  int* durs;            // (B,Lm)
  float* M;             // (3,B,T): every job's own M_t
  unsigned char* bp;    // (B,T,Lm): the Viterbi job's chosen d - 1
  int B, T, C, Lm, Dm;
  int SUB, NT, DS;      // lanes per position, threads, row stride of the ring and of dur_lp in LDS
  int jobs[3];
};

// Row stride of the ring and of dur_lp in LDS: the smallest DS >= Dmax that is an odd multiple of
// `sub`.  The 32 lanes of a half wave are 32 / sub positions times sub consecutive slots; their rows
// then start sub banks apart and the half wave's 32 words sit in 32 different banks (with the
// plain stride Dmax = 64 every row would start in bank 0).  From 32 lanes a position a half wave
// is one row of consecutive slots whatever the stride.
__host__ __device__ constexpr int df_row_stride(int Dm, int sub) {
  if (sub > 16) return Dm;
  const int m = 2 * sub;
  return Dm + (sub - Dm % m + m) % m;
}

// LDS of the chain kernel, in floats from the 16-byte aligned base
struct DfCarve {
  int vals, dur, fl, cls, win, misc, total;
};
__host__ __device__ constexpr int df_up4(int n) { return (n + 3) / 4 * 4; }
__host__ __device__ constexpr DfCarve df_carve(int Lm, int DS) {
  DfCarve c{};
  constexpr auto up = df_up4;
  c.vals = 0;
  c.dur = up(Lm * DS);
  c.fl = c.dur + up(Lm * DS);
  c.cls = c.fl + up(2 * (Lm + 1));
  c.win = c.cls + up(Lm);
  c.misc = c.win + kDfWalkRows * kDfWalkCols / 4;
  c.total = c.misc + 4;
  return c;
}

template <bool VIT, bool WAVE>
__device__ __forceinline__ void df_chain_run(const DfArgs& a, const int job, float* sm) {
  constexpr int AH = kDfAhead;
  const float NINF = -INFINITY;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int T = a.T, C = a.C, Lm = a.Lm, Dm = a.Dm, SUB = a.SUB, NT = a.NT, DS = a.DS;
  const int NW = NT >> 6;
  const int Tb = clamp_int(a.in_len[b], 1, T);
  const int Lb = clamp_int(a.st_len[b], 1, Lm);
  const bool back = job == kJobBackward;
  const int p = tid / SUB, sub = tid & (SUB - 1);  // p: the position in the job's own order
  const bool live = p < Lb;
  const int l = live ? (back ? Lb - 1 - p : p) : 0;

  const DfCarve cv = df_carve(Lm, DS);
  float* vals = sm + cv.vals;   // (Lm,DS): the open segments, slot = start step mod Dm
  float* du_l = sm + cv.dur;    // (Lm,DS): dur_lp of this sequence
  float* Fl = sm + cv.fl;       // (2,Lm+1): slot p + 1 = this step's F of position p, by step parity
  int* cls = reinterpret_cast<int*>(sm + cv.cls);
  unsigned char* win = reinterpret_cast<unsigned char*>(sm + cv.win);
  float* fin = sm + cv.misc;
  int* wpos = reinterpret_cast<int*>(sm + cv.misc + 1);

  const float* lpb = a.lp + (size_t)b * T * C;
  const float* dub = a.dur + (size_t)b * Lm * Dm;
  for (int e = tid; e < Lm * DS; e += NT) {
    const int r = e / DS, d = e - r * DS;
    vals[e] = NINF;
    du_l[e] = (r < Lb && d < Dm) ? dub[(size_t)r * Dm + d] : NINF;
  }
  for (int e = tid; e < 2 * (Lm + 1); e += NT) Fl[e] = NINF;
  for (int i = tid; i < Lm; i += NT) {
    const int c = a.ids ? a.ids[(size_t)b * Lm + i] : i;
    cls[i] = (i < Lb && c >= 0 && c < C) ? c : -1;
  }
  if (tid == 0) fin[0] = NINF;

  float* tab_in = VIT ? nullptr : (back ? a.Bend : a.begin);  // the value a segment opens with
  float* tab_out = VIT ? nullptr : (back ? a.Bbeg : a.F);     // the step's closed value
  if (tab_in) {
    tab_in += (size_t)b * T * Lm;
    tab_out += (size_t)b * T * Lm;
    // cells no step writes: frames >= T_b and positions >= L_b
    const size_t lo = (size_t)Tb * Lm, hi = (size_t)T * Lm;
    for (size_t e = lo + tid; e < hi; e += NT) tab_in[e] = tab_out[e] = NINF;
    if (Lb < Lm) {
      const int w = Lm - Lb;
      for (size_t e = tid; e < (size_t)Tb * w; e += NT) {
        const size_t at = (e / w) * Lm + Lb + (e % w);
        tab_in[at] = tab_out[at] = NINF;
      }
    }
  }
  __syncthreads();

  // M_t of this sequence: a wave per frame; the forward job's is the shift table when one is kept
  const bool keep = job == kJobForward && a.shift;
  float* Mj = keep ? a.shift + (size_t)b * T : a.M + ((size_t)job * a.B + b) * T;
  for (int t = wave; t < Tb; t += NW) {
    const float* row = lpb + (size_t)t * C;
    float m = NINF;
    for (int i = lane; i < Lb; i += 64) {
      const int c = cls[i];
      if (c >= 0) m = fmaxf(m, row[c]);
    }
    m = wave_max(m);
    if (lane == 0) Mj[t] = m > NINF ? m : 0.f;
  }
  if (keep)
    for (int t = Tb + tid; t < T; t += NT) Mj[t] = 0.f;
  global_barrier();

  const int myc = live ? cls[l] : -1;
  float* vrow = vals + l * DS;
  const float* drow = du_l + l * DS;
  unsigned char* bp = VIT ? a.bp + (size_t)b * T * Lm : nullptr;
  float beg = (live && p == 0) ? 0.f : NINF;
  double sum_m = 0.0;

  float xe[AH], xm[AH];
  auto load = [&](int u, float& e, float& m) __attribute__((always_inline)) {
    const int t = back ? Tb - 1 - u : u;
    e = myc >= 0 ? lpb[(size_t)t * C + myc] : NINF;
    m = Mj[t];
  };
  static_for<0, AH>([&](auto ph) {
    if (ph.value < Tb) load(ph.value, xe[ph.value], xm[ph.value]);
  });

  int kf = 0;  // u mod Dm: the slot of the segment that opens at this step
  auto step = [&](int u, float& e, float& m) __attribute__((always_inline)) {
    const int t = back ? Tb - 1 - u : u;
    const float x = e - m;
    sum_m += (double)m;
    if (u + AH < Tb) load(u + AH, e, m);
    const bool lead = live && sub == 0;
    if (tab_in && lead) tab_in[(size_t)t * Lm + l] = beg;
    auto dur_of = [&](int k) {  // duration - 1 of the segment in slot k
      const int di = kf - k;
      return di + (di < 0 ? Dm : 0);
    };
    // Every open segment takes the frame; the candidates' maximum.  Slots go in whole batches
    // whose loads all come before the first store, then one at a time.
    constexpr int SB = kDfSlotBatch;
    float mx = NINF;
    int bd = 0;
    auto cand = [&](float c, int di) __attribute__((always_inline)) {
      if (VIT) {
        const bool take = (c > mx) | ((c == mx) & (di < bd));
        mx = take ? c : mx;
        bd = take ? di : bd;
      } else {
        mx = fmaxf(mx, c);
      }
    };
    // the candidates of a lane's first kDfKeep batches stay in registers for the second pass
    constexpr int KB = kDfKeep;
    float kept[KB][SB];
    int nk = 0;    // how many of them this lane has (its whole batches, up to KB)
    int kc = sub;  // the first slot past them
    if (live) {
      int k0 = sub;
      auto batch = [&](float (&c)[SB]) __attribute__((always_inline)) {
        float v[SB], dd[SB];
        int di[SB];
#pragma unroll
        for (int j = 0; j < SB; ++j) {
          const int k = k0 + j * SUB;
          v[j] = vrow[k];
          v[j] = k == kf ? beg : v[j];
          di[j] = dur_of(k);
          dd[j] = drow[di[j]];
        }
#pragma unroll
        for (int j = 0; j < SB; ++j) {
          v[j] += x;
          vrow[k0 + j * SUB] = v[j];
          c[j] = v[j] + dd[j];
          cand(c[j], di[j]);
        }
        k0 += SB * SUB;
      };
      static_for<0, KB>([&](auto it) {
        // once a batch is not whole k0 stays, so the later ones are not either
        if (k0 + (SB - 1) * SUB < Dm) {
          batch(kept[it.value]);
          nk = it.value + 1;
        }
      });
      kc = k0;
      while (k0 + (SB - 1) * SUB < Dm) {
        float c[SB];
        batch(c);
      }
      for (int k = k0; k < Dm; k += SUB) {
        float v = k == kf ? beg : vrow[k];
        v += x;
        vrow[k] = v;
        const int di = dur_of(k);
        cand(v + drow[di], di);
      }
    }
    float Fv;
    if (VIT) {
      grp_argmax_rt(mx, bd, SUB);
      Fv = mx;
      if (lead) bp[(size_t)t * Lm + l] = (unsigned char)bd;
    } else {
      mx = grp_max_rt(mx, SUB);
      const float ms = mx == NINF ? 0.f : mx;
      float sum = 0.f;
      if (live) {
#pragma unroll
        for (int it = 0; it < KB; ++it)
          if (it < nk) {
#pragma unroll
            for (int j = 0; j < SB; ++j) sum += expf(kept[it][j] - ms);
          }
        int k0 = kc;
        for (; k0 + (SB - 1) * SUB < Dm; k0 += SB * SUB) {
          float c[SB];
#pragma unroll
          for (int j = 0; j < SB; ++j) c[j] = vrow[k0 + j * SUB] + drow[dur_of(k0 + j * SUB)];
#pragma unroll
          for (int j = 0; j < SB; ++j) sum += expf(c[j] - ms);
        }
        for (int k = k0; k < Dm; k += SUB) sum += expf(vrow[k] + drow[dur_of(k)] - ms);
      }
      sum = grp_sum_rt(sum, SUB);
      Fv = mx == NINF ? NINF : ms + logf(sum);
    }
    if (lead) {
      if (tab_out) tab_out[(size_t)t * Lm + l] = Fv;
      if (u == Tb - 1 && p == Lb - 1) fin[0] = Fv;
    }
    kf = kf + 1 == Dm ? 0 : kf + 1;
    // the next step's opening value: the left neighbour's F of this step
    if (WAVE) {
      const float nb = __shfl_up(Fv, SUB);
      beg = (live && p > 0) ? nb : NINF;
    } else {
      float* Fr = Fl + (u & 1) * (Lm + 1);
      if (lead) Fr[p + 1] = Fv;
      lds_barrier();
      beg = live ? Fr[p] : NINF;  // slot 0 stays -inf: nothing opens position 0 after step 0
    }
  };

  for (int u0 = 0; u0 < Tb; u0 += AH)
    static_for<0, AH>([&](auto ph) {
      if (u0 + ph.value < Tb) step(u0 + ph.value, xe[ph.value], xm[ph.value]);
    });

  if (back) return;
  __syncthreads();
  const float best = fin[0];
  const bool feasible = best > NINF;
  if (!VIT) {
    if (tid == 0) {
      a.loglik[b] = feasible ? (float)((double)best + sum_m) : NINF;
      if (a.lls) a.lls[b] = best;
    }
    return;
  }

  // ---- the walk: lane 0 follows the choices back through windows staged in LDS
  int* path = a.path + (size_t)b * T;
  int* durs = a.durs + (size_t)b * Lm;
  if (tid == 0) a.score[b] = feasible ? (float)((double)best + sum_m) : NINF;
  for (int t = (feasible ? Tb : 0) + tid; t < T; t += NT) path[t] = -1;
  for (int i = tid; i < Lm; i += NT) durs[i] = 0;
  if (!feasible) return;
  if (tid == 0) {
    wpos[0] = Tb - 1;
    wpos[1] = Lb - 1;
  }
  global_barrier();  // every lead's choices and the zeroed durations are in memory
  for (;;) {
    __syncthreads();
    int t = wpos[0], q = wpos[1];
    if (q < 0 || t < 0) break;
    const int tlo = t - (kDfWalkRows - 1) > 0 ? t - (kDfWalkRows - 1) : 0;
    const int qlo = q - (kDfWalkCols - 1) > 0 ? q - (kDfWalkCols - 1) : 0;
    const int nr = t - tlo + 1, nc = q - qlo + 1;
    for (int e = tid; e < nr * kDfWalkCols; e += NT) {
      const int r = e / kDfWalkCols, cc = e % kDfWalkCols;
      if (cc < nc) win[e] = bp[(size_t)(tlo + r) * Lm + qlo + cc];
    }
    __syncthreads();
    if (tid == 0) {
      while (q >= qlo && t >= tlo) {
        const int d = (int)win[(t - tlo) * kDfWalkCols + (q - qlo)] + 1;
        const int from = t - d + 1 > 0 ? t - d + 1 : 0;
        durs[q] = d;
        for (int f = from; f <= t; ++f) path[f] = q;
        t -= d;
        --q;
      }
      wpos[0] = t;
      wpos[1] = q;
    }
  }
}

template <bool WAVE>
__global__ void __launch_bounds__(WAVE ? 64 : kDfMaxThreads) durforced_chain_kernel(DfArgs a) {
  extern __shared__ __attribute__((aligned(16))) float df_sm[];
  const int job = a.jobs[blockIdx.y];
  if (job == kJobViterbi)
    df_chain_run<true, WAVE>(a, job, df_sm);
  else
    df_chain_run<false, WAVE>(a, job, df_sm);
}

// ------------------------------------------------------------------ posteriors, counts, gradient
struct DfGradArgs {
  const float* begin;   // (B,T,Lm)
  const float* F;
  const float* Bend;
  const float* Bbeg;
  const float* shift;   // (B,T)
  const float* lls;     // (B)
  const float* lp;      // (B,T,C)
  const int* ids;       // (B,Lm) or NULL
  const int* in_len;
  const int* st_len;
  const float* dur;     // (B,Lm,Dm)
  float* gamma;         // (B,T,Lm): the output, or the workspace's copy for the class sums, or NULL
  float* grad;          // (B,T,C) or NULL
  float* grad_dur;      // (B,Lm,Dm) or NULL
  double* P;            // (B,T,Lm) prefix sums of the finite x, or NULL
  int* Cinf;            // (B,T,Lm) -inf frames so far
  double* part;         // (B,chunks,Dm*Lm) partial sums of the counts kernel
  int B, T, C, Lm, Dm, chunks;
  int gx;               // gamma workgroups per sequence: 64 positions each
  int n_gamma;          // gamma workgroups of the first launch (the rest form prefix sums)
  int n_red;            // count-reducing workgroups of the third launch (the rest sum classes)
  int cx;               // cell blocks per sequence and chunk: 256 cells each
  int tiles;            // class-sum workgroups per sequence
};

// fp64 prefix sums of x = lp - M over the finite frames of every position, and the count of its
// -inf frames: O(a..t,l) = P_t - P_a-1 when the counts agree, else -inf
__device__ void df_prefix_run(const DfGradArgs& a, int b) {
  const int l = threadIdx.x, T = a.T, Lm = a.Lm, C = a.C;
  const int Tb = clamp_int(a.in_len[b], 1, T);
  const int Lb = clamp_int(a.st_len[b], 1, Lm);
  if (l >= Lb) return;
  const int c = a.ids ? a.ids[(size_t)b * Lm + l] : l;
  const bool ok = c >= 0 && c < C;
  const float* lp = a.lp + (size_t)b * T * C + (ok ? c : 0);
  const float* Mb = a.shift + (size_t)b * T;
  double* P = a.P + (size_t)b * T * Lm + l;
  int* Ci = a.Cinf + (size_t)b * T * Lm + l;
  double acc = 0.0;
  int cnt = 0;
#pragma unroll 8
  for (int t = 0; t < Tb; ++t) {
    const float x = ok ? lp[(size_t)t * C] : -INFINITY;
    const float m = Mb[t];
    if (x == -INFINITY)
      ++cnt;
    else
      acc += (double)x - (double)m;
    P[(size_t)t * Lm] = acc;
    Ci[(size_t)t * Lm] = cnt;
  }
}

__global__ void __launch_bounds__(64 * kDfGammaChunks) durforced_gamma_kernel(DfGradArgs a) {
  __shared__ double tot[kDfGammaChunks][64];
  if ((int)blockIdx.x >= a.n_gamma) {
    df_prefix_run(a, (int)blockIdx.x - a.n_gamma);
    return;
  }
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x / a.gx, T = a.T, Lm = a.Lm;
  const float NINF = -INFINITY;
  const int Tb = clamp_int(a.in_len[b], 1, T);
  const int Lb = clamp_int(a.st_len[b], 1, Lm);
  const float llf = a.lls[b];
  const bool feasible = llf > NINF;
  const double ll = feasible ? (double)llf : 0.0;
  const size_t off = (size_t)b * T * Lm;
  const int l = (blockIdx.x % a.gx) * 64 + lane;
  const bool col = l < Lm;            // a column of the output
  const bool live = l < Lb && feasible;
  const int lc = col ? l : Lm - 1;
  const float* bg = a.begin + off + lc;
  const float* bb = a.Bbeg + off + lc;
  const float* fe = a.F + off + lc;
  const float* be = a.Bend + off + lc;
  float* g = a.gamma + off + lc;
  // frames past T_b, and every frame of an unused position or an infeasible pair, are 0
  const int tz = live ? Tb : 0;
  if (col)
    for (int t = tz + w; t < T; t += kDfGammaChunks) g[(size_t)t * Lm] = 0.f;
  const int CH = (Tb + kDfGammaChunks - 1) / kDfGammaChunks;
  const int t0 = w * CH < Tb ? w * CH : Tb, t1 = t0 + CH < Tb ? t0 + CH : Tb;
  // P(a segment of l begins at t) - P(a segment of l ended at t - 1)
  auto delta = [&](int t) -> double {
    const float x0 = bg[(size_t)t * Lm], x1 = bb[(size_t)t * Lm];
    double d = (x0 > NINF && x1 > NINF) ? exp((double)x0 + (double)x1 - ll) : 0.0;
    if (t > 0) {
      const float y0 = fe[(size_t)(t - 1) * Lm], y1 = be[(size_t)(t - 1) * Lm];
      if (y0 > NINF && y1 > NINF) d -= exp((double)y0 + (double)y1 - ll);
    }
    return d;
  };
  double acc = 0.0;
  if (live)
    for (int t = t0; t < t1; ++t) acc += delta(t);
  tot[w][lane] = acc;
  __syncthreads();
  if (!live) return;
  double run = 0.0;
  for (int k = 0; k < w; ++k) run += tot[k][lane];
  for (int t = t0; t < t1; ++t) {
    run += delta(t);
    g[(size_t)t * Lm] = (float)run;
  }
}

// expected number of (l,d) segments: one thread per (l,d) and time chunk, ends t ascending
__global__ void __launch_bounds__(256) durforced_count_kernel(DfGradArgs a) {
  const int T = a.T, Lm = a.Lm, Dm = a.Dm, cells = Lm * Dm;
  const int blk = blockIdx.x;
  const int b = blk / (a.cx * a.chunks), rem = blk % (a.cx * a.chunks);
  const int c = rem / a.cx;
  const int idx = (rem % a.cx) * 256 + threadIdx.x;  // d * Lm + l: a wave reads along l
  if (idx >= cells) return;
  const float NINF = -INFINITY;
  const int l = idx % Lm, d = idx / Lm;  // duration d + 1
  const int Tb = clamp_int(a.in_len[b], 1, T);
  const int Lb = clamp_int(a.st_len[b], 1, Lm);
  const float llf = a.lls[b];
  const float du = a.dur[((size_t)b * Lm + l) * Dm + d];
  const int TC = (Tb + a.chunks - 1) / a.chunks;
  int t0 = c * TC;
  const int t1 = t0 + TC < Tb ? t0 + TC : Tb;
  if (t0 < d) t0 = d;
  double acc = 0.0;
  if (llf > NINF && du > NINF && l < Lb) {
    const size_t off = (size_t)b * T * Lm + l;
    const double base = (double)du - (double)llf;
    for (int t = t0; t < t1; ++t) {
      const int st = t - d;
      const float x0 = a.begin[off + (size_t)st * Lm], x1 = a.Bend[off + (size_t)t * Lm];
      const double pt = a.P[off + (size_t)t * Lm];
      const int ct = a.Cinf[off + (size_t)t * Lm];
      const double pa = st > 0 ? a.P[off + (size_t)(st - 1) * Lm] : 0.0;
      const int ca = st > 0 ? a.Cinf[off + (size_t)(st - 1) * Lm] : 0;
      if (x0 > NINF && x1 > NINF && ct == ca)
        acc += (double)expf((float)((double)x0 + (pt - pa) + (double)x1 + base));
    }
  }
  a.part[((size_t)b * a.chunks + c) * cells + idx] = acc;
}

// the chunk partials in chunk order into grad_dur (B,Lm,Dm); further workgroups: the class sums of
// gamma, d loglik / d log_probs, kDfClassRows frames each
__global__ void __launch_bounds__(256) durforced_reduce_kernel(DfGradArgs a) {
  __shared__ int lab[kDfMaxPos];
  __shared__ short nxt[kDfMaxPos];
  __shared__ unsigned char has_prev[kDfMaxPos];
  const int k = threadIdx.x, Lm = a.Lm, Dm = a.Dm, T = a.T, C = a.C;
  if ((int)blockIdx.x < a.n_red) {
    const int cells = Lm * Dm;
    const int b = blockIdx.x / a.cx;
    const int idx = (blockIdx.x % a.cx) * 256 + k;
    if (idx >= cells) return;
    double acc = 0.0;
    for (int c = 0; c < a.chunks; ++c) acc += a.part[((size_t)b * a.chunks + c) * cells + idx];
    a.grad_dur[(size_t)b * cells + (size_t)(idx % Lm) * Dm + idx / Lm] = (float)acc;
    return;
  }
  const int blk = (int)blockIdx.x - a.n_red;
  const int b = blk / a.tiles;
  const int t0 = (blk % a.tiles) * kDfClassRows;
  const int t1 = t0 + kDfClassRows < T ? t0 + kDfClassRows : T;
  const int lane = k & 63, w = k >> 6;
  const int Tb = clamp_int(a.in_len[b], 1, T);
  const int Lb = clamp_int(a.st_len[b], 1, Lm);
  // this workgroup's frames start as zero: classes that are not in the chain, frames >= T_b, an
  // infeasible pair
  float* g0 = a.grad + ((size_t)b * T + t0) * C;
  for (size_t e = k; e < (size_t)(t1 - t0) * C; e += 256) g0[e] = 0.f;
  const int tend = t1 < Tb ? t1 : Tb;
  if (!(a.lls[b] > -INFINITY) || t0 >= tend) return;
  // group the positions by class: nxt[i] is the next position of the class of position i
  for (int i = k; i < Lb; i += 256) {
    lab[i] = a.ids ? a.ids[(size_t)b * Lm + i] : i;
    has_prev[i] = 0;
  }
  __syncthreads();
  for (int i = k; i < Lb; i += 256) {
    const int v = lab[i];
    int j = i + 1;
    while (j < Lb && lab[j] != v) ++j;
    nxt[i] = (short)(j < Lb ? j : -1);
  }
  __syncthreads();
  for (int i = k; i < Lb; i += 256)
    if (nxt[i] >= 0) has_prev[nxt[i]] = 1;
  global_barrier();  // the zeros are in memory before any sum is stored over them
  for (int t = t0 + w; t < tend; t += 4) {
    const float* gm = a.gamma + ((size_t)b * T + t) * Lm;
    float* gr = a.grad + ((size_t)b * T + t) * C;
    for (int i = lane; i < Lb; i += 64) {
      if (has_prev[i]) continue;
      const int c = lab[i];
      if (c < 0 || c >= C) continue;
      float sum = 0.f;
      for (int j = i; j >= 0; j = nxt[j]) sum += gm[j];
      gr[c] = sum;
    }
  }
}

// ------------------------------------------------------------------ host side
int df_chunks(int cells, int T) {
  int c = (kDfPartCells + cells - 1) / cells;
  c = c < kDfMaxChunks ? c : kDfMaxChunks;
  const int by_t = (T + 15) / 16;  // at least 16 frames a chunk
  c = c < by_t ? c : by_t;
  return c < 1 ? 1 : c;
}

int df_shape_check(int B, int T, int C, int Lm, int Dm) {
  if (T < 1 || B < 1 || C < 1) return HMM355_E_ARG;
  if (Lm < 1 || Lm > kDfMaxPos || Dm < 1 || Dm > kDfMaxDur || Lm * Dm > kDfMaxCells) return HMM355_E_STATES;
  const size_t lim = (size_t)1 << 46;
  size_t n, m;
  if (__builtin_mul_overflow((size_t)T, (size_t)B, &n) || n > ((size_t)1 << 31)) return HMM355_E_SHAPE;
  if (__builtin_mul_overflow(n, (size_t)Lm, &m) || m > lim) return HMM355_E_SHAPE;
  if (__builtin_mul_overflow(n, (size_t)C, &m) || m > lim) return HMM355_E_SHAPE;
  // workgroups are counted in an int: B times the tiles of a sequence
  if ((size_t)B * ((size_t)Lm * Dm / 256 + 1) * kDfMaxChunks > ((size_t)1 << 31)) return HMM355_E_SHAPE;
  return HMM355_OK;
}

// (each layout ends with 256 bytes of slack)
struct DfLayout {
  float* M;
  unsigned char* bp;
  size_t total;
};
DfLayout df_layout(int B, int T, int Lm, unsigned flags, char* base) {
  DfLayout L{};
  Carver c{base};
  L.M = c.take<float>((size_t)3 * B * T);
  L.bp = c.take<unsigned char>((flags & HMM355_DURFORCED_VITERBI) ? (size_t)B * T * Lm : 0);
  L.total = c.bytes() + 256;
  return L;
}

struct DfGradLayout {
  float* gamma;
  double* P;
  int* Cinf;
  double* part;
  size_t total;
  int chunks;
};
DfGradLayout df_grad_layout(int B, int T, int Lm, int Dm, char* base) {
  DfGradLayout L{};
  Carver c{base};
  const size_t n = (size_t)B * T * Lm;
  L.chunks = df_chunks(Lm * Dm, T);
  L.gamma = c.take<float>(n);
  L.P = c.take<double>(n);
  L.Cinf = c.take<int>(n);
  L.part = c.take<double>((size_t)B * L.chunks * Lm * Dm);
  L.total = c.bytes() + 256;
  return L;
}

}  // namespace
}  // namespace hmm355

using namespace hmm355;

HMM355_API size_t hmm355_durforced_workspace_bytes(int B, int T, int Lmax, int Dmax, unsigned flags) {
  if (df_shape_check(B, T, 1, Lmax, Dmax) != HMM355_OK) return 0;
  if (flags & ~(kDfFlags | HMM355_DURFORCED_GRAD)) return 0;
  const size_t run = df_layout(B, T, Lmax, flags, nullptr).total;
  const size_t grad = (flags & HMM355_DURFORCED_GRAD) ? df_grad_layout(B, T, Lmax, Dmax, nullptr).total : 0;
  return run > grad ? run : grad;
}

HMM355_API int hmm355_durforced_f32(const float* log_probs, const int* state_ids, const int* input_lengths,
                                    const int* state_lengths, const float* dur_lp, int B, int T, int C, int Lmax,
                                    int Dmax, unsigned flags, float* begin, float* F, float* Bend, float* Bbeg,
                                    float* frame_shift, float* loglik_shifted, float* loglik, int* path, float* score,
                                    int* durations, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = df_shape_check(B, T, C, Lmax, Dmax);
  if (rc != HMM355_OK) return rc;
  if (!state_ids && C < Lmax) return HMM355_E_ARG;
  if (flags & ~kDfFlags) return HMM355_E_ARG;
  if (!log_probs || !input_lengths || !state_lengths || !dur_lp || !loglik || !workspace) return HMM355_E_ARG;
  const bool tables = flags & HMM355_DURFORCED_TABLES;
  if (tables && (!begin || !F || !Bend || !Bbeg || !frame_shift || !loglik_shifted)) return HMM355_E_ARG;
  if ((flags & HMM355_DURFORCED_VITERBI) && (!path || !score || !durations)) return HMM355_E_ARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return HMM355_E_ARG;
  const DfLayout L = df_layout(B, T, Lmax, flags, static_cast<char*>(workspace));
  if (workspace_bytes < L.total) return HMM355_E_WORKSPACE;
  DfArgs a{};
  a.lp = log_probs;
  a.ids = state_ids;
  a.in_len = input_lengths;
  a.st_len = state_lengths;
  a.dur = dur_lp;
  if (tables) {
    a.begin = begin;
    a.F = F;
    a.Bend = Bend;
    a.Bbeg = Bbeg;
    a.shift = frame_shift;
    a.lls = loglik_shifted;
  }
  a.loglik = loglik;
  a.path = path;
  a.score = score;
  a.durs = durations;
  a.M = L.M;
  a.bp = L.bp;
  a.B = B;
  a.T = T;
  a.C = C;
  a.Lm = Lmax;
  a.Dm = Dmax;
  // lanes per position: a power of two inside one wave, as many as 1024 threads hold and the
  // position's Dmax slots have work for
  int sub = 64;
  while (sub > 1 && Lmax * sub > kDfMaxThreads) sub >>= 1;
  while (sub > 1 && (sub >> 1) >= Dmax) sub >>= 1;
  a.SUB = sub;
  a.NT = (Lmax * sub + 63) / 64 * 64;
  a.DS = df_row_stride(Dmax, sub);
  int nj = 0;
  a.jobs[nj++] = kJobForward;
  if (tables) a.jobs[nj++] = kJobBackward;
  if (flags & HMM355_DURFORCED_VITERBI) a.jobs[nj++] = kJobViterbi;
  const size_t lds = (size_t)df_carve(Lmax, a.DS).total * 4;
  // the padding is less than 2 * sub floats a row and Lmax * sub <= 1024: the largest carve is
  // that of the most positions
  static_assert((size_t)df_carve(kDfMaxPos, df_row_stride(kDfMaxCells / kDfMaxPos, 1)).total * 4 <= kDfLdsBudget &&
                    (size_t)df_carve(kDfMaxCells / kDfMaxDur, df_row_stride(kDfMaxDur, 8)).total * 4 <= kDfLdsBudget,
                "the padded ring and dur_lp fit");
  if (lds > kDfLdsBudget) return HMM355_E_STATES;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return with_flag(a.NT == 64, [&](auto one_wave) {
    return launch(durforced_chain_kernel<one_wave()>, dim3(B, nj), dim3(a.NT), lds, st, a);
  });
}

HMM355_API int hmm355_durforced_grad_f32(const float* begin, const float* F, const float* Bend, const float* Bbeg,
                                         const float* frame_shift, const float* loglik_shifted,
                                         const float* log_probs, const int* state_ids, const int* input_lengths,
                                         const int* state_lengths, const float* dur_lp, int B, int T, int C, int Lmax,
                                         int Dmax, float* gamma, float* grad_log_probs, float* grad_dur_lp,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = df_shape_check(B, T, C, Lmax, Dmax);
  if (rc != HMM355_OK) return rc;
  if (!state_ids && C < Lmax) return HMM355_E_ARG;
  if (!begin || !F || !Bend || !Bbeg || !frame_shift || !loglik_shifted) return HMM355_E_ARG;
  if (!log_probs || !input_lengths || !state_lengths || !dur_lp) return HMM355_E_ARG;
  if (!gamma && !grad_log_probs && !grad_dur_lp) return HMM355_E_ARG;
  // the workspace holds gamma for the class sums when it is no output, and the counts' sums
  const bool need_ws = grad_dur_lp || (grad_log_probs && !gamma);
  const DfGradLayout L = df_grad_layout(B, T, Lmax, Dmax, static_cast<char*>(workspace));
  if (need_ws) {
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return HMM355_E_ARG;
    if (workspace_bytes < L.total) return HMM355_E_WORKSPACE;
  }
  DfGradArgs a{};
  a.begin = begin;
  a.F = F;
  a.Bend = Bend;
  a.Bbeg = Bbeg;
  a.shift = frame_shift;
  a.lls = loglik_shifted;
  a.lp = log_probs;
  a.ids = state_ids;
  a.in_len = input_lengths;
  a.st_len = state_lengths;
  a.dur = dur_lp;
  a.gamma = gamma ? gamma : (grad_log_probs ? L.gamma : nullptr);
  a.grad = grad_log_probs;
  a.grad_dur = grad_dur_lp;
  if (grad_dur_lp) {
    a.P = L.P;
    a.Cinf = L.Cinf;
    a.part = L.part;
  }
  a.B = B;
  a.T = T;
  a.C = C;
  a.Lm = Lmax;
  a.Dm = Dmax;
  a.chunks = L.chunks;
  a.gx = (Lmax + 63) / 64;
  a.n_gamma = a.gamma ? B * a.gx : 0;
  a.cx = (Lmax * Dmax + 255) / 256;
  a.n_red = grad_dur_lp ? B * a.cx : 0;
  a.tiles = (T + kDfClassRows - 1) / kDfClassRows;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // gamma workgroups, then one prefix-sum workgroup per sequence (a thread per position)
  static_assert(kDfMaxPos <= 64 * kDfGammaChunks, "the prefix sums of a sequence fit one workgroup");
  HMM355_TRY(launch(durforced_gamma_kernel, dim3(a.n_gamma + (grad_dur_lp ? B : 0)), dim3(64 * kDfGammaChunks), 0, st,
                    a));
  if (grad_dur_lp) HMM355_TRY(launch(durforced_count_kernel, dim3(B * a.chunks * a.cx), dim3(256), 0, st, a));
  const int n_cls = grad_log_probs ? B * a.tiles : 0;
  if (a.n_red + n_cls == 0) return HMM355_OK;
  return launch(durforced_reduce_kernel, dim3(a.n_red + n_cls), dim3(256), 0, st, a);
}
