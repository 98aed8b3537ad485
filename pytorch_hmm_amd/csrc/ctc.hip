// hmm355 — CTC lattice: forward (alpha, log-likelihood), backward (beta), Viterbi forced alignment
// and the occupancy / class gradient.
//
// Replaces the per-cell Python loops of pytorch_hmm.alignment.ctc (ctc_forward_algorithm,
// ctc.py:32-121; ctc_backward_algorithm, :124-199) and gives ctc_alignment_path (:202-256) the
// alpha it never fills.  The lattice of sequence b has S'_b = 2 L_b + 1 positions, ext[s] = blank
// for even s and targets[b, s / 2] for odd s; a cell takes from s, s - 1 and, where
// ext[s] != ext[s - 2], from s - 2.
//
// One launch per call, the whole batch in it: one workgroup per (sequence, job), the jobs being
// the forward sum (always: it gives loglik), the backward sum (HMM355_CTC_BETA) and the max-plus
// forward with its walk (HMM355_CTC_VITERBI).  No workgroup waits on another; no flags, no atomics.
//
// How lanes own positions.  A thread owns P consecutive positions u = k P .. k P + P - 1 and keeps
// their values in registers for the whole sequence.  The backward job runs the same recursion on
// the mirrored lattice (u = S'_b - 1 - s, time T_b - 1 - i), so one body serves both.  Per step a
// thread needs two values it does not own, those of u0 - 1 and u0 - 2: the last two of the thread
// to its left.  They travel as one float2 through LDS, double-buffered by step parity, so a step
// costs one barrier.  P is chosen per call from S' = 2 Lmax + 1, the smallest that covers it, so
// that a short lattice still spreads over the workgroup's four waves (a step's time is the P
// dependent log-sum-exps of a thread): 1 in one wave (S' <= 64: the two values come by lane
// shuffles, no LDS and no barrier), 1 (<= 256: the two values are those of threads k - 1 and
// k - 2), kCtcPosLow (<= 512), kCtcPos (<= 1024), kCtcPosMid (<= 2048), kCtcPosWide (<= 4352;
// the ABI stops at Lmax = 2048, S' = 4097).
// Emissions lp[t, b, ext[s]] are a gather; a thread issues the loads of step i + kCtcAhead while it
// computes step i, into a register ring (as dtw.hip and adjoint.hip do), so their latency is not
// on the dependent chain.  The class of every owned position, whether it is inside the lattice
// and whether it may take from u - 2 are worked out once per sequence (bit masks in registers).
// A class outside [0, C) is never read: its emission is -inf.
//
// The sum jobs carry c[u] = the value including the step's emission: r = LSE of the candidates
// (or the start value 0 at u = 0, 1 on the first step), c = r + e.  The forward job stores c
// (alpha); the backward job stores r: the reference's beta excludes the emission of its own
// frame (ctc.py:164-197).  -inf candidates drop out of the LSE, and a cell without a finite
// candidate stays -inf whatever its emission.  Without HMM355_CTC_ALPHA the forward job stores
// no table at all.
// Viterbi: the same lattice with max in place of LSE; candidates in the order stay, u - 1, u - 2
// with strict >, so the first wins a tie; the end is S' - 1 unless S' - 2 is strictly greater.
// Each step is an exact max and one fp32 add.  The choice is kept as 2 bits per cell (one byte
// per four positions of a thread; a byte per lane in the single-wave form) in the workspace, and
// lane 0 walks it afterwards through windows of the table staged in LDS, as dtw.hip does.
//
// Gradient (ctc_grad_kernel): gamma[b,t,s] = exp(alpha + beta - loglik) and
// d loglik / d lp[t,b,c] = sum over {s: ext[s] = c} of gamma.  No floating-point atomics: the
// positions of a class are grouped once per workgroup (the labels' "next label of the same value"
// links, formed in LDS); one lane sums a class's chain in position order and the blank's even
// positions are summed by a fixed shuffle tree, so two runs give the same bits.
#include "launch.h"

namespace hmm355 {
namespace {

constexpr int kCtcThreads = 256;   // threads per workgroup of the LDS forms
constexpr int kCtcPosLow = 2;      // positions per thread: S' <= 512 (1 up to S' = 256)
constexpr int kCtcPos = 4;         // S' <= 1024
constexpr int kCtcPosMid = 8;      // S' <= 2048
constexpr int kCtcPosWide = 17;    // S' <= 4352
constexpr int kCtcAhead = 4;       // steps between an emission gather and its use
constexpr int kCtcWalkRows = 64;   // backtrace window: frames
constexpr int kCtcWalkBytes = 136; // ... and bytes of a frame's choices (2 * 63 + 1 positions)
constexpr int kCtcGradRows = 32;   // frames per workgroup of the gradient kernel
constexpr int kCtcMaxTarget = HMM355_CTC_MAX_TARGET;

constexpr int kJobForward = 0, kJobBackward = 1, kJobViterbi = 2;

struct CtcArgs {
  const float* lp;        // (T,B,C)
  const int* targets;     // (B,Lmax)
  const int* in_len;      // (B)
  const int* tg_len;      // (B)
  float* alpha;           // (B,T,S') or NULL
  float* beta;            // (B,T,S') or NULL
  float* loglik;          // (B)
  int* path;              // (B,T)
  float* score;           // (B)
  unsigned char* bp;      // (B,T,row_bytes) the Viterbi choices
  int T, B, C, Lmax, blank;
  int jobs[3];
};

struct CtcShared {
  float2 xch[2][kCtcThreads + 2];  // slot k + 2: thread k's last two values
  unsigned char win[kCtcWalkRows][kCtcWalkBytes];
  float fin[2];
  int wpos[2];
};

template <int P, int NT, bool VIT>
__device__ __forceinline__ void ctc_run(const CtcArgs& a, const int job, CtcShared& sh) {
  constexpr int AH = kCtcAhead;
  constexpr int PB = (P + 3) / 4;  // bytes of choices per thread and step
  constexpr int RB = NT * PB;      // ... per frame
  const float NINF = -INFINITY;
  const int k = threadIdx.x;
  const int b = blockIdx.x;
  const int T = a.T, B = a.B, C = a.C;
  const int Tb = clamp_int(a.in_len[b], 1, T);
  const int Lb = clamp_int(a.tg_len[b], 0, a.Lmax);
  const int Sb = 2 * Lb + 1, Sm = 2 * a.Lmax + 1;
  const bool back = job == kJobBackward;
  const int* tg = a.targets + (size_t)b * a.Lmax;
  float* tab = VIT ? nullptr : (back ? a.beta : a.alpha);
  if (tab) tab += (size_t)b * T * Sm;
  unsigned char* bp = VIT ? a.bp + (size_t)b * T * RB : nullptr;

  // cells no step writes: frames >= T_b and positions >= S'_b
  if (tab) {
    const size_t lo = (size_t)Tb * Sm, hi = (size_t)T * Sm;
    for (size_t e = lo + k; e < hi; e += NT) tab[e] = NINF;
    if (Sb < Sm) {
      const int w = Sm - Sb;
      for (size_t e = k; e < (size_t)Tb * w; e += NT) tab[(e / w) * Sm + Sb + (e % w)] = NINF;
    }
  }

  // once per sequence: the class of each owned position, which of them exist, which may skip
  int cls[P], pos[P];
  unsigned valid = 0, skip = 0;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int u = k * P + j;
    const int s = back ? Sb - 1 - u : u;
    cls[j] = -1;
    pos[j] = s;
    if (u < Sb) {
      valid |= 1u << j;
      const int c = (s & 1) ? tg[s >> 1] : a.blank;
      if (c >= 0 && c < C) cls[j] = c;
      if (u >= 2) {
        const int s2 = back ? s + 2 : s - 2;
        const int c2 = (s2 & 1) ? tg[s2 >> 1] : a.blank;
        if (c2 != c) skip |= 1u << j;
      }
    }
  }

  auto gather = [&](int i, float (&e)[P]) __attribute__((always_inline)) {
    const int t = back ? Tb - 1 - i : i;
    const float* row = a.lp + ((size_t)t * B + b) * C;
#pragma unroll
    for (int j = 0; j < P; ++j) e[j] = cls[j] >= 0 ? row[cls[j]] : (((valid >> j) & 1u) ? NINF : 0.f);
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
    float in1, in2;  // the values of u0 - 1 and u0 - 2
    if (!LDS) {
      in1 = __shfl_up(c[0], 1);
      in2 = __shfl_up(c[0], 2);
      if (k < 1) in1 = NINF;
      if (k < 2) in2 = NINF;
    } else if (P == 1) {
      in1 = sh.xch[i & 1][k + 1].y;
      in2 = sh.xch[i & 1][k].y;
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
      const float stay = c[j];
      const float p1 = j >= 1 ? c[j >= 1 ? j - 1 : 0] : in1;
      float p2 = j >= 2 ? c[j >= 2 ? j - 2 : 0] : (j == 1 ? in1 : in2);
      if (!((skip >> j) & 1u)) p2 = NINF;
      float r;
      if (VIT) {
        unsigned d = 0;
        r = stay;
        if (p1 > r) {
          r = p1;
          d = 1;
        }
        if (p2 > r) {
          r = p2;
          d = 2;
        }
        bits[j >> 2] |= d << (2 * (j & 3));
      } else {
        r = lse3(stay, p1, p2);
      }
      if (i == 0) r = (u == 0 || (u == 1 && Sb >= 2)) ? 0.f : NINF;
      const bool ok = (valid >> j) & 1u;
      if (!ok) r = NINF;
      const float val = r + e[j];
      if (tab && ok) tab[(size_t)t * Sm + pos[j]] = back ? r : val;
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

  // the last frame's two end positions
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int u = k * P + j;
    if (u == Sb - 1) sh.fin[0] = c[j];
    if (u == Sb - 2) sh.fin[1] = c[j];
  }
  __syncthreads();
  const float a1 = sh.fin[0];
  const float a2 = Sb >= 2 ? sh.fin[1] : NINF;
  if (!VIT) {
    if (k == 0) a.loglik[b] = lse3(a1, a2, NINF);
    return;
  }

  // ---- the walk: lane 0 follows the choices back through windows staged in LDS
  const float best = a2 > a1 ? a2 : a1;
  int* path = a.path + (size_t)b * T;
  if (k == 0) a.score[b] = best;
  const bool feasible = best > NINF;
  for (int t = (feasible ? Tb : 0) + k; t < T; t += NT) path[t] = -1;
  if (!feasible) return;
  auto byte_of = [&](int u) { return (u / P) * PB + ((u % P) >> 2); };
  if (k == 0) {
    sh.wpos[0] = Tb - 1;
    sh.wpos[1] = a2 > a1 ? Sb - 2 : Sb - 1;
  }
  global_barrier();  // every thread's choices are in memory
  for (;;) {
    __syncthreads();
    int t = sh.wpos[0], s = sh.wpos[1];
    if (t <= 0) break;
    const int tlo = t - (kCtcWalkRows - 1) > 1 ? t - (kCtcWalkRows - 1) : 1;
    const int slo = s - 2 * (t - tlo) > 0 ? s - 2 * (t - tlo) : 0;
    const int blo = byte_of(slo);
    const int nb = byte_of(s) - blo + 1, nr = t - tlo + 1;
    for (int e = k; e < nr * kCtcWalkBytes; e += NT) {
      const int r = e / kCtcWalkBytes, cc = e % kCtcWalkBytes;
      if (cc < nb) sh.win[r][cc] = bp[(size_t)(tlo + r) * RB + blo + cc];
    }
    __syncthreads();
    if (k == 0) {
      while (t >= tlo) {
        path[t] = s;
        const unsigned d = (sh.win[t - tlo][byte_of(s) - blo] >> (2 * ((s % P) & 3))) & 3u;
        s -= (int)d;
        --t;
      }
      sh.wpos[0] = t;
      sh.wpos[1] = s;
    }
  }
  if (k == 0) path[0] = sh.wpos[1];
}

template <int P, int NT>
__global__ void __launch_bounds__(NT) ctc_kernel(CtcArgs a) {
  __shared__ CtcShared sh;
  const int job = a.jobs[blockIdx.y];
  if (job == kJobViterbi)
    ctc_run<P, NT, true>(a, job, sh);
  else
    ctc_run<P, NT, false>(a, job, sh);
}

// ------------------------------------------------------------------ occupancy and class gradient
struct CtcGradArgs {
  const float* alpha;   // (B,T,S')
  const float* beta;    // (B,T,S')
  const float* loglik;  // (B)
  const int* targets;
  const int* in_len;
  const int* tg_len;
  float* gamma;         // (B,T,S') or NULL
  float* grad;          // (T,B,C)
  int T, B, C, Lmax, blank;
};

__global__ void __launch_bounds__(kCtcThreads) ctc_grad_kernel(CtcGradArgs a) {
  constexpr int NT = kCtcThreads;
  __shared__ int lab[kCtcMaxTarget];
  __shared__ short nxt[kCtcMaxTarget];
  __shared__ unsigned char has_prev[kCtcMaxTarget];
  const int k = threadIdx.x;
  const int b = blockIdx.x;
  const int T = a.T, B = a.B, C = a.C;
  const int t0 = blockIdx.y * kCtcGradRows;
  const int t1 = t0 + kCtcGradRows < T ? t0 + kCtcGradRows : T;
  const int Tb = clamp_int(a.in_len[b], 1, T);
  const int Lb = clamp_int(a.tg_len[b], 0, a.Lmax);
  const int Sm = 2 * a.Lmax + 1;
  const float ll = a.loglik[b];
  const float NINF = -INFINITY;

  // this workgroup's frames start as zero: classes that are not in the target, frames >= T_b,
  // an infeasible pair
  for (int e = k; e < (t1 - t0) * C; e += NT) a.grad[((size_t)(t0 + e / C) * B + b) * C + e % C] = 0.f;
  if (a.gamma) {
    float* g = a.gamma + ((size_t)b * T + t0) * Sm;
    for (int e = k; e < (t1 - t0) * Sm; e += NT) g[e] = 0.f;
  }
  const int tend = t1 < Tb ? t1 : Tb;
  if (!(ll > NINF) || t0 >= tend) return;

  // group the label positions by class: nxt[i] is the next label equal to label i
  const int* tg = a.targets + (size_t)b * a.Lmax;
  for (int i = k; i < Lb; i += NT) {
    lab[i] = tg[i];
    has_prev[i] = 0;
  }
  __syncthreads();
  for (int i = k; i < Lb; i += NT) {
    const int v = lab[i];
    int j = i + 1;
    while (j < Lb && lab[j] != v) ++j;
    nxt[i] = (short)(j < Lb ? j : -1);
  }
  __syncthreads();
  for (int i = k; i < Lb; i += NT)
    if (nxt[i] >= 0) has_prev[nxt[i]] = 1;
  global_barrier();  // the zeros are in memory before any sum is stored over them

  const int lane = k & 63, w = k >> 6;
  for (int t = t0 + w; t < tend; t += NT / 64) {
    const float* ar = a.alpha + ((size_t)b * T + t) * Sm;
    const float* br = a.beta + ((size_t)b * T + t) * Sm;
    float* gr = a.grad + ((size_t)t * B + b) * C;
    float* gm = a.gamma ? a.gamma + ((size_t)b * T + t) * Sm : nullptr;
    auto occ = [&](int s) {
      const float al = ar[s], be = br[s];
      const float d = (float)((double)al + (double)be - (double)ll);
      const float g = (al > NINF && be > NINF) ? expf(d) : 0.f;
      if (gm) gm[s] = g;
      return g;
    };
    float acc = 0.f;  // the blank: even positions
    for (int i = lane; i <= Lb; i += 64) acc += occ(2 * i);
    float extra = 0.f;  // ... and the labels that equal it
    for (int i = lane; i < Lb; i += 64) {
      if (has_prev[i]) continue;
      float sum = 0.f;
      for (int j = i; j >= 0; j = nxt[j]) sum += occ(2 * j + 1);
      const int c = lab[i];
      if (c == a.blank)
        extra = sum;
      else if (c >= 0 && c < C)
        gr[c] = sum;
    }
    acc = wave_sum(acc);
    extra = wave_sum(extra);
    if (lane == 0) gr[a.blank] = acc + extra;
  }
}

// the 2-bit choices of the Viterbi job, (B,T,row_bytes); 256 bytes otherwise, so that 0 always
// means a rejected shape
int ctc_row_bytes(int Sm) {
  if (Sm <= 64) return 64;
  if (Sm <= kCtcThreads * kCtcPosLow) return kCtcThreads;
  if (Sm <= kCtcThreads * kCtcPos) return kCtcThreads * ((kCtcPos + 3) / 4);
  if (Sm <= kCtcThreads * kCtcPosMid) return kCtcThreads * ((kCtcPosMid + 3) / 4);
  return kCtcThreads * ((kCtcPosWide + 3) / 4);
}

int ctc_shape_check(int T, int B, int C, int Lmax) {
  if (T < 1 || B < 1 || C < 1) return HMM355_E_ARG;
  if (Lmax < 1 || Lmax > kCtcMaxTarget) return HMM355_E_STATES;
  const size_t Sm = 2 * (size_t)Lmax + 1, lim = (size_t)1 << 46;
  size_t n;
  if (__builtin_mul_overflow((size_t)T, (size_t)B, &n) || n > lim) return HMM355_E_SHAPE;
  size_t m;
  if (__builtin_mul_overflow(n, Sm, &m) || m > lim) return HMM355_E_SHAPE;
  if (__builtin_mul_overflow(n, (size_t)C, &m) || m > lim) return HMM355_E_SHAPE;
  return HMM355_OK;
}

constexpr unsigned kCtcFlags = HMM355_CTC_ALPHA | HMM355_CTC_BETA | HMM355_CTC_VITERBI;

size_t ctc_ws_bytes(int B, int T, int Lmax, unsigned flags) {
  if (!(flags & HMM355_CTC_VITERBI)) return 256;
  return align_up((size_t)B * T * ctc_row_bytes(2 * Lmax + 1), 256) + 256;
}

}  // namespace
}  // namespace hmm355

using namespace hmm355;

HMM355_API size_t hmm355_ctc_workspace_bytes(int B, int T, int Lmax, unsigned flags) {
  if (ctc_shape_check(T, B, 1, Lmax) != HMM355_OK) return 0;
  if (flags & ~kCtcFlags) return 0;
  return ctc_ws_bytes(B, T, Lmax, flags);
}

HMM355_API int hmm355_ctc_f32(const float* log_probs, const int* targets, const int* input_lengths,
                              const int* target_lengths, int T, int B, int C, int Lmax, int blank, unsigned flags,
                              float* alpha, float* beta, float* loglik, int* path, float* score, void* workspace,
                              size_t workspace_bytes, void* stream) {
  const int rc = ctc_shape_check(T, B, C, Lmax);
  if (rc != HMM355_OK) return rc;
  if (flags & ~kCtcFlags) return HMM355_E_ARG;
  if (blank < 0 || blank >= C) return HMM355_E_ARG;
  if (!log_probs || !targets || !input_lengths || !target_lengths || !loglik || !workspace) return HMM355_E_ARG;
  if ((flags & HMM355_CTC_ALPHA) && !alpha) return HMM355_E_ARG;
  if ((flags & HMM355_CTC_BETA) && !beta) return HMM355_E_ARG;
  if ((flags & HMM355_CTC_VITERBI) && (!path || !score)) return HMM355_E_ARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return HMM355_E_ARG;
  if (workspace_bytes < ctc_ws_bytes(B, T, Lmax, flags)) return HMM355_E_WORKSPACE;
  CtcArgs a{};
  a.lp = log_probs;
  a.targets = targets;
  a.in_len = input_lengths;
  a.tg_len = target_lengths;
  a.alpha = (flags & HMM355_CTC_ALPHA) ? alpha : nullptr;
  a.beta = (flags & HMM355_CTC_BETA) ? beta : nullptr;
  a.loglik = loglik;
  a.path = path;
  a.score = score;
  a.bp = static_cast<unsigned char*>(workspace);
  a.T = T;
  a.B = B;
  a.C = C;
  a.Lmax = Lmax;
  a.blank = blank;
  int nj = 0;
  a.jobs[nj++] = kJobForward;
  if (flags & HMM355_CTC_BETA) a.jobs[nj++] = kJobBackward;
  if (flags & HMM355_CTC_VITERBI) a.jobs[nj++] = kJobViterbi;
  const int Sm = 2 * Lmax + 1;
  hipStream_t sm = static_cast<hipStream_t>(stream);
  const dim3 grid(B, nj), block(kCtcThreads);
  if (Sm <= 64) return launch(ctc_kernel<1, 64>, grid, dim3(64), 0, sm, a);
  if (Sm <= kCtcThreads) return launch(ctc_kernel<1, kCtcThreads>, grid, block, 0, sm, a);
  if (Sm <= kCtcThreads * kCtcPosLow) return launch(ctc_kernel<kCtcPosLow, kCtcThreads>, grid, block, 0, sm, a);
  if (Sm <= kCtcThreads * kCtcPos) return launch(ctc_kernel<kCtcPos, kCtcThreads>, grid, block, 0, sm, a);
  if (Sm <= kCtcThreads * kCtcPosMid) return launch(ctc_kernel<kCtcPosMid, kCtcThreads>, grid, block, 0, sm, a);
  return launch(ctc_kernel<kCtcPosWide, kCtcThreads>, grid, block, 0, sm, a);
}

HMM355_API int hmm355_ctc_grad_f32(const float* alpha, const float* beta, const float* loglik, const int* targets,
                                   const int* input_lengths, const int* target_lengths, int T, int B, int C, int Lmax,
                                   int blank, float* gamma, float* grad, void* stream) {
  const int rc = ctc_shape_check(T, B, C, Lmax);
  if (rc != HMM355_OK) return rc;
  if (blank < 0 || blank >= C) return HMM355_E_ARG;
  if (!alpha || !beta || !loglik || !targets || !input_lengths || !target_lengths || !grad) return HMM355_E_ARG;
  CtcGradArgs a{alpha, beta, loglik, targets, input_lengths, target_lengths, gamma, grad, T, B, C, Lmax, blank};
  const dim3 grid(B, (T + kCtcGradRows - 1) / kCtcGradRows);
  return launch(ctc_grad_kernel, grid, dim3(kCtcThreads), 0, static_cast<hipStream_t>(stream), a);
}
