// hmm355 — occupancy-weighted sufficient statistics of diagonal Gaussian (mixture) emissions on
// gfx950: the emission half of the Baum-Welch E-step (pytorch_hmm_amd/em.py).
//
// For a signed frame weight weight[b,t,s] (EM passes the state posteriors) and the component
// responsibilities r[b,t,s,c] (softmax over c of the scorer's comp, csrc/gmm.hip):
//     w   = weight * r
//     occ[s,c]   = sum_{b, t < len_b} w
//     sx [s,c,d] = sum w (x_d - mu_scd)
//     sxx[s,c,d] = sum w (x_d - mu_scd)^2
// centred on the current means: the M-step's mu' = mu + sx/occ and var' = sxx/occ - (sx/occ)^2
// have none of the cancellation of raw second moments.
//
// Layout.  A workgroup (256 threads) owns NC = 64 / 128 / 256 component lanes (the smallest that
// holds one state's C components: spb = NC / C whole states) and a contiguous span of 32-frame
// tiles; its NG = 256 / NC lane groups split the feature dims in 8-dim chunks, so a lane owns one
// component and every NG-th chunk.  Per tile:
//   phase A  each lane group accumulates the scorer's fp64 quadratic form of its chunks (frames
//            staged fp32 -> fp64 in an LDS double buffer, read as broadcasts; 2 v_fma_f64 per
//            (frame, component, dim)); the groups' partial forms are summed through LDS, a thread
//            per (frame, state) takes the maximum and 1 / sum exp over c, and every lane forms w
//            for its component and the tile's 32 frames in registers.  Skipped when C == 1 (r = 1).
//   phase B  walks the lane's own chunks again: diff = x - mu, sx += w diff, sxx += (w diff) diff in
//            fp64 registers that persist across the span's tiles (kEsKC chunks = 48 accumulators).
// One wave per SIMD (256 VGPRs + 232 AGPRs, no scratch): nothing hides a latency, so the frame
// weights, the frames and the lane's parameters are requested ahead of their use and the inner
// loops are ordered so that no fp64 operation waits on the one just issued.
// D above NG * kEsKC * 8 dims splits over blockIdx.z; every split repeats phase A (all dims) and
// keeps its own dims in phase B.  The span's sums go to a slab [span][2D + 1][PP] (fp32) and
// es_reduce_kernel adds the spans in index order in fp64: no atomics, the same bits on every call.
// Frames at t >= lengths[b] are selected out (x staged as 0, weight 0) and never read.
#include "launch.h"

namespace hmm355 {

constexpr int kEsThreads = 256;
constexpr int kEsFrames = 32;     // frames per tile (fp64 accumulators of phase A per lane)
constexpr int kEsDc = 8;          // dims per chunk
constexpr int kEsKC = 3;          // chunks a lane accumulates in phase B (2 * 8 * kEsKC fp64 registers)
constexpr int kEsSub = 8;         // frames per LDS round of the responsibilities
constexpr int kEsMinTiles = 4;    // tiles per span at least (the flush is 2 * 8 * kEsKC stores per lane)
constexpr int kEsWorkgroups = 512;  // spans are sized so that about this many workgroups run
constexpr int kEsDMax = HMM355_GMM_STATS_MAX_DIM;

struct EsGeo {
  int NC, NG, spb, ngroups, NDC, DP, nz, PP, K;
  size_t ntiles, tps, nspans;
};

static EsGeo es_geo(int B, int T, int D, int S, int C) {
  EsGeo g;
  g.NC = C <= 64 ? 64 : (C <= 128 ? 128 : 256);
  g.NG = kEsThreads / g.NC;
  g.spb = g.NC / C;
  g.ngroups = (S + g.spb - 1) / g.spb;
  g.NDC = (D + kEsDc - 1) / kEsDc;
  g.DP = g.NDC * kEsDc;
  g.nz = (g.NDC + kEsKC * g.NG - 1) / (kEsKC * g.NG);
  g.PP = (S * C + 63) / 64 * 64;
  g.K = 2 * D + 1;
  const size_t nframes = (size_t)B * T;
  g.ntiles = (nframes + kEsFrames - 1) / kEsFrames;
  size_t want = (size_t)kEsWorkgroups / ((size_t)g.ngroups * g.nz);
  if (want < 1) want = 1;
  g.tps = (g.ntiles + want - 1) / want;
  if (g.tps < (size_t)kEsMinTiles) g.tps = kEsMinTiles;
  g.nspans = (g.ntiles + g.tps - 1) / g.tps;
  return g;
}

struct EsWs {
  double *pw, *pmw, *pmu, *cst;
  float* slab;
};
static size_t es_ws_layout(const EsGeo& g, int S, int C, char* base, EsWs* w) {
  const size_t tab = (size_t)g.PP * g.DP;
  Carver c{base};
  w->pw = c.take<double>(tab);
  w->pmw = c.take<double>(tab);
  w->pmu = c.take<double>(tab);
  w->cst = c.take<double>((size_t)S * C * 2);
  w->slab = c.take<float>(g.nspans * (size_t)g.K * g.PP);
  return c.bytes();
}

// the scorer's tables (gmm_prep_kernel: scales w = exp(-lv/2) and offsets -mu w, fp64, d-major
// [d][PP], K_p and log_w_p) and the means in the same layout; one block per component p < PP,
// the pad components and dims get zeros
__global__ void es_prep_kernel(const float* __restrict__ means, const float* __restrict__ log_vars,
                               const float* __restrict__ log_w, double* __restrict__ pw, double* __restrict__ pmw,
                               double* __restrict__ pmu, double* __restrict__ cst, int P, int PP, int D, int DP) {
  const int p = blockIdx.x;
  if (p >= PP) return;
  for (int d = threadIdx.x; d < DP; d += blockDim.x) {
    double w = 0.0, mw = 0.0, mu = 0.0;
    if (d < D && p < P) {
      mu = (double)means[(size_t)p * D + d];
      w = exp(-0.5 * (double)log_vars[(size_t)p * D + d]);
      mw = -mu * w;
    }
    pw[(size_t)d * PP + p] = w;
    pmw[(size_t)d * PP + p] = mw;
    pmu[(size_t)d * PP + p] = mu;
  }
  if (threadIdx.x == 0 && p < P) {
    double s = 0.0;
    for (int d = 0; d < D; ++d) s += (double)log_vars[(size_t)p * D + d];
    cst[2 * p + 0] = s + (double)D * 1.8378770664093453;  // D*log(2*pi)
    cst[2 * p + 1] = log_w ? (double)log_w[p] : 0.0;
  }
}

// exp(a), a <= 0, to fp32 accuracy from fp64 arguments: expf of the argument rounded to fp32
// times 1 + the rounding's remainder (|a| 2^-24 would otherwise enter the result); below fp32's
// normal range the fp64 exp (rare: a component e^-80 below its state's best)
__device__ __forceinline__ double es_exp(double a) {
  if (a < -80.0) return exp(a);
  const float hi = (float)a;
  return (double)expf(hi) * (1.0 + (a - (double)hi));
}

__global__ void __launch_bounds__(kEsThreads) es_stats_kernel(
    const float* __restrict__ x, const float* __restrict__ weight, const int* __restrict__ lengths,
    const double* __restrict__ pw, const double* __restrict__ pmw, const double* __restrict__ pmu,
    const double* __restrict__ cst, float* __restrict__ slab, int nframes, int T, int D, int NDC, int S, int C,
    int PP, int NC, int ntiles, int tps, int mix_lse) {
  constexpr int CHUNK = kEsFrames * kEsDc;           // doubles per staged chunk
  __shared__ double xs[2][(kEsThreads / 64) * CHUNK];  // [buffer][lane group][frame][dim]
  __shared__ double tq[kEsSub * kEsThreads];           // [lane group][frame][component lane]
  __shared__ double max_s[kEsSub][64];  // the state's largest comp, and 1 / sum_c exp(comp - max)
  __shared__ double inv_s[kEsSub][64];
  __shared__ float wl_s[kEsFrames][64];                // the tile's frame weights [frame][state]
  __shared__ int fvalid[kEsFrames];
  const int tid = threadIdx.x;
  const int NG = kEsThreads / NC;
  const int g = tid / NC, cl = tid - g * NC;
  const int spb = NC / C;  // <= 64
  const int s0 = blockIdx.y * spb;
  const int sl = cl / C, c = cl - sl * C;
  const int s = s0 + sl;
  const bool active = sl < spb && s < S;
  const int p = active ? s * C + c : 0;
  const int z = blockIdx.z;
  const int NSA = (NDC + NG - 1) / NG;  // staging steps of phase A
  const bool skip_a = C == 1;           // one component: r = 1 (0 for log_w = -inf)
  const double kp = cst[2 * p], lw = cst[2 * p + 1];
  const double r_one = (mix_lse && lw == -INFINITY) ? 0.0 : 1.0;

  double sx[kEsKC][kEsDc], sxx[kEsKC][kEsDc], occ = 0.0;
#pragma unroll
  for (int j = 0; j < kEsKC; ++j)
#pragma unroll
    for (int k = 0; k < kEsDc; ++k) sx[j][k] = sxx[j][k] = 0.0;

  const int t_begin = blockIdx.x * tps;
  const int t_end = t_begin + tps < ntiles ? t_begin + tps : ntiles;
  for (int tile = t_begin; tile < t_end; ++tile) {
    const size_t f_begin = (size_t)tile * kEsFrames;
    int ok = 0;
    if (tid < kEsFrames) {
      const size_t frame = f_begin + tid;
      ok = frame < (size_t)nframes;
      if (ok && lengths) {
        const unsigned b = (unsigned)frame / (unsigned)T;
        ok = (int)((unsigned)frame - b * (unsigned)T) < lengths[b];
      }
      fvalid[tid] = ok;
    }
    if (!__syncthreads_or(ok)) continue;  // a tile of padding (uniform: every thread sees the OR)

    // chunks base .. base + NG - 1 of the tile, one per lane group: NG * 256 floats, NG per thread,
    // consecutive threads on consecutive dims of a frame; fp32 -> fp64 on the way into LDS
    float pre[kEsThreads / 64];
    auto fetch = [&](int base) {
#pragma unroll
      for (int j = 0; j < kEsThreads / 64; ++j) {
        if (j < NG) {
          const int e = tid + j * kEsThreads;
          const int k = e & (kEsDc - 1), r = e >> 3;
          const int gg = r % NG, f = r / NG;
          const int d = (base + gg) * kEsDc + k;
          pre[j] = (fvalid[f] && d < D) ? x[(f_begin + f) * D + d] : 0.f;
        }
      }
    };
    auto stage = [&](int buf) {
#pragma unroll
      for (int j = 0; j < kEsThreads / 64; ++j) {
        if (j < NG) {
          const int e = tid + j * kEsThreads;
          const int k = e & (kEsDc - 1), r = e >> 3;
          const int gg = r % NG, f = r / NG;
          xs[buf][(gg * kEsFrames + f) * kEsDc + k] = (double)pre[j];
        }
      }
    };

    // the tile's frame weights are requested now and reach LDS after phase A: their latency passes
    // behind it.  Thread (wave wv, lane sj) takes state s0 + sj of frames wv, wv + 4, ..
    constexpr int kWpt = kEsFrames * 64 / kEsThreads;
    float wpre[kWpt];
    {
      const int sj = tid & 63, ss = s0 + sj;
#pragma unroll
      for (int i = 0; i < kWpt; ++i) {
        const int f = (tid >> 6) + (kEsThreads / 64) * i;
        wpre[i] = (sj < spb && ss < S && fvalid[f]) ? weight[(f_begin + f) * S + ss] : 0.f;
      }
    }

    double wgt[kEsFrames];
    double q[kEsFrames];
    if (!skip_a) {
      // ---- phase A: the quadratic form, z = fma(x, w, -mu w), q = fma(z, z, q) as the scorer
#pragma unroll
      for (int f = 0; f < kEsFrames; ++f) q[f] = 0.0;
      fetch(0);
      for (int i = 0; i < NSA; ++i) {
        // the lane's scales and offsets are requested before the barrier, so part of their L2 round
        // trip passes while the chunk is staged (one wave per SIMD has nothing else to cover it)
        const int dc = i * NG + g;
        double w[kEsDc], mw[kEsDc];
#pragma unroll
        for (int k = 0; k < kEsDc; ++k) {
          w[k] = dc < NDC ? pw[(size_t)(dc * kEsDc + k) * PP + p] : 0.0;
          mw[k] = dc < NDC ? pmw[(size_t)(dc * kEsDc + k) * PP + p] : 0.0;
        }
        stage(i & 1);
        __syncthreads();
        if (i + 1 < NSA) fetch((i + 1) * NG);
        if (dc < NDC) {
          const double2* xb = reinterpret_cast<const double2*>(&xs[i & 1][g * CHUNK]);
          // Two frames at a time, their x read (broadcast: the same address in every lane of the
          // group) while the previous pair is in the FMAs.  The 16 z values are formed first and
          // the two frames' sums then advance in turn: with one wave per SIMD nothing else hides
          // an fp64 FMA that waits on the one just issued.  The fences keep that order.
          double2 xn[2][kEsDc / 2];
#pragma unroll
          for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int k2 = 0; k2 < kEsDc / 2; ++k2) xn[u][k2] = xb[u * (kEsDc / 2) + k2];
#pragma unroll
          for (int f = 0; f < kEsFrames; f += 2) {
            double zz[2][kEsDc];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
              for (int k2 = 0; k2 < kEsDc / 2; ++k2) {
                zz[u][2 * k2] = fma(xn[u][k2].x, w[2 * k2], mw[2 * k2]);
                zz[u][2 * k2 + 1] = fma(xn[u][k2].y, w[2 * k2 + 1], mw[2 * k2 + 1]);
              }
            __builtin_amdgcn_sched_barrier(0);
            if (f + 2 < kEsFrames) {
#pragma unroll
              for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int k2 = 0; k2 < kEsDc / 2; ++k2) xn[u][k2] = xb[(f + 2 + u) * (kEsDc / 2) + k2];
            }
#pragma unroll
            for (int k = 0; k < kEsDc; ++k) {
              q[f] = fma(zz[0][k], zz[0][k], q[f]);
              q[f + 1] = fma(zz[1][k], zz[1][k], q[f + 1]);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }

    // ---- the frame weights w = weight * r, kEsSub frames per round
#pragma unroll
    for (int i = 0; i < kWpt; ++i) wl_s[(tid >> 6) + (kEsThreads / 64) * i][tid & 63] = wpre[i];
    __syncthreads();
#pragma unroll
    for (int f0 = 0; f0 < kEsFrames; f0 += kEsSub) {
      if (!skip_a) {
#pragma unroll
        for (int fi = 0; fi < kEsSub; ++fi) tq[(g * kEsSub + fi) * NC + cl] = q[f0 + fi];
        __syncthreads();
        // this thread sums the groups' partial forms of its own component lane (frames g, g + NG, ..)
        for (int fi = g; fi < kEsSub; fi += NG) {
          double a = 0.0;
          for (int gg = 0; gg < NG; ++gg) a += tq[(gg * kEsSub + fi) * NC + cl];
          tq[fi * NC + cl] = -0.5 * (a + kp) + lw;
        }
        __syncthreads();
      }
      if (!skip_a) {
        for (int pair = tid; pair < kEsSub * spb; pair += kEsThreads) {
          const int fi = pair / spb, sj = pair - fi * spb;
          double m = -INFINITY;
          for (int cc = 0; cc < C; ++cc) m = fmax(m, tq[fi * NC + sj * C + cc]);
          double inv = 0.0;  // every component at -inf: r = 0
          if (m != -INFINITY) {
            double e = 0.0;  // terms <= 1, the largest exactly 1
            for (int cc = 0; cc < C; ++cc) e += es_exp(tq[fi * NC + sj * C + cc] - m);
            inv = 1.0 / e;
          }
          max_s[fi][sj] = m;
          inv_s[fi][sj] = inv;
        }
        __syncthreads();
      }
#pragma unroll
      for (int fi = 0; fi < kEsSub; ++fi) {
        double r = r_one;
        if (!skip_a) {
          const double inv = inv_s[fi][sl & 63];
          r = inv == 0.0 ? 0.0 : es_exp(tq[fi * NC + cl] - max_s[fi][sl & 63]) * inv;
        }
        const float wv = wl_s[f0 + fi][sl & 63];
        wgt[f0 + fi] = (active && wv != 0.f) ? (double)wv * r : 0.0;
      }
      if (!skip_a) __syncthreads();  // (tq, max_s, inv_s are rewritten by the next round)
    }
#pragma unroll
    for (int f = 0; f < kEsFrames; ++f) occ += wgt[f];

    // ---- phase B: the centred moments of this lane's chunks (z * kEsKC + j) * NG + g
    if (z * kEsKC * NG < NDC) fetch(z * kEsKC * NG);
#pragma unroll
    for (int j = 0; j < kEsKC; ++j) {
      const int base = (z * kEsKC + j) * NG;
      if (base < NDC) {  // (uniform)
        const int dc = base + g;
        double mu[kEsDc];  // (requested before the barrier, as in phase A)
#pragma unroll
        for (int k = 0; k < kEsDc; ++k) mu[k] = dc < NDC ? pmu[(size_t)(dc * kEsDc + k) * PP + p] : 0.0;
        stage(j & 1);
        __syncthreads();
        if (j + 1 < kEsKC && base + NG < NDC) fetch(base + NG);
        if (dc < NDC) {
          const double2* xb = reinterpret_cast<const double2*>(&xs[j & 1][g * CHUNK]);
          // a frame's x is read while the previous frame is in the FMAs; the 8 differences, the
          // 8 products and the 16 accumulations go in three passes, so no fp64 operation waits on
          // the one just issued (fences as in phase A)
          double2 xn[kEsDc / 2];
#pragma unroll
          for (int k2 = 0; k2 < kEsDc / 2; ++k2) xn[k2] = xb[k2];
#pragma unroll
          for (int f = 0; f < kEsFrames; ++f) {
            const double wf = wgt[f];
            double diff[kEsDc], wd[kEsDc];
#pragma unroll
            for (int k2 = 0; k2 < kEsDc / 2; ++k2) {
              diff[2 * k2] = xn[k2].x - mu[2 * k2];
              diff[2 * k2 + 1] = xn[k2].y - mu[2 * k2 + 1];
            }
            __builtin_amdgcn_sched_barrier(0);
            if (f + 1 < kEsFrames) {
#pragma unroll
              for (int k2 = 0; k2 < kEsDc / 2; ++k2) xn[k2] = xb[(f + 1) * (kEsDc / 2) + k2];
            }
#pragma unroll
            for (int k = 0; k < kEsDc; ++k) wd[k] = wf * diff[k];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < kEsDc; ++k) sx[j][k] = fma(wf, diff[k], sx[j][k]);
#pragma unroll
            for (int k = 0; k < kEsDc; ++k) sxx[j][k] = fma(wd[k], diff[k], sxx[j][k]);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
  }

  // the span's sums: slab[span][k][p], k = 0 occ, 1 + d sx, 1 + D + d sxx (each slot of a
  // component p < P is written by exactly one lane)
  if (active) {
    float* out = slab + (size_t)blockIdx.x * (2 * D + 1) * PP;
    if (g == 0 && z == 0) out[p] = (float)occ;
#pragma unroll
    for (int j = 0; j < kEsKC; ++j) {
      const int dc = (z * kEsKC + j) * NG + g;
#pragma unroll
      for (int k = 0; k < kEsDc; ++k) {
        const int d = dc * kEsDc + k;
        if (d < D) {
          out[(size_t)(1 + d) * PP + p] = (float)sx[j][k];
          out[(size_t)(1 + D + d) * PP + p] = (float)sxx[j][k];
        }
      }
    }
  }
}

// out[k][p] = the spans' slab entries added in span order (fp64, rounded once)
__global__ void __launch_bounds__(256) es_reduce_kernel(const float* __restrict__ slab, int nspans, int P, int PP,
                                                        int D, float* __restrict__ occ, float* __restrict__ sx,
                                                        float* __restrict__ sxx) {
  const int K = 2 * D + 1;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)K * PP) return;
  const int k = (int)(idx / PP), p = (int)(idx - (size_t)k * PP);
  if (p >= P) return;
  // eight spans' loads in flight, added in span order all the same
  double a = 0.0;
  int sp = 0;
  for (; sp + 8 <= nspans; sp += 8) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = slab[((size_t)(sp + i) * K + k) * PP + p];
#pragma unroll
    for (int i = 0; i < 8; ++i) a += (double)v[i];
  }
  for (; sp < nspans; ++sp) a += (double)slab[((size_t)sp * K + k) * PP + p];
  if (k == 0) {
    if (occ) occ[p] = (float)a;
  } else if (k <= D) {
    if (sx) sx[(size_t)p * D + (k - 1)] = (float)a;
  } else {
    if (sxx) sxx[(size_t)p * D + (k - 1 - D)] = (float)a;
  }
}

static bool es_shape_ok(int B, int T, int D, int S, int C) {
  return B >= 0 && T >= 1 && D >= 1 && D <= kEsDMax && S >= 1 && C >= 1 && C <= 256 && (size_t)S * C <= 65536 &&
         (size_t)B * T <= ((size_t)1 << 31) - kEsFrames;
}

}  // namespace hmm355

using namespace hmm355;

HMM355_API size_t hmm355_gmm_stats_workspace_bytes(int B, int T, int D, int S, int C) {
  if (!es_shape_ok(B, T, D, S, C)) return 0;
  EsWs w;
  return es_ws_layout(es_geo(B, T, D, S, C), S, C, nullptr, &w);
}

HMM355_API int hmm355_gmm_stats_f32(const float* x, const float* weight, const float* means, const float* log_vars,
                                    const float* log_w, const int* lengths, int B, int T, int D, int S, int C,
                                    int mix_lse, float* occ, float* sx, float* sxx, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (B < 0 || T < 0 || D < 1 || S < 1 || C < 1) return HMM355_E_ARG;
  if (C > 256 || (size_t)S * C > 65536) return HMM355_E_STATES;
  if (D > kEsDMax) return HMM355_E_SHAPE;
  if (B == 0) return HMM355_OK;
  if (T < 1 || (size_t)B * T > ((size_t)1 << 31) - kEsFrames) return HMM355_E_SHAPE;
  if (!x || !weight || !means || !log_vars || !workspace) return HMM355_E_ARG;
  if (!mix_lse && C != 1) return HMM355_E_ARG;
  if (workspace_bytes < hmm355_gmm_stats_workspace_bytes(B, T, D, S, C)) return HMM355_E_WORKSPACE;
  const EsGeo g = es_geo(B, T, D, S, C);
  EsWs w;
  es_ws_layout(g, S, C, static_cast<char*>(workspace), &w);
  const int P = S * C;
  hipStream_t st = static_cast<hipStream_t>(stream);
  HMM355_TRY(launch(es_prep_kernel, dim3(g.PP), dim3(64), 0, st, means, log_vars, log_w, w.pw, w.pmw, w.pmu, w.cst, P,
                    g.PP, D, g.DP));
  dim3 grid((unsigned)g.nspans, (unsigned)g.ngroups, (unsigned)g.nz);
  HMM355_TRY(launch(es_stats_kernel, grid, dim3(kEsThreads), 0, st, x, weight, lengths, w.pw, w.pmw, w.pmu, w.cst,
                    w.slab, B * T, T, D, g.NDC, S, C, g.PP, g.NC, (int)g.ntiles, (int)g.tps, mix_lse));
  const size_t total = (size_t)g.K * g.PP;
  return launch(es_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w.slab, (int)g.nspans, P,
                g.PP, D, occ, sx, sxx);
}
