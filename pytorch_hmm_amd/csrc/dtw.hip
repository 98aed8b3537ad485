// hmm355 — dynamic time warping: hard DTW with backtrace, soft-DTW and the soft-DTW gradient.
//
// Replaces the per-cell Python loops of pytorch_hmm.alignment.dtw (compute_dtw_path, dtw.py:61-152;
// DTWAligner._soft_dtw_align, dtw.py:277-299) and the autograd through the latter.
//
// One workgroup per pair runs the whole recursion in one launch; no workgroup waits on another
// and there are no atomics or flags.  A thread owns kDtwRows consecutive rows and walks them four
// columns ("a column block") per step, one block behind the thread above it: at step g thread k
// works on block g - k.  Its own "left" values stay in registers; the last of its rows goes to the
// thread below as one float4 through LDS (double-buffered: one barrier per step, that is per
// 4 * kDtwRows cells of a thread).  The 4 x kDtwRows cells of a step form a small wavefront of
// their own, so the dependent chain of a step is kDtwRows + 3 cells, not all of them.
// When a pair has more rows than one pass covers (kDtwStrip), the passes run one after another;
// the last row of a pass is the "up" input of the next (a row buffer in the workspace, or the
// stored R matrix for soft-DTW).
// A thread reads its rows of D and writes its rows of C as 16-byte pieces (scalar when the row
// stride or the base address is not a multiple of 16 bytes); the loads are issued kDtwAhead
// steps before their use into a register ring (as adjoint.hip does), so memory latency is not on
// the dependent chain.  Nothing is accessed along an anti-diagonal.
//
// Hard DTW: each cell is one fp32 add (rabiner_juang: d + d, exact, then one add per candidate)
// and exact minima, so the cost matrix is bit-identical to the reference's for finite or +inf
// distances.  The backtrace moves to the predecessor of smallest RAW cost, ties in the order
// diagonal, (i-1,j), (i,j-1) (dtw.py:127-143); that direction is recorded while the three
// predecessors are in hand, 2 bits per cell (one byte per row and column block), and one lane
// walks it afterwards through windows of the table staged in LDS.
#include "launch.h"

namespace hmm355 {
namespace {

constexpr int kDtwRows = 4;                          // consecutive rows per thread
constexpr int kDtwThreads = 256;                     // threads per workgroup (one workgroup per pair)
constexpr int kDtwStrip = kDtwRows * kDtwThreads;    // rows per pass of the workgroup
constexpr int kDtwAhead = 4;                         // steps between a load of D and its use
constexpr int kGradAhead = 2;                        // the same for the gradient's loads of R
constexpr int kWalkRows = 128;                       // backtrace window: rows ...
constexpr int kWalkBlocks = 128;                     // ... and column blocks (bytes) per row

constexpr int kModeSym = 0, kModeRJ = 1, kModeSoft = 2;

__device__ __forceinline__ float& comp(float4& v, int x) { return reinterpret_cast<float*>(&v)[x]; }

// softmin_g(a, b, c) = m - g log sum exp(-(c - m) / g), +inf when every candidate is
__device__ __forceinline__ float softmin3(float a, float b, float c, float g, float ig) {
  const float m = fminf(fminf(a, b), c);
  const float ms = m == INFINITY ? 0.f : m;
  const float s = expf((ms - a) * ig) + expf((ms - b) * ig) + expf((ms - c) * ig);
  const float r = ms - g * logf(s);
  return m == INFINITY ? INFINITY : r;
}

struct DtwArgs {
  const float* dist;   // (B,N,M)
  const int* n_len;    // (B) or NULL
  const int* m_len;    // (B) or NULL
  float* cost;         // hard: (B,N,M) or NULL; soft: R (B,N+1,M+1)
  float* total;        // (B)
  unsigned char* dirs; // (B,N,Q) 2-bit directions of four columns per byte, or NULL (no path)
  float* edge;         // (B,4Q) last row of a pass (hard only)
  int* rev_i;          // (B,N+M-1) the walk, end to start
  int* rev_j;
  int* path_i;         // (B,N+M-1)
  int* path_j;
  int* path_len;       // (B)
  int N, M;
  float gamma, inv_gamma;
};

// fill v outside the top-left n x m corner of a row-major (rows x cols) matrix
__device__ __forceinline__ void fill_outside(float* p, int rows, int cols, int n, int m, float v) {
  const int tid = threadIdx.x;
  const size_t lo = (size_t)n * cols, hi = (size_t)rows * cols;
  for (size_t e = lo + tid; e < hi; e += kDtwThreads) p[e] = v;
  if (m < cols) {
    const int l = tid & 63, w = tid >> 6;
    for (int i = w; i < n; i += kDtwThreads / 64)
      for (int j = m + l; j < cols; j += 64) p[(size_t)i * cols + j] = v;
  }
}

template <int MODE>
__global__ void __launch_bounds__(kDtwThreads) dtw_fwd_kernel(DtwArgs a) {
  constexpr int R = kDtwRows, T = kDtwThreads, AH = kDtwAhead;
  constexpr bool SOFT = MODE == kModeSoft;
  __shared__ float4 xch[2][T + 1];
  __shared__ unsigned char win[kWalkRows][kWalkBlocks];
  __shared__ int wpos[4];
  const int k = threadIdx.x;
  const size_t b = blockIdx.x;
  const int N = a.N, M = a.M;
  const int n = seq_len(a.n_len, b, N), m = seq_len(a.m_len, b, M);
  const int Q = (M + 3) >> 2, Qm = (m + 3) >> 2;
  const float* D = a.dist + b * (size_t)N * M;
  const size_t RS = (size_t)M + 1;  // row stride of R
  float* C = nullptr;
  if (a.cost) C = SOFT ? a.cost + b * ((size_t)N + 1) * RS : a.cost + b * (size_t)N * M;
  unsigned char* dirs = (!SOFT && a.dirs) ? a.dirs + b * (size_t)N * Q : nullptr;
  float* edge = SOFT ? nullptr : a.edge + b * (size_t)Q * 4;
  const bool vec_d = (M & 3) == 0 && (reinterpret_cast<uintptr_t>(a.dist) & 15) == 0;
  const bool vec_c = !SOFT && C && (M & 3) == 0 && (reinterpret_cast<uintptr_t>(a.cost) & 15) == 0;
  const float INF = INFINITY;
  const float4 INF4 = make_float4(INF, INF, INF, INF);

  // cells no step writes: outside the pair's corner, and the borders of R
  if (SOFT) {
    for (int j = k; j <= M; j += T) C[j] = j == 0 ? 0.f : INF;
    for (int i = 1 + k; i <= N; i += T) C[(size_t)i * RS] = INF;
    const size_t lo = ((size_t)n + 1) * RS, hi = ((size_t)N + 1) * RS;
    for (size_t e = lo + k; e < hi; e += T) C[e] = INF;
    if (m < M) {
      const int l = k & 63, w = k >> 6;
      for (int i = 1 + w; i <= n; i += T / 64)
        for (int j = m + 1 + l; j <= M; j += 64) C[(size_t)i * RS + j] = INF;
    }
  } else if (C && (n < N || m < M)) {
    fill_outside(C, N, M, n, m, INF);
  }

  for (int s0 = 0; s0 < n; s0 += kDtwStrip) {
    const int rows_here = n - s0 < kDtwStrip ? n - s0 : kDtwStrip;
    const int ka = (rows_here + R - 1) / R;  // threads with a row in this pass
    const int G = Qm + ka - 1;               // steps of this pass
    const int row0 = s0 + k * R;
    const bool act = k < ka;
    const bool more = s0 + kDtwStrip < n;    // another pass follows: thread T-1 keeps its last row
    float c[R];
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = INF;
    float diag0 = (SOFT && s0 == 0 && k == 0) ? 0.f : INF;
    float4 rd[AH][R];
    float4 re[AH];

    auto load_block = [&](int q, float4 (&d)[R], float4& e) __attribute__((always_inline)) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int row = row0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < n) {
          const float* src = D + (size_t)row * M + 4 * q;
          if (vec_d) {
            v = *reinterpret_cast<const float4*>(src);
          } else {
#pragma unroll
            for (int x = 0; x < 4; ++x)
              if (4 * q + x < m) comp(v, x) = src[x];
          }
        }
        d[r] = v;
      }
      if (k == 0 && s0 > 0) {  // the row above this pass
        if (SOFT) {
          float4 v = INF4;
#pragma unroll
          for (int x = 0; x < 4; ++x)
            if (4 * q + x < m) comp(v, x) = C[(size_t)s0 * RS + 4 * q + x + 1];
          e = v;
        } else {
          e = *reinterpret_cast<const float4*>(edge + 4 * q);
        }
      }
    };

    static_for<0, AH>([&](auto ph) {
      const int q = ph.value - k;
      if (act && q >= 0 && q < Qm) load_block(q, rd[ph.value], re[ph.value]);
    });

    auto step = [&](int g, float4 (&d)[R], float4& e) __attribute__((always_inline)) {
      const int q = g - k;
      const bool on = act && q >= 0 && q < Qm;
      float4 in = INF4;
      if (k == 0) {
        if (s0 > 0) in = e;
      } else {
        in = xch[g & 1][k];
      }
      float4 outv = INF4;
      if (on) {
        float pl = diag0;
        float4 p = in;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int row = row0 + r;
          const float l = c[r];
          float4 cur;
          unsigned dbits = 0;
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float dg = x ? comp(p, x - 1) : pl;
            const float u = comp(p, x);
            const float lf = x ? comp(cur, x - 1) : l;
            const float dv = comp(d[r], x);
            float v;
            if (SOFT) {
              v = dv + softmin3(dg, u, lf, a.gamma, a.inv_gamma);
            } else if (MODE == kModeRJ) {
              v = fminf(fminf(dg + (dv + dv), u + dv), lf + dv);
            } else {
              v = dv + fminf(fminf(dg, u), lf);
            }
            if (!SOFT && r == 0 && x == 0 && row == 0 && q == 0) v = dv;  // C[0,0] = D[0,0]
            comp(cur, x) = v;
            if (!SOFT) {  // the predecessor of smallest raw cost: diagonal, up, left; strict <
              unsigned dr = 0;
              float bst = dg;
              if (u < bst) {
                dr = 1;
                bst = u;
              }
              if (lf < bst) dr = 2;
              dbits |= dr << (2 * x);
            }
          }
          if (row < n) {
            if (SOFT) {
#pragma unroll
              for (int x = 0; x < 4; ++x)
                if (4 * q + x < m) C[((size_t)row + 1) * RS + 4 * q + x + 1] = comp(cur, x);
            } else if (C) {
              float* dst = C + (size_t)row * M + 4 * q;
              if (vec_c && 4 * q + 3 < m) {
                *reinterpret_cast<float4*>(dst) = cur;
              } else {
#pragma unroll
                for (int x = 0; x < 4; ++x)
                  if (4 * q + x < m) dst[x] = comp(cur, x);
              }
            }
            if (dirs) dirs[(size_t)row * Q + q] = (unsigned char)dbits;
            if (row == n - 1 && q == Qm - 1) {
              const int xl = (m - 1) & 3;
              a.total[b] = xl == 0 ? cur.x : (xl == 1 ? cur.y : (xl == 2 ? cur.z : cur.w));
            }
          }
          pl = l;
          p = cur;
          c[r] = cur.w;
        }
        diag0 = in.w;
        outv = p;
        if (!SOFT && more && k == T - 1) *reinterpret_cast<float4*>(edge + 4 * q) = outv;
      }
      xch[(g + 1) & 1][k + 1] = outv;
      const int qn = q + AH;
      if (act && qn >= 0 && qn < Qm) load_block(qn, d, e);
      lds_barrier();
    };

    for (int g0 = 0; g0 < G; g0 += AH)
      static_for<0, AH>([&](auto ph) { step(g0 + ph.value, rd[ph.value], re[ph.value]); });

    // the next pass (and the walk) read what this pass stored
    global_barrier();
  }

  if (SOFT || !dirs) return;

  // ---- backtrace (dtw.py:127-150): lane 0 walks windows of the direction table staged in LDS
  const size_t P = (size_t)N + M - 1;
  int* rev_i = a.rev_i + b * P;
  int* rev_j = a.rev_j + b * P;
  int i = n - 1, j = m - 1, cnt = 0;
  if (k == 0) {
    wpos[0] = i;
    wpos[1] = j;
  }
  for (;;) {
    __syncthreads();
    const int wi = wpos[0], wj = wpos[1];
    if (wi <= 0 || wj <= 0) break;
    const int ilo = wi - (kWalkRows - 1) > 1 ? wi - (kWalkRows - 1) : 1;
    const int qb = wj >> 2;
    const int qlo = qb - (kWalkBlocks - 1) > 0 ? qb - (kWalkBlocks - 1) : 0;
    const int wr = wi - ilo + 1, wc = qb - qlo + 1;
    for (int e = k; e < wr * kWalkBlocks; e += T) {
      const int r = e / kWalkBlocks, cc = e % kWalkBlocks;
      if (cc < wc) win[r][cc] = dirs[((size_t)ilo + r) * Q + qlo + cc];
    }
    __syncthreads();
    if (k == 0) {
      while (i >= ilo && j > 0 && (j >> 2) >= qlo) {
        rev_i[cnt] = i;
        rev_j[cnt] = j;
        ++cnt;
        const unsigned dr = (win[i - ilo][(j >> 2) - qlo] >> (2 * (j & 3))) & 3u;
        if (dr != 2) --i;
        if (dr != 1) --j;
      }
      wpos[0] = i;
      wpos[1] = j;
    }
  }
  if (k == 0) {
    // along row 0 or column 0 one predecessor is left
    while (i > 0 || j > 0) {
      rev_i[cnt] = i;
      rev_j[cnt] = j;
      ++cnt;
      if (i > 0) --i; else --j;
    }
    rev_i[cnt] = 0;
    rev_j[cnt] = 0;
    ++cnt;
    wpos[2] = cnt;
    a.path_len[b] = cnt;
  }
  global_barrier();
  const int L = wpos[2];
  int* pi = a.path_i + b * P;
  int* pj = a.path_j + b * P;
  for (size_t t = k; t < P; t += T) {
    const bool in = t < (size_t)L;
    pi[t] = in ? rev_i[L - 1 - t] : -1;
    pj[t] = in ? rev_j[L - 1 - t] : -1;
  }
}

// ------------------------------------------------------------------ soft-DTW gradient
// E = d total / d dist (Cuturi & Blondel 2017, Algorithm 2) over the stored R.  The factor of
// that recursion, e^{(R[s] - R[p] - D[s]) / gamma} for a cell s and its predecessor p, is the
// weight of p in the softmin that formed R[s]; it is evaluated here as that softmax weight,
//   w_s(p) = e^{(m_s - R[p]) / gamma} / sum_{p'} e^{(m_s - R[p']) / gamma},  m_s = min_p' R[p'],
// from the three predecessors' R alone (as autograd through the log-sum-exp does), so a cell with
// one reachable predecessor passes its E on exactly and no R - R - D cancellation is formed.
// The same wavefront as the forward pass, run from the far corner: reversed row rr <-> i = n - rr,
// reversed column cc <-> j = m - cc (indices of R).  A cell adds what (i+1,j), (i,j+1) and
// (i+1,j+1) send it, then sends E w to its own three predecessors: to the cell below it (rr+1:
// (i-1,j)), to its right (cc+1: (i,j-1)) and diagonally.  Between threads the last row's "below"
// and "diagonal" shares travel through LDS; thread 0 of a later pass forms those of the row
// above it again from the stored E and R.
struct GradArgs {
  const float* R;     // (B,N+1,M+1)
  const int* n_len;
  const int* m_len;
  float* E;           // (B,N,M)
  int N, M;
  float inv_gamma;
};

// shares of e sent to the predecessors with soft-DTW values rdg, rup, rlf (none when all are +inf)
__device__ __forceinline__ void grad_shares(float e, float rdg, float rup, float rlf, float ig, float& sdg, float& sup,
                                            float& slf) {
  const float m = fminf(fminf(rdg, rup), rlf);
  const float ms = m == INFINITY ? 0.f : m;
  const float a = expf((ms - rdg) * ig), b = expf((ms - rup) * ig), c = expf((ms - rlf) * ig);
  const float z = a + b + c;
  const float s = m == INFINITY ? 0.f : e / z;
  sdg = a * s;
  sup = b * s;
  slf = c * s;
}

__global__ void __launch_bounds__(kDtwThreads) softdtw_grad_kernel(GradArgs a) {
  constexpr int R = kDtwRows, T = kDtwThreads, AH = kGradAhead;
  __shared__ float4 xu[2][T + 1], xg[2][T + 1];
  const int k = threadIdx.x;
  const size_t b = blockIdx.x;
  const int N = a.N, M = a.M;
  const int n = seq_len(a.n_len, b, N), m = seq_len(a.m_len, b, M);
  const int Qm = (m + 3) >> 2;
  const size_t RS = (size_t)M + 1;
  const float* Rm = a.R + b * ((size_t)N + 1) * RS;
  float* E = a.E + b * (size_t)N * M;
  const float ig = a.inv_gamma;
  const float INF = INFINITY;
  const float4 Z4 = make_float4(0.f, 0.f, 0.f, 0.f);

  if (n < N || m < M) fill_outside(E, N, M, n, m, 0.f);

  for (int s0 = 0; s0 < n; s0 += kDtwStrip) {
    const int rows_here = n - s0 < kDtwStrip ? n - s0 : kDtwStrip;
    const int ka = (rows_here + R - 1) / R;
    const int G = Qm + ka - 1;
    const int rr0 = s0 + k * R;
    const bool act = k < ka;
    float cLf[R], cDg[R];  // what the cell left of this block sent right / diagonally, per row
#pragma unroll
    for (int r = 0; r < R; ++r) cLf[r] = cDg[r] = 0.f;
    float diag0 = 0.f;
    float rv[AH][R + 1][5];  // R of rows i .. i-R and columns j .. j-4 of a block
    float4 ea[AH], ra[AH];   // thread 0 of a later pass: E and R[., j-1] of the row above

    auto load_block = [&](int q, float (&v)[R + 1][5], float4& e_up, float4& r_up) __attribute__((always_inline)) {
#pragma unroll
      for (int r = 0; r <= R; ++r) {
        const int rr = rr0 + r;
#pragma unroll
        for (int x = 0; x < 5; ++x) {
          const int cc = 4 * q + x;
          v[r][x] = (rr <= n && cc <= m) ? Rm[(size_t)(n - rr) * RS + (size_t)(m - cc)] : INF;
        }
      }
      if (k == 0 && s0 > 0) {
        const size_t iu = (size_t)(n - s0) + 1;
        float4 te = Z4, tr = make_float4(INF, INF, INF, INF);
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int cc = 4 * q + x;
          if (cc < m) {
            comp(te, x) = E[(iu - 1) * M + (size_t)(m - cc - 1)];
            comp(tr, x) = Rm[iu * RS + (size_t)(m - cc - 1)];
          }
        }
        e_up = te;
        r_up = tr;
      }
    };

    static_for<0, AH>([&](auto ph) {
      const int q = ph.value - k;
      if (act && q >= 0 && q < Qm) load_block(q, rv[ph.value], ea[ph.value], ra[ph.value]);
    });

    auto step = [&](int g, float (&v)[R + 1][5], float4& e_up, float4& r_up) __attribute__((always_inline)) {
      const int q = g - k;
      const bool on = act && q >= 0 && q < Qm;
      float4 in_up = Z4, in_dg = Z4;
      if (k == 0) {
        if (s0 > 0 && on) {
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            float slf;
            grad_shares(comp(e_up, x), v[0][x + 1], v[0][x], comp(r_up, x), ig, comp(in_dg, x), comp(in_up, x), slf);
          }
        }
      } else {
        in_up = xu[g & 1][k];
        in_dg = xg[g & 1][k];
      }
      float4 out_up = Z4, out_dg = Z4;
      if (on) {
        float4 p_up = in_up, p_dg = in_dg;
        float pl_dg = diag0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int rr = rr0 + r;
          float4 c_up, c_dg, c_lf, ev;
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            const float f_lf = x ? comp(c_lf, x - 1) : cLf[r];
            const float f_dg = x ? comp(p_dg, x - 1) : pl_dg;
            float e = comp(p_up, x) + f_lf + f_dg;
            if (r == 0 && x == 0 && rr == 0 && q == 0) e = v[0][0] < INF ? 1.f : 0.f;  // E[n,m] = 1
            comp(ev, x) = e;
            grad_shares(e, v[r + 1][x + 1], v[r + 1][x], v[r][x + 1], ig, comp(c_dg, x), comp(c_up, x), comp(c_lf, x));
          }
          if (rr < n) {
            const size_t i = (size_t)(n - rr);
#pragma unroll
            for (int x = 0; x < 4; ++x) {
              const int cc = 4 * q + x;
              if (cc < m) E[(i - 1) * M + (size_t)(m - cc - 1)] = comp(ev, x);
            }
          }
          pl_dg = cDg[r];
          cDg[r] = c_dg.w;
          cLf[r] = c_lf.w;
          p_up = c_up;
          p_dg = c_dg;
        }
        diag0 = in_dg.w;
        out_up = p_up;
        out_dg = p_dg;
      }
      xu[(g + 1) & 1][k + 1] = out_up;
      xg[(g + 1) & 1][k + 1] = out_dg;
      const int qn = q + AH;
      if (act && qn >= 0 && qn < Qm) load_block(qn, v, e_up, r_up);
      lds_barrier();
    };

    for (int g0 = 0; g0 < G; g0 += AH)
      static_for<0, AH>([&](auto ph) { step(g0 + ph.value, rv[ph.value], ea[ph.value], ra[ph.value]); });

    global_barrier();
  }
}

// edge (B,4Q) fp32 | dirs (B,N,Q) bytes | rev_i | rev_j (B,N+M-1) int32, pieces 256-B aligned;
// false on overflow
struct DtwWs {
  float* edge;
  unsigned char* dirs;
  int *rev_i, *rev_j;
  size_t total;
};
bool mul_ok(size_t a, size_t b, size_t* out) { return !__builtin_mul_overflow(a, b, out); }

bool dtw_layout(int B, int N, int M, unsigned flags, char* base, DtwWs* w) {
  const size_t Q = ((size_t)M + 3) / 4, P = (size_t)N + M - 1;
  const size_t lim = (size_t)1 << 46;
  size_t cells, edge, dirs = 0, rev = 0;
  if (!mul_ok((size_t)N, (size_t)M, &cells) || !mul_ok(cells, (size_t)(B > 0 ? B : 1), &cells) || cells > lim) return false;
  if (!mul_ok((size_t)(B > 0 ? B : 1), Q * 16, &edge)) return false;
  if (flags & HMM355_DTW_PATH) {
    if (!mul_ok((size_t)B * N, Q, &dirs) || !mul_ok((size_t)B, P * 4, &rev) || dirs > lim || rev > lim) return false;
  }
  Carver c{base};
  w->edge = c.take<float>(edge / sizeof(float));
  w->dirs = c.take<unsigned char>(dirs);
  w->rev_i = c.take<int>(rev / sizeof(int));
  w->rev_j = c.take<int>(rev / sizeof(int));
  w->total = c.bytes();
  return true;
}

int dtw_shape_check(int B, int N, int M) {
  if (B < 0 || N < 0 || M < 0) return HMM355_E_ARG;
  if (N < 1 || M < 1) return HMM355_E_SHAPE;
  if ((size_t)N + (size_t)M - 1 > (size_t)0x7fffffff) return HMM355_E_SHAPE;
  size_t cells;
  // the (N+1) x (M+1) table of every pair, in bytes, fits a size_t with room to spare
  if (!mul_ok((size_t)N + 1, (size_t)M + 1, &cells) || !mul_ok(cells, (size_t)(B > 0 ? B : 1), &cells) ||
      cells > ((size_t)1 << 46))
    return HMM355_E_SHAPE;
  return HMM355_OK;
}

}  // namespace
}  // namespace hmm355

using namespace hmm355;

HMM355_API size_t hmm355_dtw_workspace_bytes(int B, int N, int M, unsigned flags) {
  if (dtw_shape_check(B, N, M) != HMM355_OK) return 0;
  if (flags & ~HMM355_DTW_PATH) return 0;
  DtwWs w;
  if (!dtw_layout(B, N, M, flags, nullptr, &w)) return 0;
  return w.total;
}

HMM355_API int hmm355_dtw_f32(const float* dist, const int* n_len, const int* m_len, int B, int N, int M, int pattern,
                              unsigned flags, float* cost_matrix, float* total, int* path_i, int* path_j,
                              int* path_len, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = dtw_shape_check(B, N, M);
  if (rc != HMM355_OK) return rc;
  if (pattern != HMM355_DTW_SYMMETRIC && pattern != HMM355_DTW_ASYMMETRIC && pattern != HMM355_DTW_RABINER_JUANG)
    return HMM355_E_ARG;
  if (flags & ~HMM355_DTW_PATH) return HMM355_E_ARG;
  if (B == 0) return HMM355_OK;
  if (!dist || !total || !workspace) return HMM355_E_ARG;
  const bool want_path = (flags & HMM355_DTW_PATH) != 0;
  if (want_path && (!path_i || !path_j || !path_len)) return HMM355_E_ARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return HMM355_E_ARG;
  DtwWs w;
  if (!dtw_layout(B, N, M, flags, static_cast<char*>(workspace), &w)) return HMM355_E_SHAPE;
  if (workspace_bytes < w.total) return HMM355_E_WORKSPACE;
  DtwArgs a{};
  a.dist = dist;
  a.n_len = n_len;
  a.m_len = m_len;
  a.cost = cost_matrix;
  a.total = total;
  a.edge = w.edge;
  if (want_path) {
    a.dirs = w.dirs;
    a.rev_i = w.rev_i;
    a.rev_j = w.rev_j;
    a.path_i = path_i;
    a.path_j = path_j;
    a.path_len = path_len;
  }
  a.N = N;
  a.M = M;
  hipStream_t sm = static_cast<hipStream_t>(stream);
  // asymmetric: min(c + d) = d + min(c) in fp32 (the add is monotone), the symmetric kernel
  if (pattern == HMM355_DTW_RABINER_JUANG)
    return launch(dtw_fwd_kernel<kModeRJ>, dim3(B), dim3(kDtwThreads), 0, sm, a);
  return launch(dtw_fwd_kernel<kModeSym>, dim3(B), dim3(kDtwThreads), 0, sm, a);
}

static bool gamma_ok(float g) { return g > 0.f && g < INFINITY; }

HMM355_API int hmm355_softdtw_f32(const float* dist, const int* n_len, const int* m_len, int B, int N, int M,
                                  float gamma, float* R, float* total, void* stream) {
  const int rc = dtw_shape_check(B, N, M);
  if (rc != HMM355_OK) return rc;
  if (!gamma_ok(gamma)) return HMM355_E_ARG;
  if (B == 0) return HMM355_OK;
  if (!dist || !R || !total) return HMM355_E_ARG;
  DtwArgs a{};
  a.dist = dist;
  a.n_len = n_len;
  a.m_len = m_len;
  a.cost = R;
  a.total = total;
  a.N = N;
  a.M = M;
  a.gamma = gamma;
  a.inv_gamma = (float)(1.0 / (double)gamma);
  return launch(dtw_fwd_kernel<kModeSoft>, dim3(B), dim3(kDtwThreads), 0, static_cast<hipStream_t>(stream), a);
}

HMM355_API int hmm355_softdtw_grad_f32(const float* dist, const float* R, const int* n_len, const int* m_len, int B,
                                       int N, int M, float gamma, float* E, void* stream) {
  const int rc = dtw_shape_check(B, N, M);
  if (rc != HMM355_OK) return rc;
  if (!gamma_ok(gamma)) return HMM355_E_ARG;
  if (B == 0) return HMM355_OK;
  if (!dist || !R || !E) return HMM355_E_ARG;
  // (dist is part of the signature; the weights are functions of R alone)
  GradArgs a{R, n_len, m_len, E, N, M, (float)(1.0 / (double)gamma)};
  return launch(softdtw_grad_kernel, dim3(B), dim3(kDtwThreads), 0, static_cast<hipStream_t>(stream), a);
}
