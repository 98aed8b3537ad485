/*
 * hmm355 — MI355X (gfx950) HMM inference core: the C ABI.
 *
 * This is the drop-in boundary for the hot path of crlotwhite/pytorch_hmm.  The reference
 * is pure Python over ATen (no FFI of its own); each entry point below replaces the
 * per-time-step Python loop of one reference routine (file:line into
 * /root/reference/pytorch_hmm) and is what a binding (ctypes, pybind11, or the
 * torch.library custom ops in pytorch_hmm_amd/ops.py) calls.
 *
 * Conventions (all entry points)
 *   - Plain device pointers and sizes; no framework types.  Every buffer is caller-owned
 *     device memory (hipMalloc / torch allocator); the library allocates nothing.
 *   - Output and workspace buffers may hold anything on entry: every entry point writes each
 *     byte of its workspace and outputs before it reads it, and writes every element of every
 *     output it was asked for (tests/test_gpu_poison.py).
 *   - Dense row-major fp32, (B, T, N) = batch, time, states; states int64 (B, T).
 *   - `stream` is a hipStream_t (NULL = legacy default stream).  Launches are
 *     stream-ordered and asynchronous; there is no host synchronisation and no global
 *     mutable state, so calls are re-entrant and may run concurrently on different streams
 *     (and may be captured into a hipGraph).
 *   - Return 0 on success, a negative HMM355_E* code on a rejected argument (nothing is
 *     launched), or a positive hipError_t if a launch failed.  hmm355_strerror() names it.
 *   - Supported sizes: T >= 1, B >= 0 (B == 0 is a no-op).  States: 1 <= N <= 256 for the
 *     recursions that run one workgroup per sequence (padded internally to 64/128/256), and
 *     1 <= N <= 4096 for the batch-tiled hmm355_viterbi_wide_f32 /
 *     hmm355_forward_backward_wide_f32 (one launch per time step, no padding).
 */
#ifndef HMM355_H
#define HMM355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMM355_OK 0
#define HMM355_E_ARG (-1)       /* null pointer or negative size                      */
#define HMM355_E_STATES (-2)    /* N outside the entry point's range ([1, 256]; *_wide [1, 4096]; CTC Lmax [1, 2048]; DCHMM S [1, 256], group*S <= 4096; forced alignment Smax [1, 4096]; explicit-duration forced alignment Lmax [1, 1024], Dmax [1, 128], Lmax*Dmax <= 16384; posterior path sampling hmm355_ffbs_f32 [1, 256]; emission statistics hmm355_gmm_stats_f32 C [1, 256], S*C <= 65536; N-best Viterbi hmm355_viterbi_nbest_f32 N [1, 256], K <= 16; arc-list recursions hmm355_sparse_* N [1, HMM355_SPARSE_MAX_STATES = 8192], with E outside [1, HMM355_SPARSE_MAX_ARCS = 2^20] an HMM355_E_SHAPE) */
#define HMM355_E_SHAPE (-3)     /* T < 1 (DTW: N < 1 or M < 1), or a size product overflows */
#define HMM355_E_WORKSPACE (-4) /* workspace smaller than *_workspace_bytes() reports   */
#define HMM355_E_DURATION (-5)  /* HSMM max_duration outside [1, 1024] (hmm355_hsmm_fb_f32: [1, 128], S * Dmax <= 16384) */

/* Emission encodings accepted by the recursions. */
#define HMM355_OBS_PROB 0   /* x is a probability: the kernel uses log(x + 1e-8) / x + 1e-8 (hmm.py:86,152) */
#define HMM355_OBS_LOG 1    /* x is already a log-emission (mixture_gaussian.py:354, hsmm.py:225)           */

/* forward_backward output mask bits */
#define HMM355_FB_POSTERIOR 1u   /* posterior (B,T,N)              hmm.py:120-126 */
#define HMM355_FB_FORWARD 2u     /* forward = exp(log alpha)        hmm.py:127     */
#define HMM355_FB_BACKWARD 4u    /* backward = exp(log beta)        hmm.py:128     */
/* Hint (forward_backward with a plan, no log_beta_T): the plan is banded in both directions
 * (hmm355_plan_banded() returned 1).  Both chains of a sequence then run in one workgroup and
 * form posterior / forward / backward inside it (csrc/fbpair.h): the scaled rows are not
 * written back in full, so the workspace does NOT hold U / V / LA / LB afterwards.  A wrong
 * hint still gives correct results (slower).  N <= 128; ignored otherwise. */
#define HMM355_FB_PAIR 0x100u
/* Hint (forward_backward with a plan): the caller read hmm355_plan_banded(plan) == 1.  The chains
 * then publish their rows as they go and extra workgroups (two per sequence while 4B workgroups
 * fit the device, else one) form the posterior (and the chain forms lik_ref) inside the chains'
 * own launch, instead of a pass after them (csrc/follow.h).  Needs HMM355_FB_POSTERIOR; ignored
 * when the 3B workgroups would not fit the device at once.  Passing it with a plan that is not banded is a caller error: posterior and
 * lik_ref come back NaN. */
#define HMM355_FB_PLAN_BANDED 0x200u
/* With HMM355_FB_PLAN_BANDED and T >= 256 each chain's own workgroup forms the posterior of the
 * rows of its last two 16-step blocks (the first 17..32 times for the backward chain, the last
 * for the forward chain) from the rows still in its LDS when it ends, instead of handing them to
 * the followers through memory (csrc/recur.h rec_band, end rows).  Results are bit-identical
 * with and without.  Two switches for tests and A/B timing:
 * NO_END_ROWS turns that off (the followers form every row); END_ROWS_ODD_LEFT makes the chains
 * leave the end rows of every odd 16-step block to the followers, the path taken when a partner
 * chain's rows are not yet published. */
#define HMM355_FB_NO_END_ROWS 0x400u
#define HMM355_FB_END_ROWS_ODD_LEFT 0x800u

const char* hmm355_strerror(int code);
int hmm355_version(void);

/* ---------------------------------------------------------------------------------
 * Forward-backward.  Replaces HMMPyTorch.forward_backward (hmm.py:66-130) and the
 * likelihood of HMMPyTorch.compute_likelihood (hmm.py:186-211).
 *   obs        (B,T,N) emissions, encoding `obs_mode`
 *   log_P      (N,N) log transition matrix, exactly as the reference holds it
 *              (log(P/rowsum + 1e-8), hmm.py:39-42, or hmm_layer.py:84)
 *   log_p0     (N) log initial distribution (hmm.py:55 / hmm_layer.py:86)
 *   posterior, forward, backward  (B,T,N) outputs, written iff the mask bit is set
 *   loglik     (B) or NULL: log sum_j alpha_{T-1}[j] (the well-defined sequence
 *              log-likelihood the reference's exp() underflow hides)
 *   lik_ref    (B) or NULL: the reference's compute_likelihood value
 *              logsumexp_j(log(exp(log alpha_{T-1}[j]) + 1e-8))  (hmm.py:206)
 *   workspace  >= hmm355_fb_workspace_bytes(B,T,N) bytes of device memory
 *
 * Range contract of every sum-product entry point of this library (forward-backward: plan, ex,
 * ragged, wide, tv; the sparse sums and arc counts).  State probabilities are fp32, rescaled once
 * per step by one factor for the whole row, and with HMM355_OBS_LOG a frame's emissions are
 * e_t = exp(obs_t - M_t) with M_t the maximum over ALL states: a state more than about 87 nats
 * behind its row's leader is exactly 0.  The results are those of the exact sums (to fp32
 * rounding) whenever the leader can pass its mass on -- always with a floored table
 * (log(P + 1e-8): the leader refills every state at -18.4 nats per step).  With exact zeros
 * (-inf) in log_P or log_p0 the leader may be a state that no path reaches or that leads
 * nowhere; the states that carry the sequence's probability are then flushed and a feasible
 * sequence comes back with loglik -inf and a zero posterior, or with a finite but wrong loglik.
 * Such a call still fails cleanly: no NaN in loglik, posterior, forward or backward (nor in the
 * sparse arc counts), loglik finite or -inf, every posterior row a distribution or all zero
 * (csrc/common.h rcp_normal / row_value / clean_loglik), other sequences of the batch
 * untouched.  These entry points do not detect the condition.  The rows they leave (U, V, CA
 * below; the sparse workspace) are enough to: pytorch_hmm_amd/range_guard.py flags the affected
 * sequences from them and recomputes those in float64 log space, and the package's E-step and
 * likelihood entry points do so by default.  The batch-tiled form (wide, N > 256)
 * leaves no such rows to the package: it stays unguarded.
 * ------------------------------------------------------------------------------ */
size_t hmm355_fb_workspace_bytes(int B, int T, int N);
/* Same as hmm355_forward_backward_f32 with a custom terminal backward vector:
 *   log_beta_T (B,N) or NULL: log beta_{T-1} (NULL = 0, the reference's beta_{T-1} = 1,
 *              hmm.py:105).  With log_beta_T = log(dL/d log alpha_{T-1}) - log alpha_{T-1}
 *              the backward pass is the adjoint of the forward recursion for a loss L of
 *              alpha_{T-1}: dL/d log_obs_t = G * posterior_t with G = sum_j dL/d log alpha_{T-1,j}
 *              (pytorch_hmm_amd/autograd.py; replaces the reference's autograd through
 *              hmm.py:89-101 for compute_likelihood / HMMLayer.compute_loss, hmm_layer.py:144-173).
 * Workspace layout (256-B aligned pieces, in order): U (B,T,NP) scaled alpha rows | V
 * (B,T,NP) scaled beta rows | LA (B,T) | LB (B,T) | BandDesc (hmm355_plan_bytes(N)) |
 * (B,NP) | (B) | (B,T) | CA (B,T) | CB (B,T); alpha_t = U_t exp(LA_t), beta_t = V_t exp(LB_t),
 * NP = N padded to 64/128/256.  CA / CB are the steps' normalisers by time:
 * U_{t+1} = (A^T U_t) e_{t+1} / CA_t  (t <= T-2)  and  V_{t-1} = A (e_t V_t) / CB_t  (t >= 1),
 * A = exp(log_P) -- the chains do not normalise every row to sum 1 (the dense chain applies a
 * scale predicted a step ahead), so an adjoint takes its step factors from CA / CB.  With obs_mode == HMM355_OBS_LOG
 * the chains use the shifted emissions e_t = exp(obs_t - M_t), M_t = max_j obs_t[j] (a row
 * without a finite maximum: M_t = 0), and LA / LB carry the shifts, so log-emissions far
 * below -87 do not underflow; U and V are the rows of that shifted recursion. */
/* Byte offsets of the workspace pieces above, in order U, V, LA, LB, BandDesc, beta init, its
 * scale, row maxima M, CA, CB (offsets[10]), for callers that read U / V / LA / LB / CA / CB back
 * (pytorch_hmm_amd/autograd.py); 0 or an HMM355_E_* code. */
int hmm355_fb_workspace_layout(int B, int T, int N, size_t* offsets);
int hmm355_forward_backward_ex_f32(const float* obs, int obs_mode, const float* log_P,
                                   const float* log_p0, const float* log_beta_T, int B, int T, int N,
                                   unsigned out_mask, float* posterior, float* forward,
                                   float* backward, float* loglik, float* lik_ref, void* workspace,
                                   size_t workspace_bytes, void* stream);
int hmm355_forward_backward_f32(const float* obs, int obs_mode, const float* log_P,
                                const float* log_p0, int B, int T, int N, unsigned out_mask,
                                float* posterior, float* forward, float* backward,
                                float* loglik, float* lik_ref, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Adjoint of forward-backward's outputs (posterior / forward / backward).  Replaces the
 * reference's autograd through its log-space loops (hmm.py:89-130) when a loss of the
 * posteriors is back-propagated (HMMLayer training mode, hmm_layer.py:119-121; the
 * supervised cross-entropy of compute_loss, :159-165).  Two linear chains per sequence:
 *   W_{T-1} = Sw_{T-1};  W_{t-1}[i] = Sw_{t-1}[i] + Fw_{t-1} * sum_j A[i][j] E_t[j] W_t[j]
 *   Z_0 = Sz_0;          Z_{t+1}[j] = Sz_{t+1}[j] + P_{t+1}[j],
 *                        P_{t+1}[j] = Fz_{t+1} * E_{t+1}[j] * sum_i Z_t[i] A[i][j]
 * with A = exp(log_P).  E, src_w (Sw), src_z (Sz) are (B,T,N); scale_w (Fw), scale_z (Fz)
 * are (B,T) (Fw[T-1] and Fz[0] are not read).  Outputs W (B,T,N) and P (B,T,N), P_0 = 0.
 * pytorch_hmm_amd/autograd.py (ForwardBackwardFn) forms the sources from the output
 * gradients and the stored scaled rows, and the parameter gradients from W and Z.
 * ------------------------------------------------------------------------------ */
int hmm355_fb_adjoint_f32(const float* E, const float* log_P, const float* src_w,
                          const float* scale_w, const float* src_z, const float* scale_z,
                          int B, int T, int N, float* W, float* P, void* stream);

/* ---------------------------------------------------------------------------------
 * Transition plan: the banded decomposition of log_P (csrc/band.h) measured once into
 * caller-owned device memory (hmm355_plan_bytes(N) bytes), for callers whose matrix is fixed
 * across calls (HMMPyTorch computes log_P once in __init__, hmm.py:39-42).  The *_plan_f32
 * entry points use it instead of re-measuring the matrix on every call; plan == NULL
 * behaves exactly as the plain entry points.  A plan is valid for the log_P it was made
 * from; the results are identical with or without it.
 * ------------------------------------------------------------------------------ */
size_t hmm355_plan_bytes(int N);
int hmm355_plan_f32(const float* log_P, int N, void* plan, void* stream);
/* As hmm355_plan_f32 with flags.  HMM355_PLAN_DENSE: the plan selects the dense chains for every
 * recursion whatever the matrix's structure (hmm355_plan_banded then reads 0): the two chain
 * families give the same results, and parity tests run both on one matrix. */
#define HMM355_PLAN_DENSE 0x1u
int hmm355_plan_ex_f32(const float* log_P, int N, unsigned flags, void* plan, void* stream);
/* 1 if the plan selects banded chains for both the forward and the backward recursion (the
 * condition for HMM355_FB_PAIR), 0 if not, < 0 on error.  Synchronous: waits for `stream`
 * and copies a few bytes of the plan to the host (call once per plan, not per step). */
int hmm355_plan_banded(const void* plan, void* stream);
int hmm355_forward_backward_plan_f32(const float* obs, int obs_mode, const float* log_P,
                                     const float* log_p0, const void* plan,
                                     const float* log_beta_T, int B, int T, int N,
                                     unsigned out_mask, float* posterior, float* forward,
                                     float* backward, float* loglik, float* lik_ref,
                                     void* workspace, size_t workspace_bytes, void* stream);
int hmm355_viterbi_plan_f32(const float* obs, int obs_mode, const float* log_P, const float* init,
                            const void* plan, int B, int T, int N, int64_t* states,
                            float* log_delta, float* final_score, void* workspace,
                            size_t workspace_bytes, void* stream);
/* Viterbi with flags.  HMM355_VIT_PLAN_BANDED: the caller read hmm355_plan_banded(plan) == 1 for
 * this plan.  For N > 64 the decode then finishes inside the chain's own launch (csrc/follow.h):
 * one extra workgroup per sequence forms log(x + 1e-8) of the emissions ahead of the chain
 * (OBS_PROB), composes the 64-step chunk maps from the psi rows the chain publishes, and
 * backtraces the path once the chain is done -- one launch instead of four.  Ignored when the 2B
 * workgroups would not fit the device at once or T exceeds what the follower's LDS holds:
 * csrc/follow.h vit_follow_lds_bytes(T, NP) <= 160 KiB, that is ceil(T / 64) * (NP + 4) <= 98240
 * with NP = 128 for N <= 128 and 256 above -- T <= 47616 and T <= 24128.  (The follower keeps its
 * end-state table, which spares the walk over the chunk maps at the end, while that fits as well:
 * vit_follow_lds_bytes(T, NP, true) <= 160 KiB, T <= 16128 and T <= 8000.)  Passing the flag with a plan that is not banded
 * is a caller error: the states come back as -1 and the final score as NaN. */
#define HMM355_VIT_PLAN_BANDED 0x1u
/* HMM355_VIT_PLAN_DENSE: the caller read hmm355_plan_banded(plan) == 0.  Then, for N <= 128, the
 * argmax pointers of each 64-step chunk are computed while the chain still runs, by workgroups
 * of the chain's own launch on the CUs the chain leaves idle (they follow the rows the chain
 * has flushed; a chunk they did not finish is computed by the pass after the chain, so the
 * result never depends on their timing).  Without the flag the pointers are computed after the
 * chain.  With HMM355_OBS_PROB the emissions' log(x + 1e-8) is formed in one full-tensor pass
 * into the workspace first.  The flag with a banded plan only costs the idle launch. */
#define HMM355_VIT_PLAN_DENSE 0x2u
int hmm355_viterbi_plan_ex_f32(const float* obs, int obs_mode, const float* log_P, const float* init,
                               const void* plan, unsigned flags, int B, int T, int N, int64_t* states,
                               float* log_delta, float* final_score, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Viterbi.  Replaces HMMPyTorch.viterbi_decode (hmm.py:132-184) and
 * MixtureGaussianHMMLayer._viterbi_decode (mixture_gaussian.py:290-338).
 *   init       (N) additive t=0 vector: log_p0 (hmm.py:159), or -log(S) per state
 *              (mixture_gaussian.py:312; lp + (-c) == lp - c exactly in fp32)
 *   states     (B,T) int64: backtraced path, first index on ties (hmm.py:167,174)
 *   log_delta  (B,T,N) fp32: the trellis the reference returns as `scores`
 *   final_score (B) or NULL: max_j delta_{T-1}[j] (mixture_gaussian.py:327)
 *   workspace  >= hmm355_viterbi_workspace_bytes(B,T,N) bytes
 * Given identical fp32 log-emissions and log_P the result is bit-identical to the
 * reference's (every delta is one fp32 add of an exact max).
 * ------------------------------------------------------------------------------ */
size_t hmm355_viterbi_workspace_bytes(int B, int T, int N);
/* The size for one emission encoding: HMM355_OBS_LOG decodes need no log-emission buffer
 * (B*T*N*4 bytes less); hmm355_viterbi_workspace_bytes is the HMM355_OBS_PROB (larger) size. */
size_t hmm355_viterbi_workspace_bytes_ex(int B, int T, int N, int obs_mode);
int hmm355_viterbi_f32(const float* obs, int obs_mode, const float* log_P, const float* init,
                       int B, int T, int N, int64_t* states, float* log_delta,
                       float* final_score, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------
 * Batch-tiled ("wide") Viterbi and forward-backward, 1 <= N <= 4096 (csrc/wide.hip).  Arguments,
 * conventions and results as hmm355_viterbi_f32 / hmm355_forward_backward_f32 (the Viterbi
 * trellis and path are bit-identical to theirs; OBS_PROB decodes use the same correctly
 * rounded log(x + 1e-8)); N outside [1, 4096] returns HMM355_E_STATES and the size queries 0.
 * All B sequences share log_P, so one time step of the batch is a (B,N).(N,N) product tiled over
 * 64 output columns and 2 sequences per workgroup; consecutive time steps are separate launches
 * on `stream` (T + 1 or T + 2 launches for a decode, T + 3 or T + 4 for forward-backward), so a call's host time
 * grows with T.  No plan, no log_beta_T (gradients stay with N <= 256), no padding: the
 * workspace rows have stride N.
 *   Viterbi workspace: psi (B,T,N) uint16 | log-emissions (B,T,N) fp32 (OBS_PROB only).
 *   Forward-backward workspace: A = exp(log_P) | A^T (N,N) | U | V (B,T,N) raw alpha / beta rows
 *   | SA | SB | M (B,T) fp32 | CLA | CLB (B,T) fp64, pieces 256-B aligned.  U_{t+1} =
 *   (A^T (U_t / SA_t)) e_{t+1} with SA_t = sum_j U_t[j]; V_{t-1} = A (e_t V_t / SB_t) with SB_t =
 *   sum_j e_t[j] V_t[j]; e_t as in hmm355_forward_backward_ex_f32 (x + 1e-8, or exp(x - M_t));
 *   log alpha_t = log U_t + CLA_t, log beta_t = log V_t + CLB_t (the log-scales, summed in fp64).
 * ------------------------------------------------------------------------------ */
size_t hmm355_viterbi_wide_workspace_bytes(int B, int T, int N, int obs_mode);
int hmm355_viterbi_wide_f32(const float* obs, int obs_mode, const float* log_P, const float* init,
                            int B, int T, int N, int64_t* states, float* log_delta,
                            float* final_score, void* workspace, size_t workspace_bytes,
                            void* stream);
size_t hmm355_fb_wide_workspace_bytes(int B, int T, int N);
int hmm355_forward_backward_wide_f32(const float* obs, int obs_mode, const float* log_P,
                                     const float* log_p0, int B, int T, int N, unsigned out_mask,
                                     float* posterior, float* forward, float* backward,
                                     float* loglik, float* lik_ref, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Padded batches with per-sequence lengths ("ragged", csrc/ragged.hip), 1 <= N <= 256.  Sequence b
 * is the first lengths[b] frames of row b; the result is what hmm355_viterbi_f32 /
 * hmm355_forward_backward_ex_f32 give for obs[b, :lengths[b]] alone.  Arguments and conventions
 * as theirs, plus
 *   lengths   (B) int32 device array.  The caller guarantees 1 <= lengths[b] <= T (the Python
 *             layer checks it on the host); the kernels clamp what they read to that range.
 * One workgroup per sequence and job (alpha chain, beta chain; Viterbi chain), each running
 * exactly lengths[b] steps; no workgroup waits on another, no flags, no floating-point atomics:
 * two calls on the same inputs return the same bits.  No plan.
 * Padded frames t >= lengths[b]: the input there is never read (it may hold NaN or +-inf) and no
 * output, workspace piece or gradient of any sequence depends on it.  posterior, forward and
 * backward are 0 there, log_delta is -inf and states is -1.
 *
 * hmm355_viterbi_ragged_f32: delta_0 = init + lo_0, delta_t[j] = fl(max_i fl(delta_{t-1}[i] +
 *   log_P[i][j]) + lo_t[j]), first index on ties, a column without a finite candidate index 0
 *   (hmm.py:154-184); lo = log(x + 1e-8) correctly rounded for HMM355_OBS_PROB.  states and
 *   log_delta of the valid frames are bit-identical to hmm355_viterbi_f32's on the slice.
 *   states[b, lengths[b]-1] = the first argmax of delta[lengths[b]-1], final_score[b] (or NULL)
 *   its value.  The backtrace runs in the chain's own workgroup.
 *   workspace >= hmm355_viterbi_ragged_workspace_bytes(B,T,N,obs_mode): psi (B,T,NP) uint8,
 *   NP = N padded to 64/128/256.
 * hmm355_forward_backward_ragged_f32: the scaled recursion with a deferred normaliser (a step
 *   stores its raw row, the next step divides by that row's sum):
 *     U_0 = exp(log_p0) e_0;                      U_{t+1} = (A^T U_t) e_{t+1} / CA_t,  CA_t = sum_i U_t[i]
 *     V_{len-1} = 1 or exp(log_beta_T - its max);  V_{t-1} = A (e_t V_t) / CB_t,   CB_t = sum_j e_t[j] V_t[j]
 *   e_t as in hmm355_forward_backward_ex_f32 (x + 1e-8, or exp(x - M_t)); the log-scales LA / LB
 *   are summed in fp64 after the chains.  loglik[b] = log sum_j alpha_{len-1}[j]; lik_ref[b] the
 *   reference's saturating value at frame len - 1.  log_beta_T (B,N) or NULL applies at frame
 *   lengths[b] - 1.  out_mask takes the three HMM355_FB_POSTERIOR / _FORWARD / _BACKWARD bits only.
 *   workspace >= hmm355_fb_workspace_bytes(B,T,N), in the layout hmm355_fb_workspace_layout
 *   reports: U | V (B,T,NP), LA | LB, .., M, CA | CB (B,T) with alpha_t = U_t exp(LA_t), beta_t =
 *   V_t exp(LB_t), so hmm355_fb_adjoint_f32 and its callers read the same pieces at the same
 *   offsets.  In frames t >= lengths[b]: U = V = 0, LA = LB = 0, CA = CB = 1; also CA = 1 at
 *   lengths[b] - 1 and CB = 1 at frame 0 (no step divides by them).
 * Status: HMM355_E_ARG for a null pointer (lengths included), a bad obs_mode, an unknown mask bit
 * or a mask bit without its pointer; HMM355_E_STATES for N outside [1, 256]; HMM355_E_SHAPE for
 * T < 1 or a size that overflows; HMM355_E_WORKSPACE for a short workspace; B == 0 is a no-op.
 * Every check comes before any launch.  The size query returns 0 for a rejected shape or mode.
 * ------------------------------------------------------------------------------ */
size_t hmm355_viterbi_ragged_workspace_bytes(int B, int T, int N, int obs_mode);
int hmm355_viterbi_ragged_f32(const float* obs, int obs_mode, const float* log_P, const float* init,
                              const int* lengths, int B, int T, int N, int64_t* states,
                              float* log_delta, float* final_score, void* workspace,
                              size_t workspace_bytes, void* stream);
int hmm355_forward_backward_ragged_f32(const float* obs, int obs_mode, const float* log_P,
                                       const float* log_p0, const float* log_beta_T /* (B,N) or NULL */,
                                       const int* lengths, int B, int T, int N, unsigned out_mask,
                                       float* posterior, float* forward, float* backward,
                                       float* loglik, float* lik_ref, void* workspace,
                                       size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Posterior path sampling (csrc/ffbs.hip), 1 <= N <= 256: the backward-sampling pass of
 * forward-filter backward-sample.  Draws K state paths per sequence from p(z | x), given the scaled
 * forward rows a forward-backward call leaves in its workspace and uniform numbers from the caller
 * (no random number generation in the kernel).
 *   fwd       (B,T) rows of ld floats, ld >= N: row (b,t) is proportional to alpha_t of sequence b
 *             (non-negative entries, any positive scale: the kernel forms the total itself).
 *             Columns N .. ld-1 are never read.  The U piece of hmm355_fb_workspace_layout with
 *             ld = NP (N padded to 64/128/256) is the intended input; keep it by calling
 *             hmm355_forward_backward_plan_f32 without the HMM355_FB_PAIR / _PLAN_BANDED hints, or
 *             hmm355_forward_backward_ragged_f32.
 *   log_P     (N,N); A = exp(log_P) in fp32
 *   lengths   (B) int32 or NULL (every sequence has T frames); clamped to [1, T] as read
 *   uniforms  (B,K,T) numbers in [0, 1)
 *   states    (B,K,T) int64 out
 * With L = lengths[b], for each (b,k) and t = L-1 down to 0:
 *   w[i]  = fwd[b,t,i] at t = L-1, else fwd[b,t,i] * A[i][z_{t+1}]
 *   C[i]  = the inclusive prefix sum of w in ascending i (fp32, any association),
 *           total = C[N-1], r = uniforms[b,k,t] * total
 *   z_t   = the smallest i with C[i] > r; if there is none (u * total rounded up to total) the
 *           largest i with w[i] > 0.  The chosen state always has w[z_t] > 0: a search that lands
 *           on a zero weight (a tree-shaped scan is not exactly monotone from lane to lane) moves
 *           to the nearest positive-weight index at or below it, else the nearest above it.
 *   A total that is not positive and finite: z_t = the first index maximising fwd[b,t,.] (state 0
 *   for a row of zeros).  Every state of a valid frame lies in [0, N-1].
 *   Frames t >= L get state -1; their fwd rows and uniforms are never read.
 * One wave per (b,k) chain; each launch is complete on its own (no waits between workgroups, no
 * atomics): the same inputs give the same states.
 * workspace >= hmm355_ffbs_workspace_bytes(N): exp(log_P)^T (NP,NP), built once per call.
 * Status: HMM355_E_STATES for N outside [1, 256] (the size query returns 0); HMM355_E_SHAPE for
 * T < 1, K < 1 or a size that overflows; HMM355_E_ARG for ld < N, a null pointer (lengths
 * excepted) or B < 0; HMM355_E_WORKSPACE for a short workspace; B == 0 is a no-op.  Every check
 * comes before any launch.
 * ------------------------------------------------------------------------------ */
size_t hmm355_ffbs_workspace_bytes(int N);
int hmm355_ffbs_f32(const float* fwd, int ld, const float* log_P, const int* lengths /* (B) or NULL */,
                    const float* uniforms /* (B,K,T) */, int B, int T, int N, int K,
                    int64_t* states /* (B,K,T) */, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * N-best (list) Viterbi (csrc/nbest.hip), 1 <= N <= 256, 1 <= K <= 16: the K most probable state
 * paths of every sequence, in order, with their scores.  All arithmetic is fp32.
 *   lo_t[j]   the log-emission: obs itself (HMM355_OBS_LOG) or the correctly rounded log(x + 1e-8)
 *             (HMM355_OBS_PROB), the bits hmm355_viterbi_f32 uses
 *   len       lengths[b] (clamped to [1, T] as read), or T with lengths == NULL
 *   d_0[j][0] = init[j] + lo_0[j];  d_0[j][k] = -inf for k >= 1 (empty slots)
 *   t >= 1:   the N*K candidates c(i, r) = fl(d_{t-1}[i][r] + log_P[i][j]) of state j are ordered by
 *             value descending, ties by i ascending, then r ascending (all -inf candidates tie);
 *             the k-th in that order gives d_t[j][k] = fl(c + lo_t[j]) and the back-pointer (i, r)
 *   end:      the N*K values d_{len-1}[j][k] ordered the same way (value, then j, then k); the
 *             first K are ranks 0 .. K-1, each path read back through the pointers
 * fp32 addition is monotone, so scores[b, :] are exactly the K largest values over all N^len paths
 * of the left-folded score fl(fl(s + log_P[z_{t-1}][z_t]) + lo_t[z_t]); the paths behind finite
 * scores are pairwise distinct.  Rank 0 follows the rule of hmm355_viterbi_f32 (first index on
 * ties, index 0 in a column without a finite candidate, first argmax at the last frame): its path
 * and score are the states and final_score of hmm355_viterbi_f32 / hmm355_viterbi_ragged_f32.
 *   paths   (B,K,T) int64;  scores (B,K) fp32, non-increasing in k
 *   count   (B) int32 or NULL: the number of ranks with a score above -inf
 * Rank 0 is always reported, even with score -inf.  Ranks k >= max(count, 1) do not exist (fewer
 * than K paths with a score above -inf, or N^len < K): score -inf, states -1.  Frames
 * t >= lengths[b] are never read (they may hold NaN) and get state -1.
 * One workgroup per sequence runs exactly len steps, its final selection and the K backtraces:
 * one launch, no waits between workgroups, no atomics; the same inputs give the same bits.
 * workspace >= hmm355_viterbi_nbest_workspace_bytes: the back-pointers, (B,T,K,NP) uint16 with
 * NP = N padded to 64/128/256, a pointer being 16 i + r.  That is B*T*K*NP*2 bytes: large, but
 * linear in every size (B = 32, T = 2000, N = 256, K = 16: 500 MiB).
 * Status, all before any launch: HMM355_E_ARG for a null pointer (lengths and count excepted),
 * a bad obs_mode or B < 0; HMM355_E_STATES for N outside [1, 256] or K > 16; HMM355_E_SHAPE for
 * T < 1, K < 1 or a size that overflows; HMM355_E_WORKSPACE for a short workspace; B == 0 is a
 * no-op.  The size query returns 0 for a rejected shape.
 * ------------------------------------------------------------------------------ */
size_t hmm355_viterbi_nbest_workspace_bytes(int B, int T, int N, int K, int obs_mode);
int hmm355_viterbi_nbest_f32(const float* obs, int obs_mode, const float* log_P, const float* init,
                             const int* lengths /* (B) int32 device, or NULL */, int B, int T, int N, int K,
                             int64_t* paths /* (B,K,T) */, float* scores /* (B,K) */, int* count /* (B) or NULL */,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * HMM recursions over an arc list: a sparse transition matrix (csrc/sparse.hip).
 * 1 <= N <= HMM355_SPARSE_MAX_STATES states, 1 <= E <= HMM355_SPARSE_MAX_ARCS arcs
 * (src[e], dst[e], log_w[e]) shared by the batch; self-loops and log_w = -inf are allowed, a
 * (src, dst) pair appears at most once (the caller's duty).  The model is exactly the dense one
 * whose log_P is -inf off the arcs.  log_obs (B,T,N) holds log-emissions (HMM355_OBS_LOG only);
 * lengths is (B) int32 on the device or NULL (= T everywhere), clamped to [1, T] as read; frames
 * t >= lengths[b] are never read (they may hold NaN).  The cost of a step is proportional to E.
 *
 * The arcs come sorted, grouped by an owner state, as a row-pointer array and two arc arrays:
 *   in_*   by destination, source ascending within a destination: state j owns the arcs
 *          in_ptr[j] .. in_ptr[j+1]-1, in_src[k] is the arc's source, in_log_w[k] its weight
 *   out_*  by source: state i owns out_ptr[i] .. out_ptr[i+1]-1, out_dst[k], out_log_w[k]
 * A row-pointer array is passed twice with the same N+1 values: *_ptr_host in host memory, checked
 * before any launch (non-decreasing from 0 to E, else HMM355_E_ARG; its largest difference selects
 * the kernel: up to 4 arcs per state, 3 above 4096 states, stay in registers for the whole
 * sequence, more are read through L2 every step, and a state with more than 64 is taken by a
 * whole wave), and *_ptr in
 * device memory, read by the kernels.  As read on the device a row pointer is clamped into [0, E]
 * and a state id into [0, N), so a wrong device array cannot index out of bounds.
 *
 * One workgroup per (sequence, job) -- the Viterbi chain with its backtrace, the alpha chain, the
 * beta chain -- running exactly lengths[b] steps with the state rows in LDS; one launch for the
 * chains, no waits between workgroups, no atomics: the same inputs give the same bits.
 *
 * hmm355_sparse_viterbi_f32: all fp32,
 *   delta_0 = init + e_0;  delta_t[j] = fl(max over in-arcs of fl(delta_{t-1}[src] + log_w) + e_t[j])
 * candidates in ascending source with strict >; a destination whose maximum is -inf (no in-arcs,
 * or every candidate -inf) gets delta = -inf and back-pointer 0; the final state is the first
 * argmax of delta_{len-1}.  states (B,T) int64, log_delta (B,T,N), final_score (B) or NULL are
 * bit-identical to hmm355_viterbi_f32 / _ragged_f32 / _wide_f32 on the densified matrix.  Padded
 * frames: state -1, log_delta -inf.  workspace: the back-pointers, (B,T,N rounded up to 8) uint16.
 *
 * hmm355_sparse_forward_backward_f32: the scaled probability-domain recursion with a deferred
 * normaliser (as hmm355_forward_backward_ragged_f32), e_t = exp(log_obs_t - max_j log_obs_t), the
 * log-scales summed in fp64 after the chains.  loglik (B); posterior (B,T,N) or NULL: gamma, 0 in
 * padded frames.  A sequence with no path of positive probability gets loglik -inf and exact
 * zeros in posterior.  The workspace keeps the scaled rows U, V (B,T,N fp32 each), the step
 * normalisers and two per-frame factors for hmm355_sparse_arc_counts_f32.
 *
 * hmm355_sparse_arc_counts_f32, after a forward-backward call with the same log_obs, lengths and
 * sizes, whose workspace is fb_workspace:
 *   xi[e] = sum_b weight[b] sum_{1 <= t < lengths[b]} P(z_{t-1} = src[e], z_t = dst[e] | x_b)
 * (weight (B) fp32 or NULL = 1), in the order of the src / dst / log_w arrays given (any order).
 * xi is (E) fp64: a thread per arc, per-tile partial sums in fp64 added in tile order, no atomics.
 * An arc with log_w = -inf and every arc of a sequence with no path count exactly 0.
 *
 * Status, every check before any launch: HMM355_E_ARG for B < 0, a null pointer (lengths,
 * final_score, posterior and weight excepted) or a bad row-pointer array; HMM355_E_STATES for N
 * outside [1, 8192]; HMM355_E_SHAPE for E outside [1, 2^20], T < 1 or a size that overflows;
 * HMM355_E_WORKSPACE for a short workspace; B == 0 is a no-op.  The size queries return 0 for a
 * rejected shape.
 * ------------------------------------------------------------------------------ */
#define HMM355_SPARSE_MAX_STATES 8192
#define HMM355_SPARSE_MAX_ARCS 1048576 /* 2^20 */
size_t hmm355_sparse_viterbi_workspace_bytes(int B, int T, int N, int E);
int hmm355_sparse_viterbi_f32(const float* log_obs, const int* in_ptr_host /* (N+1) host */,
                              const int* in_ptr /* (N+1) device */, const int* in_src /* (E) */,
                              const float* in_log_w /* (E) */, const float* init /* (N) */,
                              const int* lengths /* (B) int32 device, or NULL */, int B, int T, int N, int E,
                              int64_t* states /* (B,T) */, float* log_delta /* (B,T,N) */,
                              float* final_score /* (B) or NULL */, void* workspace, size_t workspace_bytes,
                              void* stream);
size_t hmm355_sparse_forward_backward_workspace_bytes(int B, int T, int N, int E);
int hmm355_sparse_forward_backward_f32(const float* log_obs, const int* in_ptr_host, const int* in_ptr,
                                       const int* in_src, const float* in_log_w, const int* out_ptr_host,
                                       const int* out_ptr, const int* out_dst, const float* out_log_w,
                                       const float* log_p0 /* (N) */, const int* lengths, int B, int T, int N, int E,
                                       float* loglik /* (B) */, float* posterior /* (B,T,N) or NULL */,
                                       void* workspace, size_t workspace_bytes, void* stream);
size_t hmm355_sparse_arc_counts_workspace_bytes(int B, int T, int N, int E);
int hmm355_sparse_arc_counts_f32(const float* log_obs, const int* src /* (E) device */, const int* dst /* (E) */,
                                 const float* log_w /* (E) */, const float* weight /* (B) or NULL */,
                                 const int* lengths, int B, int T, int N, int E, const void* fb_workspace,
                                 size_t fb_workspace_bytes, double* xi /* (E) */, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Diagonal-covariance Gaussian-mixture emission scorer.  Replaces
 * MixtureGaussianHMMLayer.get_observation_log_probs for covariance_type='diag'
 * (mixture_gaussian.py:157-214, LSE of :141-155) and, with C == 1 and log_w == 0,
 * GaussianHMMLayer._compute_gaussian_log_probs 'diag'/'full' (hmm_layer.py:300-321) and
 * HSMMLayer.get_observation_log_probs (hsmm.py:181-206).
 *   x (B,T,D); means, log_vars (S,C,D); log_w (S,C) = log(clamp(softmax(w),1e-8));
 *   out (B,T,S) = LSE_c[ -0.5*(sum_d (x-mu)^2/exp(lv) + sum_d lv + D*log(2pi)) + log_w ].
 * `mix_lse` selects the reference's mixture LSE (clamped sum, :141-155); with C == 1 pass 0
 * to get the plain component log-density.  Supported: 1 <= D <= 8192, 1 <= C <= 256,
 * 1 <= S*C <= 65536, B*T < 2^31.  workspace >= hmm355_gmm_workspace_bytes(B,T,D,S,C)
 * (per-component scales and an fp64 copy of the frames; written by the call).  The
 * quadratic form is accumulated in fp64 and each score rounded to fp32 once, so the scores
 * are as close to the exact value as the reference's fp32 ones (its Viterbi paths decode
 * identically at BASELINE config 3).
 * ------------------------------------------------------------------------------ */
size_t hmm355_gmm_workspace_bytes(int B, int T, int D, int S, int C);
int hmm355_gmm_diag_logprob_f32(const float* x, const float* means, const float* log_vars,
                                const float* log_w, int B, int T, int D, int S, int C,
                                int mix_lse, float* out, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Occupancy-weighted sufficient statistics of the diagonal Gaussian (mixture) emissions
 * (csrc/emstats.hip): the emission half of the Baum-Welch E-step (pytorch_hmm_amd/em.py).  The
 * reference has no counterpart (it trains by autograd only).
 *   x (B,T,D); weight (B,T,S), any sign (EM passes the state posteriors); means, log_vars (S,C,D);
 *   log_w (S,C) or NULL for 0; lengths (B) int32 or NULL (every sequence has T frames).
 * With comp[b,t,s,c] the scorer's component score above (-0.5*(...) + log_w) and r the softmax of
 * comp over c, shifted by its maximum (r = 0 for every c of a state whose components are all -inf;
 * r = 1 when mix_lse == 0, which requires C == 1), and w[b,t,s,c] = weight[b,t,s] * r[b,t,s,c]:
 *   occ (S,C)   = sum_{b, t < lengths[b]} w
 *   sx  (S,C,D) = sum w * (x - mu)
 *   sxx (S,C,D) = sum w * (x - mu)^2
 * all fp32; any of the three may be NULL and is then skipped.  The moments are centred on the
 * means passed in: mu' = mu + sx/occ and var' = sxx/occ - (sx/occ)^2 have none of the cancellation
 * of raw second moments.  A component with log_w = -inf gets exactly 0 in all three outputs.
 * Frames at t >= lengths[b] are never read, in x or in weight (their values are selected out, not
 * multiplied by a mask).  Precision: the quadratic form, the products and the sums are fp64; the
 * exponentials of the softmax are fp32 (expf/logf), each workgroup's partial sum is rounded to fp32
 * once and the partial sums are added in index order in fp64: the error of an output is a few
 * 2^-24 of the sum of its terms' magnitudes, and the result is bitwise the same on every call and
 * stream (no atomics).
 * Supported: 1 <= D <= HMM355_GMM_STATS_MAX_DIM (else HMM355_E_SHAPE), 1 <= C <= 256 and
 * 1 <= S*C <= 65536 (else HMM355_E_STATES), T >= 1 and B*T < 2^31 (else HMM355_E_SHAPE).
 * HMM355_E_ARG for a negative size, a null x / weight / means / log_vars / workspace, or
 * mix_lse == 0 with C > 1; HMM355_E_WORKSPACE for a short workspace; B == 0 is a no-op.  Every
 * check comes before any launch; the size query returns 0 for an unsupported shape.
 * workspace >= hmm355_gmm_stats_workspace_bytes(B,T,D,S,C): three fp64 (D,S*C) parameter tables
 * and one (2D+1, S*C) fp32 partial sum per frame span (at most 512 spans); nothing proportional to
 * frames * S*C.
 * ------------------------------------------------------------------------------ */
#define HMM355_GMM_STATS_MAX_DIM 1024
size_t hmm355_gmm_stats_workspace_bytes(int B, int T, int D, int S, int C);
int hmm355_gmm_stats_f32(const float* x, const float* weight, const float* means, const float* log_vars,
                         const float* log_w /* or NULL */, const int* lengths /* (B) or NULL */, int B, int T,
                         int D, int S, int C, int mix_lse, float* occ /* (S,C) or NULL */,
                         float* sx /* (S,C,D) or NULL */, float* sxx /* (S,C,D) or NULL */, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * HSMM segment Viterbi.  Replaces HSMMLayer.viterbi_decode_hsmm / _viterbi_decode_single
 * (hsmm.py:208-354), reproducing its candidate order (s' outer, d' inner, strict >), its
 * fp32 addition order ((prev + logT) + obs_sum) + dur and torch-CPU's summation order for
 * obs_sum, so paths are bit-identical given identical fp32 inputs.
 *   lp (B,T,S) obs log-probs; dur_lp (S,Dmax) = log(p_dur + 1e-8); log_T (S,S)
 *   states (B,T) int64; scores (B) fp32
 *   1 <= S <= 1024 (HMM355_E_STATES beyond), 1 <= Dmax <= 1024 (HMM355_E_DURATION beyond).
 *   obs_sum follows ATen's cascade_sum order (csrc/tsum.h; it changes from 72 frames on).
 *   S = 1: the slice is contiguous and takes torch's vectorised order; the path is all 0.
 *   Frames the walk never reaches (no predecessor path: every score -inf) are written 0,
 *   the reference's torch.zeros initial value.
 *   S <= 64 with Dmax <= 71, or S <= 128 with Dmax <= 63: one workgroup per sequence keeps
 *   every open segment in registers and the tables in LDS (csrc/hsmm.hip); larger sizes take
 *   the general form (csrc/hsmm_wide.hip: M history and segment sums in the workspace,
 *   B*T*S*(Dmax+1) floats).
 * ------------------------------------------------------------------------------ */
size_t hmm355_hsmm_workspace_bytes(int B, int T, int S, int Dmax);
int hmm355_hsmm_viterbi_f32(const float* lp, const float* dur_lp, const float* log_T, int B,
                            int T, int S, int Dmax, int64_t* states, float* scores,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Kernel-form flags of the segment recursions (results are identical in every form; parity
 * tests compare them):
 *   HMM355_FORM_GENERAL      the general form (workspace tables) whatever the size
 *   HMM355_FORM_SERIAL_WALK  HSMM only: the serial backtrace walk instead of the chunked one
 * The _ex workspace queries take the same flags. */
#define HMM355_FORM_GENERAL 0x1u
#define HMM355_FORM_SERIAL_WALK 0x2u
size_t hmm355_hsmm_workspace_bytes_ex(int B, int T, int S, int Dmax, unsigned flags);
int hmm355_hsmm_viterbi_ex_f32(const float* lp, const float* dur_lp, const float* log_T, int B,
                               int T, int S, int Dmax, unsigned flags, int64_t* states,
                               float* scores, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * HSMM forward-backward (csrc/hsmm_fb.hip): the sum over the segmentations that
 * hmm355_hsmm_viterbi_f32 maximises over.  Log-likelihood, state posteriors and the expected
 * counts, each the derivative of loglik with respect to the matching input.  The reference has
 * no such routine (HSMMLayer can only decode, hsmm.py:208-354).
 *   lp (B,T,S) frame log-scores; dur_lp (S,Dmax), column d-1 scores duration d; log_T (S,S);
 *   log_init (S) or NULL = all zeros (what the decoder uses).  -inf entries are allowed, +inf
 *   and NaN are not.
 * A segmentation (s_1,d_1)..(s_K,d_K) has sum d_k = T exactly (the last segment ends at frame
 * T-1: no censoring), 1 <= d_k <= Dmax and s_k != s_k+1: log_T's diagonal is never used.  Its
 * score is sum_k dur_lp[s_k,d_k-1] + (lp over its frames) + (k = 1 ? log_init[s_1] :
 * log_T[s_k-1,s_k]).  With O(a..t,s) the sum of lp[.,s] over frames a..t:
 *   begin_0(s) = log_init(s);  F_t(s) = LSE_{d <= min(Dmax,t+1)} begin_t-d+1(s) + O(t-d+1..t,s)
 *   + dur_lp[s,d-1];  begin_t+1(s) = LSE_{s' != s} F_t(s') + log_T[s',s];
 *   Bend_T-1(s) = 0;  Bend_t(s) = LSE_{s' != s} log_T[s,s'] + Bbeg_t+1(s');
 *   Bbeg_t(s) = LSE_{d <= min(Dmax,T-t)} dur_lp[s,d-1] + O(t..t+d-1,s) + Bend_t+d-1(s).
 * Every LSE takes its own maximum (exact whatever the spread of its candidates); -inf candidates
 * drop out and a cell without a finite candidate is -inf.  The recursions run on lp[t,.] minus
 * its row maximum (0 for a row without a finite one), which every segmentation pays once per
 * frame; the sum of the maxima is carried in fp64 and added to loglik.
 *   loglik (B)             = LSE_s F_T-1(s).  Always produced.
 *   gamma (B,T,S)          = P(state at frame t is s) = sum_{a<=t} P(segment of s begins at a) -
 *                            sum_{e<t} P(segment of s ends at e), an fp64 running sum, with
 *                            P(begin) = exp(begin + Bbeg - loglik), P(end) = exp(F + Bend - loglik)
 *   dur_counts (B,S,Dmax)  = expected number of (s,d) segments
 *   trans_counts (B,S,S)   = expected number of i -> j transitions (zero diagonal)
 *   init_post (B,S)        = exp(log_init + Bbeg_0 - loglik)
 * sum dur_counts = sum trans_counts + 1.  A sequence without a segmentation has loglik = -inf
 * and every posterior and count 0; no NaN is written and its neighbours are unaffected.  No
 * floating-point atomics: two calls on the same inputs return the same bits.
 *   flags  HMM355_HSMM_FB_GAMMA / _DUR / _TRANS / _INIT select the optional outputs (their
 *          pointers may be NULL otherwise).  With none of them only the forward sum runs and no
 *          (B,T,S) table is written.  HMM355_FORM_GENERAL is accepted (there is one form).
 *   workspace >= hmm355_hsmm_fb_workspace_bytes(B,T,S,Dmax,flags), 16-byte aligned: log_T in both
 *          orientations, the row maxima, and with any output flag begin | F | Bend | Bbeg (B,T,S)
 *          fp32 of the shifted scores; with _DUR fp64 prefix sums of the shifted scores and
 *          -inf counts (B,T,S); with _DUR / _TRANS the partial sums of the counts.
 * 1 <= S <= HMM355_HSMM_FB_MAX_STATES (else HMM355_E_STATES); 1 <= Dmax <=
 * HMM355_HSMM_FB_MAX_DURATION and S * Dmax <= HMM355_HSMM_FB_MAX_CELLS (else HMM355_E_DURATION:
 * a sequence's open segments live in 64 KiB of one workgroup's LDS); T >= 1, 0 <= B <=
 * HMM355_HSMM_FB_MAX_BATCH (a sequence is a grid row) and B * T <= 2^31 (else HMM355_E_SHAPE: call
 * in batch slices); B == 0 is a no-op.  The size query returns 0 for a rejected shape or
 * flag.  Every check comes before any launch.
 * ------------------------------------------------------------------------------ */
#define HMM355_HSMM_FB_GAMMA 0x10u
#define HMM355_HSMM_FB_DUR 0x20u
#define HMM355_HSMM_FB_TRANS 0x40u
#define HMM355_HSMM_FB_INIT 0x80u
#define HMM355_HSMM_FB_MAX_STATES 256
#define HMM355_HSMM_FB_MAX_DURATION 128
#define HMM355_HSMM_FB_MAX_CELLS 16384
#define HMM355_HSMM_FB_MAX_BATCH 65535
size_t hmm355_hsmm_fb_workspace_bytes(int B, int T, int S, int Dmax, unsigned flags);
int hmm355_hsmm_fb_f32(const float* lp, const float* dur_lp, const float* log_T,
                       const float* log_init /* (S) or NULL */, int B, int T, int S, int Dmax,
                       unsigned flags, float* loglik, float* gamma /* (B,T,S) or NULL */,
                       float* dur_counts /* (B,S,Dmax) or NULL */,
                       float* trans_counts /* (B,S,S) or NULL */, float* init_post /* (B,S) or NULL */,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Recursions with one transition matrix per time step (NeuralHMM).  Replace
 * NeuralHMM._forward_algorithm / _backward_algorithm and the posterior epilogue of
 * NeuralHMM.forward (neural.py:391-461) and NeuralHMM.viterbi_decode (neural.py:463-511).
 *   log_obs (B,T,N): log-emissions (the observation network's output, any finite values);
 *   log_A: log transition matrices, element (b,k,i,j) at
 *          log_A[b*a_bstride + k*a_tstride + i*N + j] (strides in elements; pass 0, 0 for one
 *          (N,N) matrix shared by every step: neural.py:383-385).  Forward and Viterbi step t
 *          use matrix k = t-1 (neural.py:419-427, :489-496), backward step t matrix k = t
 *          (neural.py:449-458); matrix T-1 is never read.  Entries must be <= ~88 (exp range);
 *          -inf is allowed.
 *   log_p0 / init (N): log initial probabilities (neural.py:388-389, :478-479).
 * FB outputs as hmm355_forward_backward_f32 (posterior = exp(log_post), forward =
 * exp(log_forward), backward = exp(log_backward), loglik = LSE(log_forward[T-1]), lik_ref =
 * the reference's compute_likelihood LSE(log(forward[T-1] + 1e-8)), neural.py:513-519).
 * Viterbi: states (B,T) int64, log_delta (B,T,N) fp32 (bit-identical to the reference's
 * fp32 sums; first index on ties).  1 <= N <= 256.
 * Workspaces >= hmm355_tv_fb_workspace_bytes / hmm355_tv_viterbi_workspace_bytes(B,T,N).
 * ------------------------------------------------------------------------------ */
size_t hmm355_tv_fb_workspace_bytes(int B, int T, int N);
int hmm355_tv_forward_backward_f32(const float* log_obs, const float* log_A, long long a_bstride,
                                   long long a_tstride, const float* log_p0, int B, int T, int N,
                                   unsigned out_mask, float* posterior, float* forward,
                                   float* backward, float* loglik, float* lik_ref,
                                   void* workspace, size_t workspace_bytes, void* stream);
/* As hmm355_tv_forward_backward_f32 with an optional terminal backward vector log_beta_T
 * (B,N) (NULL = 0, the reference's beta_{T-1}); used by the adjoint (see
 * hmm355_forward_backward_ex_f32).  Workspace layout: U | V (B,T,NP) | LA | LB (B,T) |
 * E (B,T,NP) = exp(log_obs - M) | M (B,T) | CA | CB (B,T) | ..., pieces 256-B aligned,
 * NP = 64/128/256; log alpha = log U + LA, log beta = log V + LB. */
int hmm355_tv_forward_backward_ex_f32(const float* log_obs, const float* log_A, long long a_bstride,
                                      long long a_tstride, const float* log_p0,
                                      const float* log_beta_T, int B, int T, int N,
                                      unsigned out_mask, float* posterior, float* forward,
                                      float* backward, float* loglik, float* lik_ref,
                                      void* workspace, size_t workspace_bytes, void* stream);
/* Adjoint of the time-varying forward-backward outputs (NeuralHMM training through its
 * posteriors, neural.py:355-461): hmm355_fb_adjoint_f32's two chains with matrix k
 * (exp(log_A[b,k]), linking steps k and k+1, strides as above) in place of one log_P.  E, the
 * sources and W / P are (B,T,N) with row stride N; scale_w / scale_z (B,T). */
int hmm355_tv_fb_adjoint_f32(const float* E, const float* log_A, long long a_bstride,
                             long long a_tstride, const float* src_w, const float* scale_w,
                             const float* src_z, const float* scale_z, int B, int T, int N,
                             float* W, float* P, void* stream);
size_t hmm355_tv_viterbi_workspace_bytes(int B, int T, int N);
int hmm355_tv_viterbi_f32(const float* log_obs, const float* log_A, long long a_bstride,
                          long long a_tstride, const float* init, int B, int T, int N,
                          int64_t* states, float* log_delta, void* workspace,
                          size_t workspace_bytes, void* stream);
/* ---------------------------------------------------------------------------------
 * Explicit-duration (semi-Markov) HMM, indexed by segment END time.  Replace
 * SemiMarkovHMM.viterbi_decode (semi_markov.py:455-570), the segment observation score
 * SemiMarkovHMM._compute_segment_observation_logprob (semi_markov.py:411-435) and the
 * segment forward SemiMarkovHMM._unsupervised_forward (semi_markov.py:308-383, whose
 * intended logaddexp recursion this computes; the reference raises TypeError there).
 *
 * hmm355_semimarkov_quad_f32: per-frame Mahalanobis term
 *   quad[b,t,s] = sum_k ((x[b,t,k] - mu[s,k])^2) / var[s,k]   (k ascending, fp32)
 *   x (B,T,Df); means_t, vars_t are (Df,S) (transposed); var = exp(logvar) formed by the
 *   caller with the reference's torch op (semi_markov.py:418).
 * hmm355_semimarkov_viterbi_f32 / _forward_f32: the segment recursions over
 *   quad (B,T,S); seg_const (S) or NULL.  Segment score of frames [st, t] in state s:
 *     seg_const != NULL (gaussian): seg_const[s] - 0.5 * Q   (the reference adds the
 *        constant -0.5*sum(logvar) - 0.5*D*log(2 pi) once per SEGMENT, :420-424)
 *     seg_const == NULL (additive, observation_model='neural'): Q
 *   with Q = quad[st] + quad[st+1] + ... + quad[t] (left to right).
 *   log_init (S) = log(softmax(initial_logits) + 1e-8); log_T (S,S) = log(softmax(
 *   transition_logits) + 1e-8) (self-transitions are excluded by the recursion);
 *   dur_lp (S,Dmax) = DurationModel log-probabilities for d = 1..Dmax.
 * Viterbi outputs: segments right-aligned in (B,T) int64 seg_states / seg_durs, the last
 *   seg_count[b] entries of row b in time order, the T - seg_count[b] entries in front of them
 *   seg_states = -1 and seg_durs = 0; scores (B) = best final delta.  Candidate
 *   order (s' outer, d' inner, strict >) and fp32 addition order ((prev + logT) then
 *   (best + obs) + dur) are the reference's, so segmentations are bit-identical given
 *   identical fp32 quad/table inputs.
 * Forward outputs: log_prob (B) = LSE over (s,d) of log alpha[T-1]; log_alpha (B,T,S,Dmax)
 *   optional (NULL = not written), -inf where a segment is impossible.
 * 1 <= S <= 1024, 1 <= Dmax <= 1024.  S <= 64 with Dmax <= 63 runs the register form; larger
 * sizes the general form (its workspace holds a (B,T,S,Dmax) fp32 segment-score table:
 * hmm355_semimarkov_workspace_bytes).
 * ------------------------------------------------------------------------------ */
size_t hmm355_semimarkov_workspace_bytes(int B, int T, int S, int Dmax);
int hmm355_semimarkov_quad_f32(const float* x, const float* means_t, const float* vars_t, int B,
                               int T, int Df, int S, float* quad, void* stream);
int hmm355_semimarkov_viterbi_f32(const float* quad, const float* seg_const,
                                  const float* log_init, const float* log_T,
                                  const float* dur_lp, int B, int T, int S, int Dmax,
                                  int64_t* seg_states, int64_t* seg_durs, int* seg_count,
                                  float* scores, void* workspace, size_t workspace_bytes,
                                  void* stream);
int hmm355_semimarkov_forward_f32(const float* quad, const float* seg_const,
                                  const float* log_init, const float* log_T,
                                  const float* dur_lp, int B, int T, int S, int Dmax,
                                  float* log_alpha, float* log_prob, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* The same with kernel-form flags (HMM355_FORM_GENERAL). */
size_t hmm355_semimarkov_workspace_bytes_ex(int B, int T, int S, int Dmax, unsigned flags);
int hmm355_semimarkov_viterbi_ex_f32(const float* quad, const float* seg_const,
                                     const float* log_init, const float* log_T,
                                     const float* dur_lp, int B, int T, int S, int Dmax,
                                     unsigned flags, int64_t* seg_states, int64_t* seg_durs,
                                     int* seg_count, float* scores, void* workspace,
                                     size_t workspace_bytes, void* stream);
int hmm355_semimarkov_forward_ex_f32(const float* quad, const float* seg_const,
                                     const float* log_init, const float* log_T,
                                     const float* dur_lp, int B, int T, int S, int Dmax,
                                     unsigned flags, float* log_alpha, float* log_prob,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Streaming decoders of StreamingHMMProcessor, one chunk of B independent streams.
 *   emis (B,T,N): the emission network's log-probabilities; log_T (N,N) =
 *   log(softmax(transition_logits) + 1e-8).  1 <= N <= 256 (log_T LDS-resident up to 128; above
 *   that its rows are read from global memory per step).
 * hmm355_stream_greedy_f32 replaces _greedy_decode (streaming.py:267-320):
 *   s_t = argmax_j (log_T[s_{t-1}][j] + emis[t][j]), first index on ties; the chain starts
 *   from prev_state[b], or, when prev_state[b] < 0 (the stream's first chunk), from
 *   emis[0][j] - log_n with log_n = log(N) in fp32.  states (B,T) int64, scores (B,T) the
 *   chosen step scores (the reference returns exp(scores)).
 * hmm355_stream_beam_f32 replaces _beam_search_decode (streaming.py:322-377):
 *   hyp_score / hyp_last (B,32) and hyp_count (B) (<= 32) hold each stream's hypotheses in
 *   rank order and are updated in place (a stream may carry more hypotheses than the new K,
 *   after its beam width was lowered, streaming.py:459-461); first[b] != 0 applies the empty-path rule of the stream's first
 *   frame (score + emis, no transition).  Each step keeps the K best of the hyp_count * N
 *   expansions by score descending, ties by expansion index h*N + j ascending (Python's
 *   stable sort), score = (score_h + log_T[last_h][j]) + emis[t][j] in fp32.
 *   parent / hstate (B,T,K) int16: new hypothesis r at step t came from hypothesis
 *   parent[t][r] of step t-1 and entered state hstate[t][r]; while the beam is under-full (a step
 *   has kn = min(K, live * N) < K hypotheses) the ranks r >= kn get parent = hstate = -1.
 *   states (B,T) int64: the best
 *   hypothesis' last T states.  1 <= K <= 32 and live_max (<= 32) bounds every hyp_count[b];
 *   for N > 128, K and live_max <= 16 (else HMM355_E_ARG).
 * ------------------------------------------------------------------------------ */
int hmm355_stream_greedy_f32(const float* emis, const float* log_T, const int* prev_state,
                             float log_n, int B, int T, int N, int64_t* states, float* scores,
                             void* stream);
int hmm355_stream_beam_f32(const float* emis, const float* log_T, int B, int T, int N, int K,
                           int live_max, float* hyp_score, int* hyp_last, int* hyp_count, const int* first,
                           int16_t* parent, int16_t* hstate, int64_t* states, void* stream);

/* ---------------------------------------------------------------------------------
 * Dynamic time warping over a distance matrix (csrc/dtw.hip).  Replace compute_dtw_path
 * (alignment/dtw.py:61-152), the soft-DTW loop of DTWAligner._soft_dtw_align (dtw.py:277-299) and
 * the autograd through it.  One workgroup per pair, one launch per call.
 *   dist   (B,N,M) fp32 row-major distance matrices; +inf entries are allowed (a band), NaN is not
 *   n_len, m_len  (B) int32 or NULL: pair b uses the top-left n_len[b] x m_len[b] corner
 *          (NULL = N / M; values are clamped to [1, N] / [1, M])
 * Any N, M >= 1, B >= 0 (B == 0 launches nothing); N < 1 or M < 1 or a size that overflows
 * returns HMM355_E_SHAPE and the size query 0.
 *
 * hmm355_dtw_f32: hard DTW.  C[0,0] = D[0,0]; predecessors that do not exist are left out.
 *   HMM355_DTW_SYMMETRIC / _ASYMMETRIC  C[i,j] = D[i,j] + min(C[i-1,j-1], C[i-1,j], C[i,j-1])
 *          (the reference's asymmetric min(c + d) has the same bits: the fp32 add is monotone)
 *   HMM355_DTW_RABINER_JUANG            C[i,j] = min(C[i-1,j-1] + 2 D[i,j], C[i-1,j] + D[i,j],
 *                                                    C[i,j-1] + D[i,j])
 *   The cost matrix is bit-identical to the reference's.  Any other pattern: HMM355_E_ARG.
 *   flags  HMM355_DTW_PATH: also backtrace from (n-1, m-1) to (0,0), at each step to the
 *          predecessor of smallest raw cost, ties in the order (i-1,j-1), (i-1,j), (i,j-1)
 *          (dtw.py:127-143).  path_i / path_j / path_len must then be given.
 *   cost_matrix (B,N,M) or NULL; cells outside a pair's corner are +inf.  With NULL and no path
 *          only `total` is produced and no N x M table is written.
 *   total  (B): C[n-1, m-1] (+inf when the end cell is unreachable)
 *   path_i, path_j (B, N+M-1) int32 in path order from index 0, -1 past the end; path_len (B)
 *   workspace >= hmm355_dtw_workspace_bytes(B, N, M, flags), 16-byte aligned: a row buffer
 *          (B, 4 ceil(M/4)) fp32 | with HMM355_DTW_PATH the directions, one byte per row and four
 *          columns (B, N, ceil(M/4)) | the walk end-to-start, 2 x (B, N+M-1) int32.
 *
 * hmm355_softdtw_f32: R (B,N+1,M+1) with R[0,0] = 0, the rest of row 0 and column 0 +inf,
 *   R[i,j] = D[i-1,j-1] + softmin_gamma(R[i-1,j-1], R[i-1,j], R[i,j-1]),
 *   softmin_gamma(c) = m - gamma log sum exp(-(c - m) / gamma), m = min c (+inf when m is);
 *   total (B) = R[n,m]; entries of R outside a pair's corner are +inf.  gamma must be > 0 and
 *   finite (HMM355_E_ARG).
 * hmm355_softdtw_grad_f32: E (B,N,M) = d total / d dist from the R hmm355_softdtw_f32 stored
 *   (Cuturi & Blondel 2017, Algorithm 2, its factors evaluated as the softmin's weights, which R
 *   alone determines; dist must be given and is not read); 0 outside a pair's corner and on
 *   cells R marks unreachable.
 * ------------------------------------------------------------------------------ */
#define HMM355_DTW_SYMMETRIC 0
#define HMM355_DTW_ASYMMETRIC 1
#define HMM355_DTW_RABINER_JUANG 2
#define HMM355_DTW_PATH 0x1u
size_t hmm355_dtw_workspace_bytes(int B, int N, int M, unsigned flags);
int hmm355_dtw_f32(const float* dist, const int* n_len, const int* m_len, int B, int N, int M,
                   int pattern, unsigned flags, float* cost_matrix, float* total, int* path_i,
                   int* path_j, int* path_len, void* workspace, size_t workspace_bytes,
                   void* stream);
int hmm355_softdtw_f32(const float* dist, const int* n_len, const int* m_len, int B, int N, int M,
                       float gamma, float* R, float* total, void* stream);
int hmm355_softdtw_grad_f32(const float* dist, const float* R, const int* n_len, const int* m_len,
                            int B, int N, int M, float gamma, float* E, void* stream);

/* ---------------------------------------------------------------------------------
 * CTC lattice (csrc/ctc.hip).  Replace the per-cell loops of ctc_forward_algorithm
 * (alignment/ctc.py:32-121) and ctc_backward_algorithm (:124-199), and give ctc_alignment_path
 * (:202-256) the alpha it never fills.  One launch per call, one workgroup per sequence and job
 * (forward sum, backward sum, Viterbi).
 *   log_probs (T,B,C) fp32 row-major; -inf entries are allowed, +inf and NaN are not
 *   targets   (B,Lmax) int32; only the first target_lengths[b] of row b are read.  A label
 *             outside [0, C) is never used as an index: its emission counts as -inf
 *   input_lengths, target_lengths  (B) int32 device arrays.  The caller guarantees
 *             1 <= input_lengths[b] <= T and 0 <= target_lengths[b] <= Lmax (the Python layer
 *             checks them on the host); the kernels clamp what they read to those ranges
 *   blank     in [0, C)
 * Sequence b has S'_b = 2 target_lengths[b] + 1 positions, ext[s] = blank (s even) or
 * targets[b, s / 2] (s odd); tables are (B,T,S') with S' = 2 Lmax + 1.
 * T, B, C >= 1 (else HMM355_E_ARG); 1 <= Lmax <= HMM355_CTC_MAX_TARGET (else HMM355_E_STATES); a
 * size that overflows returns HMM355_E_SHAPE; the size query returns 0 for any of them.
 *
 * hmm355_ctc_f32
 *   loglik (B): LSE(alpha[T_b-1, S'_b-1], alpha[T_b-1, S'_b-2]) (the first alone when the target
 *          is empty); -inf for a pair with no alignment.  Always produced.
 *   flags  HMM355_CTC_ALPHA: store alpha (B,T,S'): alpha[0,0] = lp[0,b,blank], alpha[0,1] =
 *            lp[0,b,ext[1]], then alpha[t,s] = lp[t,b,ext[s]] + LSE(alpha[t-1,s], alpha[t-1,s-1],
 *            alpha[t-1,s-2] if ext[s] != ext[s-2]); frames >= input_lengths[b] and positions
 *            >= S'_b are -inf.  Without it no (B,T,S') table is written for the forward sum.
 *          HMM355_CTC_BETA: store beta (B,T,S') in the reference's convention, which leaves the
 *            frame's own emission out: beta[T_b-1, S'_b-1] = beta[T_b-1, S'_b-2] = 0,
 *            beta[t,s] = LSE over s' in {s, s+1, s+2 if ext[s] != ext[s+2]} of
 *            beta[t+1,s'] + lp[t+1,b,ext[s']]; the same -inf fill.
 *          HMM355_CTC_VITERBI: the best single path.  path (B,T) int32: the expanded position of
 *            each frame, -1 for frames >= input_lengths[b] and in every frame of a pair with no
 *            alignment; score (B): its log-probability (-inf then).  Ties go to the first of
 *            s, s-1, s-2; the path ends in S'_b-1 unless S'_b-2 scores strictly higher.
 *   workspace >= hmm355_ctc_workspace_bytes(B, T, Lmax, flags), 16-byte aligned (with
 *          HMM355_CTC_VITERBI the 2-bit choices of every cell; 256 bytes otherwise).
 * hmm355_ctc_grad_f32: from the alpha, beta and loglik of one hmm355_ctc_f32 call,
 *   gamma (B,T,S') or NULL: exp(alpha + beta - loglik), 0 where either is -inf;
 *   grad (T,B,C) = d loglik / d log_probs: grad[t,b,c] = sum of gamma[b,t,s] over ext[s] = c.
 *   Both are 0 in frames >= input_lengths[b] and for a pair with no alignment.  No atomics: two
 *   calls on the same inputs return the same bits.
 * ------------------------------------------------------------------------------ */
#define HMM355_CTC_ALPHA 0x1u
#define HMM355_CTC_BETA 0x2u
#define HMM355_CTC_VITERBI 0x4u
#define HMM355_CTC_MAX_TARGET 2048
size_t hmm355_ctc_workspace_bytes(int B, int T, int Lmax, unsigned flags);
int hmm355_ctc_f32(const float* log_probs, const int* targets, const int* input_lengths,
                   const int* target_lengths, int T, int B, int C, int Lmax, int blank,
                   unsigned flags, float* alpha, float* beta, float* loglik, int* path,
                   float* score, void* workspace, size_t workspace_bytes, void* stream);
int hmm355_ctc_grad_f32(const float* alpha, const float* beta, const float* loglik,
                        const int* targets, const int* input_lengths, const int* target_lengths,
                        int T, int B, int C, int Lmax, int blank, float* gamma, float* grad,
                        void* stream);

/* ---------------------------------------------------------------------------------
 * Duration-constrained Viterbi (csrc/dchmm.hip).  Replaces the t / s / prev_s loops of
 * DurationConstrainedHMM._constrained_viterbi (hsmm.py:520-590): a Viterbi recursion with a
 * run-length counter per cell and soft penalties that depend on the counters.  One launch per
 * call, one workgroup per penalty group; no workgroup waits on another.
 *   emis   (B,T,S) fp32 emission log-probs, log_T (S,S) fp32 log-transitions; -inf entries are
 *          allowed, +inf and NaN are not.  log_T's diagonal is never read.
 *   group  G in [1, B]: sequences [k G, min(B, (k+1) G)) share their penalties.  G = B is the
 *          reference (it takes .max() / .min() over the whole batch, so the sequences of a
 *          batch are coupled); G = 1 decodes every sequence as the reference would alone.
 * Per cell (b,s) and time t: delta (fp32), psi, dur (ints).  Every fl() is one fp32 rounding.
 *   t = 0   delta = fl(e[b,0,s] - fl32(log S)), dur = 1.
 *   t >= 1  over the group's previous row:  dmax1[s] = max_b dur[b,t-1,s] + 1,
 *           dmin[s] = min_b dur[b,t-1,s];
 *           pen_self[s] = fl(fl32(-w) * fl32(dmax1[s] - max_duration))  if dmax1[s] > max_duration
 *           pen_from[p] = fl(fl32(-w) * fl32(min_duration - dmin[p]))   if dmin[p] < min_duration
 *           (an absent penalty is not added); candidates in ascending p:
 *             p == s: fl(fl(delta[b,t-1,s] + e[b,t,s]) + pen_self[s]),         dur' = dur[b,t-1,s] + 1
 *             p != s: fl(fl(fl(delta[b,t-1,p] + log_T[p,s]) + e[b,t,s]) + pen_from[p]),  dur' = 1
 *           a candidate wins only if strictly greater than the best so far, which starts at
 *           -inf: the first index wins a tie, and a cell whose candidates are all -inf keeps
 *           delta = -inf, psi = 0, dur = 0 (that 0 enters the next step's dmin).
 *   end     states[b,T-1] = the first argmax of delta[b,T-1,:], final_score[b] its value;
 *           states[b,t] = psi[b,t+1,states[b,t+1]].
 *   log_delta, durations  (B,T,S) or NULL: the whole trellis, written only when given.
 *   workspace >= hmm355_dchmm_workspace_bytes(B, T, S), 16-byte aligned: psi, one byte per cell.
 * Limits: 1 <= S <= HMM355_DCHMM_MAX_STATES and group * S <= HMM355_DCHMM_MAX_CELLS (else
 * HMM355_E_STATES: the rows of a group live in one workgroup's LDS), T >= 1 (else
 * HMM355_E_SHAPE), B >= 1 and 1 <= group <= B (else HMM355_E_ARG); the size query returns 0 for
 * a rejected B, T or S.  Every check comes before any launch.
 * ------------------------------------------------------------------------------ */
#define HMM355_DCHMM_MAX_STATES 256
#define HMM355_DCHMM_MAX_CELLS 4096
size_t hmm355_dchmm_workspace_bytes(int B, int T, int S);
int hmm355_dchmm_viterbi_f32(const float* emis, const float* log_T, int B, int T, int S, int group,
                             int min_duration, int max_duration, float penalty_weight,
                             int64_t* states, float* final_score,
                             float* log_delta /* (B,T,S) or NULL */, int32_t* durations /* (B,T,S) or NULL */,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Transcript forced alignment (csrc/forced.hip): every sequence has its own left-to-right chain
 * of S_b positions (the states of its transcript, in order); a position stays, advances by one
 * or skips one; a path starts in position 0 and ends in position S_b - 1.  One launch per call,
 * one workgroup per sequence and job (forward sum, backward sum, Viterbi).
 *   log_probs (B,T,C) fp32 row-major, batch first; -inf entries are allowed, +inf and NaN are not
 *   state_ids (B,Smax) int32: the class (column of log_probs) of each position; only the first
 *             state_lengths[b] of row b are read.  An id outside [0, C) is never used as an
 *             index: its emission counts as -inf.  NULL: id_s = s (log_probs is already
 *             (B,T,S): monotonic alignment search); needs C >= Smax, else HMM355_E_ARG
 *   input_lengths, state_lengths  (B) int32 device arrays.  The caller guarantees
 *             1 <= input_lengths[b] <= T and 1 <= state_lengths[b] <= Smax (the Python layer
 *             checks them on the host); the kernels clamp what they read to those ranges
 *   log_stay, log_next, log_skip  (B,Smax) fp32 or NULL: the weights of s -> s, s -> s + 1 and
 *             s -> s + 2, indexed by the source position; -inf entries are allowed.  NULL means
 *             0, 0 and -inf (no skips).  With all three and state_ids NULL the step has no
 *             weight adds and reads its emissions as consecutive floats.
 * With e[t,s] = log_probs[b,t,id_s]; tables are (B,T,Smax):
 *   alpha[0,0] = e[0,0], alpha[0,s>0] = -inf,
 *   alpha[t,s] = e[t,s] + LSE(alpha[t-1,s] + stay[s], alpha[t-1,s-1] + next[s-1],
 *                             alpha[t-1,s-2] + skip[s-2]);
 *   beta[T_b-1,S_b-1] = 0, beta[t,s] = LSE(stay[s] + e[t+1,s] + beta[t+1,s],
 *                next[s] + e[t+1,s+1] + beta[t+1,s+1], skip[s] + e[t+1,s+2] + beta[t+1,s+2])
 *   (beta leaves its own frame's emission out, as the CTC tables do).  -inf candidates drop out
 *   of the LSE; frames >= input_lengths[b] and positions >= S_b are -inf.
 * T, B, C >= 1 (else HMM355_E_ARG); 1 <= Smax <= HMM355_FORCED_MAX_POSITIONS (else
 * HMM355_E_STATES); a size that overflows returns HMM355_E_SHAPE; the size query returns 0 for any
 * of them.  Every check comes before any launch.
 *
 * hmm355_forced_f32
 *   loglik (B): alpha[T_b-1, S_b-1]; -inf for a pair with no path (S_b > T_b without skips,
 *          for example).  Always produced.
 *   flags  HMM355_FORCED_ALPHA: store alpha.  Without it the forward sum writes no table.
 *          HMM355_FORCED_BETA: store beta.
 *          HMM355_FORCED_VITERBI: the best single path, max in place of LSE; candidates in the
 *            order stay, s-1, s-2 with strict >, so the first wins a tie; each candidate is one
 *            fp32 add of value and weight, the cell one more add of the emission.  path (B,T)
 *            int32: the position of each frame, -1 for frames >= input_lengths[b] and in every
 *            frame of a pair with no path; score (B): alpha's max-plus counterpart at
 *            [T_b-1, S_b-1] (-inf then); durations (B,Smax) int32: the frames the path spends
 *            in each position, 0 for a skipped position, one >= S_b and a pair with no path.
 *   workspace >= hmm355_forced_workspace_bytes(B, T, Smax, flags), 16-byte aligned (with
 *          HMM355_FORCED_VITERBI the 2-bit choices of every cell; 256 bytes otherwise).
 * hmm355_forced_grad_f32: from the alpha, beta and loglik of one hmm355_forced_f32 call and the
 *   same ids, lengths and weights (log_probs itself is not read again: alpha holds its
 *   emissions), any of (at least one)
 *   gamma (B,T,Smax): exp(alpha + beta - loglik), 0 where either is -inf.  Every such exponent
 *     is normalised by its frame's own LSE over s of alpha + beta - loglik (0 in exact
 *     arithmetic), which cancels the rounding that the frame's fp32 alpha and beta share;
 *   grad_log_probs (B,T,C) = d loglik / d log_probs: the sum of gamma[b,t,s] over id_s = c;
 *   grad_stay, grad_next, grad_skip (B,Smax) = d loglik / d log_stay, ...:
 *     grad_stay[b,s] = sum over 1 <= t < T_b of exp(alpha[t-1,s] + stay[s] + e[t,s] + beta[t,s]
 *     - loglik), grad_next / grad_skip with e and beta at s + 1 / s + 2 (a NULL weight array
 *     counts as its default).  Each term is formed as gamma of the target position times the
 *     transition's share among the candidates into it, which is the same number.
 *   All are 0 in frames >= input_lengths[b], positions >= S_b and for a pair with no path.  For
 *   a pair with a path every frame of grad_log_probs sums to 1 and the three transition
 *   gradients together to T_b - 1.  No atomics: two calls on the same inputs return the same bits.
 *   workspace: needed for the transition gradients only (else it may be NULL):
 *     >= hmm355_forced_workspace_bytes(B, T, Smax, HMM355_FORCED_GRAD), 16-byte aligned (the sums
 *     of every tile of frames, added in tile order by a second launch); HMM355_FORCED_GRAD is a
 *     flag of the size query alone (together with the others it returns the larger need), and
 *     hmm355_forced_f32 rejects it.
 * ------------------------------------------------------------------------------ */
#define HMM355_FORCED_ALPHA 0x1u
#define HMM355_FORCED_BETA 0x2u
#define HMM355_FORCED_VITERBI 0x4u
#define HMM355_FORCED_GRAD 0x8u
#define HMM355_FORCED_MAX_POSITIONS 4096
size_t hmm355_forced_workspace_bytes(int B, int T, int Smax, unsigned flags);
int hmm355_forced_f32(const float* log_probs, const int* state_ids, const int* input_lengths,
                      const int* state_lengths, const float* log_stay, const float* log_next,
                      const float* log_skip, int B, int T, int C, int Smax, unsigned flags,
                      float* alpha, float* beta, float* loglik, int* path, float* score,
                      int* durations, void* workspace, size_t workspace_bytes, void* stream);
int hmm355_forced_grad_f32(const float* alpha, const float* beta, const float* loglik,
                           const int* state_ids, const int* input_lengths,
                           const int* state_lengths, const float* log_stay, const float* log_next,
                           const float* log_skip, int B, int T, int C, int Smax, float* gamma,
                           float* grad_log_probs, float* grad_stay, float* grad_next,
                           float* grad_skip, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---------------------------------------------------------------------------------
 * Explicit-duration forced alignment (csrc/durforced.hip): the transcript chain of the forced
 * alignment above with the duration model of the HSMM in the place of stay / next weights.
 * Sequence b has T_b = input_lengths[b] frames and L_b = state_lengths[b] positions; every position
 * is visited once, in order (no skips), for d_l frames, 1 <= d_l <= Dmax, sum d_l = T_b exactly.
 * One launch per call for the chains, one workgroup per sequence and job (forward sum, backward
 * sum, max-plus forward with its walk).
 *   log_probs (B,T,C) fp32 row-major, batch first; -inf entries are allowed, +inf and NaN are not
 *   state_ids (B,Lmax) int32: the class (column of log_probs) of each position; only the first
 *             state_lengths[b] of row b are read.  An id outside [0, C) is never used as an
 *             index: its emission counts as -inf.  NULL: id_l = l (log_probs is already
 *             (B,T,Lmax)); needs C >= Lmax, else HMM355_E_ARG
 *   input_lengths, state_lengths  (B) int32 device arrays.  The caller guarantees
 *             1 <= input_lengths[b] <= T and 1 <= state_lengths[b] <= Lmax (the Python layer
 *             checks them on the host); the kernels clamp what they read to those ranges
 *   dur_lp    (B,Lmax,Dmax) fp32: dur_lp[b,l,d-1] scores a segment of d frames for position l;
 *             -inf forbids that duration (a minimum duration is a run of leading -inf)
 * A segmentation scores sum_l dur_lp[b,l,d_l-1] + sum_t log_probs[b,t,id(position of t)].  With
 * O(a..t,l) the sum of position l's emissions over frames a..t, tables (B,T,Lmax):
 *   begin_0(0) = 0, begin_0(l>0) = -inf, begin_t(0) = -inf for t > 0
 *   F_t(l)     = OP_{d <= min(Dmax,t+1)} begin_{t-d+1}(l) + O(t-d+1..t,l) + dur_lp[l,d-1]
 *   begin_t+1(l+1) = F_t(l);   result = F_{T_b-1}(L_b-1)
 *   Bend_{T_b-1}(L_b-1) = 0;  Bend_t(l) = Bbeg_t+1(l+1)
 *   Bbeg_t(l)  = LSE_d dur_lp[l,d-1] + O(t..t+d-1,l) + Bend_{t+d-1}(l)
 * OP is log-sum-exp for loglik and max for the best segmentation.  -inf candidates drop out of an
 * LSE; no NaN is formed.  The recursions run on log_probs[b,t,id_l] - M_t, M_t the maximum over
 * the chain's positions at frame t (0 where none is finite): every segmentation covers every frame
 * once, so all scores move by sum_t M_t, which loglik and score get back in fp64.  The stored
 * tables are those of the shifted scores; frames >= T_b and positions >= L_b are -inf.
 * A pair is infeasible when T_b < L_b, T_b > L_b * Dmax or the -inf entries leave no
 * segmentation: loglik / score -inf, path -1 everywhere, durations 0, gamma and gradients 0.
 * T, B, C >= 1 (else HMM355_E_ARG); 1 <= Lmax <= HMM355_DURFORCED_MAX_POSITIONS, 1 <= Dmax <=
 * HMM355_DURFORCED_MAX_DURATION and Lmax * Dmax <= HMM355_DURFORCED_MAX_CELLS (else
 * HMM355_E_STATES: a sequence's open segments and its dur_lp live in one workgroup's LDS); B * T
 * <= 2^31 and sizes that do not overflow (else HMM355_E_SHAPE); the size query returns 0 for any
 * of them.  Every check comes before any launch.
 *
 * hmm355_durforced_f32
 *   loglik (B): the log of the sum over segmentations; always produced.
 *   flags  HMM355_DURFORCED_TABLES: run the backward sum too and store begin, F, Bend, Bbeg
 *            (B,T,Lmax), frame_shift (B,T) = M_t (0 past T_b) and loglik_shifted (B) = loglik
 *            without sum_t M_t: what hmm355_durforced_grad_f32 takes.  Without it no table is
 *            written and those six pointers may be NULL.
 *          HMM355_DURFORCED_VITERBI: the best segmentation.  Candidates are taken in ascending d
 *            with strict >, so the smaller d wins a tie; the walk starts at position L_b - 1,
 *            frame T_b - 1.  durations (B,Lmax) int32: d_l, 0 for l >= L_b; path (B,T) int32: the
 *            position of every frame, -1 for frames >= T_b; score (B).
 *   workspace >= hmm355_durforced_workspace_bytes(B, T, Lmax, Dmax, flags), 16-byte aligned (every
 *          job's M_t; with HMM355_DURFORCED_VITERBI one byte per cell, the chosen d - 1).
 * hmm355_durforced_grad_f32: from the tables of one hmm355_durforced_f32 call and the same
 *   log_probs, ids, lengths and dur_lp, any of (at least one)
 *   gamma (B,T,Lmax): the posterior of position l at frame t, the running sum over t of
 *     P(l begins at t) - P(l ended at t - 1) = exp(begin + Bbeg - loglik_shifted) - exp(F + Bend -
 *     loglik_shifted), exponents and sum in fp64;
 *   grad_log_probs (B,T,C) = d loglik / d log_probs: the sum of gamma[b,t,l] over id_l = c;
 *   grad_dur_lp (B,Lmax,Dmax) = d loglik / d dur_lp: grad_dur_lp[b,l,d-1] = sum_t exp(begin_{t-d+1}(l)
 *     + O(t-d+1..t,l) + dur_lp[b,l,d-1] + Bend_t(l) - loglik_shifted), the expected number of
 *     "position l lasts d frames"; O comes from fp64 prefix sums of the shifted emissions and a
 *     running count of -inf frames.
 *   For a feasible pair every used frame's gamma and every used position's grad_dur_lp row sum
 *   to 1.  Three launches (gamma and prefix sums; counts per time chunk; the chunks added in
 *   chunk order and the classes' gammas in position order); no atomics: two calls on the same
 *   inputs return the same bits.
 *   workspace: needed for grad_dur_lp, and for grad_log_probs without gamma (else it may be NULL):
 *     >= hmm355_durforced_workspace_bytes(B, T, Lmax, Dmax, HMM355_DURFORCED_GRAD), 16-byte
 *     aligned; HMM355_DURFORCED_GRAD is a flag of the size query alone (together with the others
 *     it returns the larger need), and hmm355_durforced_f32 rejects it.
 * ------------------------------------------------------------------------------ */
#define HMM355_DURFORCED_TABLES 0x1u
#define HMM355_DURFORCED_VITERBI 0x2u
#define HMM355_DURFORCED_GRAD 0x4u
#define HMM355_DURFORCED_MAX_POSITIONS 1024
#define HMM355_DURFORCED_MAX_DURATION 128
#define HMM355_DURFORCED_MAX_CELLS 16384
size_t hmm355_durforced_workspace_bytes(int B, int T, int Lmax, int Dmax, unsigned flags);
int hmm355_durforced_f32(const float* log_probs, const int* state_ids, const int* input_lengths,
                         const int* state_lengths, const float* dur_lp, int B, int T, int C,
                         int Lmax, int Dmax, unsigned flags, float* begin, float* F, float* Bend,
                         float* Bbeg, float* frame_shift, float* loglik_shifted, float* loglik,
                         int* path, float* score, int* durations, void* workspace,
                         size_t workspace_bytes, void* stream);
int hmm355_durforced_grad_f32(const float* begin, const float* F, const float* Bend,
                              const float* Bbeg, const float* frame_shift,
                              const float* loglik_shifted, const float* log_probs,
                              const int* state_ids, const int* input_lengths,
                              const int* state_lengths, const float* dur_lp, int B, int T, int C,
                              int Lmax, int Dmax, float* gamma, float* grad_log_probs,
                              float* grad_dur_lp, void* workspace, size_t workspace_bytes,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HMM355_H */
