// hmm355 — the serial recursion shared by forward-backward and Viterbi (gfx950).
//
// One workgroup runs one chain (a sequence's forward pass, backward pass, or Viterbi
// max-plus pass) over T steps.  The chain is latency-bound (T dependent steps of an
// NP x NP reduction), so the layout minimises the per-step critical path and the LDS
// instruction count:
//
//   * NW = NP/16 waves; wave w owns outputs o = 16w + c (c = lane & 15); the lane's row
//     r = lane >> 4 owns the inputs i = 64*blk + 16r + n.  Its matrix slice lives in VGPRs.
//   * The previous vector is held one value per lane (input 64*blk + lane), so DPP
//     row_newbcast folded into v_fmac_f32_dpp / v_add_f32_dpp feeds every product from a
//     register: the inner loop has no LDS traffic.
//   * The four row groups' partial results for each output are halved in-register by one
//     v_permlane32_swap (rows {0,2} and {1,3}); lanes 0..31 write the two halves as a
//     float2 per output (conflict-free ds_write_b32).  After the step's single s_barrier
//     every lane reads each of its inputs' float2 with one conflict-free ds_read_b64 (the
//     LDS cycles per step, not only the latency, bound the exchange: 8 waves x NBLK x 2).
//   * Forward-backward runs in the probability domain with Rabiner scaling: the scale of
//     step q is 1/c_{q-1} (c = sum of the previous vector, a DPP wave sum beside the FMAs)
//     and is folded, with the emission, into the partials before they are written.
//     Viterbi adds the log-emission to each partial max (fl(max + lo) == max(fl(x + lo)),
//     so the result is still the bit-exact delta).  log-scales accumulate at flush time.
//   * Emissions are staged 16 steps at a time through a 3-slot LDS ring (global loads issued
//     two blocks ahead); finished rows sit in a 64-row LDS ring and leave as 16-B stores once
//     per 16 steps.  The loop body issues no per-step global memory operation.
//   * The workgroup requests all 160 KiB of LDS so it owns its CU (no co-resident
//     workgroup of a concurrent kernel steals issue slots from the chain).
#pragma once
#include "band.h"
#include "common.h"
#include "logcr.h"
#include "post.h"

namespace hmm355 {

enum RecKind : int { kFbAlpha = 0, kFbBeta = 1, kVit = 2 };
typedef unsigned int u32x2_t __attribute__((__vector_size__(2 * sizeof(unsigned int))));  // (as fbpair.h)

// How many steps ahead the banded chain wave (band_chain) reads a step's staged emission row
// inside an unrolled 16-step block, by chain: 1 or 2.  Two for beta and Viterbi, whose reduction
// is filled (wave_red_fill): the wait for a row read two steps ahead stands in gap emis_wait_gap
// of the step in between, in the place of a wait state, and the step loses the issue slot the
// s_waitcnt took ahead of the row's first use.  alpha leaves its placing to the compiler and
// measured slower at two.  The macros are for diagnostic builds.
#ifndef HMM355_EMIS_AHEAD_ALPHA
#define HMM355_EMIS_AHEAD_ALPHA 1
#endif
#ifndef HMM355_EMIS_AHEAD_BETA
#define HMM355_EMIS_AHEAD_BETA 2
#endif
#ifndef HMM355_EMIS_AHEAD_VIT
#define HMM355_EMIS_AHEAD_VIT 2
#endif
// the gap of the filled reduction (wave_red_fill) that holds the wait for a row read two steps
// ahead (emis_wait_gap below): in form 0 gap 4, ahead of row_bcast:15; in the forms with fewer
// gaps the one ahead of row_bcast:31.  The register windows of up to two states a lane (NP <= 128)
// leave it empty (fill_cnt); where the step's own units fill it the wait costs there what it
// saved.  HMM355_EMIS_WAIT_GAP: diagnostic builds, the gap by number.
constexpr int emis_ahead(int kind) {
  return kind == kFbAlpha ? HMM355_EMIS_AHEAD_ALPHA : kind == kFbBeta ? HMM355_EMIS_AHEAD_BETA : HMM355_EMIS_AHEAD_VIT;
}
// The form of the step's wave reduction (wave_red_level) by chain: what measured faster per chain
// (DESIGN section 14 round 11): beta and Viterbi both triples, alpha, whose reduction is not
// filled, the first one.  HMM355_RED_FORM (common.h) sets all three, for diagnostic builds.
#ifdef HMM355_RED_FORM
#define HMM355_RED_FORM_ALPHA HMM355_RED_FORM
#define HMM355_RED_FORM_BETA HMM355_RED_FORM
#define HMM355_RED_FORM_VIT HMM355_RED_FORM
#endif
#ifndef HMM355_RED_FORM_ALPHA
#define HMM355_RED_FORM_ALPHA 1
#endif
#ifndef HMM355_RED_FORM_BETA
#define HMM355_RED_FORM_BETA 3
#endif
#ifndef HMM355_RED_FORM_VIT
#define HMM355_RED_FORM_VIT 3
#endif
constexpr int red_form(int kind) {
  return kind == kFbAlpha ? HMM355_RED_FORM_ALPHA : kind == kFbBeta ? HMM355_RED_FORM_BETA : HMM355_RED_FORM_VIT;
}

// diagnostic builds (HMM355_STAMP=1): per wave [gather, compute, write-wait, barrier, steps,
// total cycles, memtime, memrealtime] summed over the steps (tools/stamps.py)
constexpr int kStampWaves = 512 * 16;
static __device__ unsigned long long g_rec_stamps[kStamp ? kStampWaves * 8 : 1];
// HMM355_STAMP=2: also the staging helpers' block work by item and the psi waves (rec_band); these
// stamps wait for the wave's LDS reads, so the chain's own figures are taken from a STAMP=1 build
constexpr bool kStampItems = HMM355_STAMP > 1;
#ifndef HMM355_STAMP_BAR
#define HMM355_STAMP_BAR 1
#endif
constexpr bool kStampBar = HMM355_STAMP_BAR;  // (band_chain: stamps round the block barrier)

template <int NP>
struct RC {
  static constexpr int NW = NP / 16;     // waves
  static constexpr int NT = NW * kWave;  // threads
  static constexpr int NBLK = NP / 64;   // 64-input blocks per lane
  static constexpr int RING = 64;        // stored-row ring
  static constexpr int OFF_PART = 0;                       // [2][NP][2] half-wave partials
  static constexpr int OFF_EMIS = OFF_PART + 2 * NP * 2;   // [3][16][NP]
  static constexpr int OFF_RING = OFF_EMIS + 3 * 16 * NP;  // [RING][NP]
  static constexpr int OFF_SC = OFF_RING + RING * NP;      // [RING][64] normalisers c_rho (entry 0;
                                                           // the banded chain writes all 64 lanes)
  static constexpr int OFF_M = OFF_SC + RING * 64;        // [128] OBS_LOG FB: staged row maxima (0 else)
  static constexpr int MRING = 128;                        // rows kb-3 .. kb+1 live at once
  static constexpr int OFF_LOGT = OFF_M + MRING;           // [256] doubles: Viterbi log table (logcr.h)
  static constexpr int LDS_FLOATS = OFF_LOGT + 512;
  static_assert(LDS_FLOATS * 4 <= kExclusiveLds, "LDS layout too large");
  // forward-backward end rows (rec_band): each staging helper's left-over blocks, [16] words
  static constexpr int OFF_LEFT = LDS_FLOATS;
  static_assert((OFF_LEFT + 16) * 4 <= kExclusiveLds, "end-row LDS layout too large");
  // fused-psi Viterbi (kVitFused; the chain kernel owns all 160 KiB): the psi rows of the last
  // 64 steps (bytes [64][NP]), written by the psi waves, copied to HBM by the staging helpers
  static constexpr int PSR = 64;
  static constexpr int OFF_PSR = LDS_FLOATS;
  static_assert((OFF_PSR + PSR * NP / 4) * 4 <= kExclusiveLds, "fused Viterbi LDS layout too large");
};

// threads of a launch that may run the register-blocked dense chain (rec_run_rb, NP <= 128):
// its NW chain waves plus NH block-work helper waves (rec_rb_helper)
template <int NP>
struct kRbHelpers {
  static constexpr int NH = NP <= 128 ? RC<NP>::NW / 2 : 0;
  static constexpr int NT = RC<NP>::NT + NH * kWave;
  static_assert(NH <= 8, "kProgSlots");
};
// the forward-backward chain kernel's threads: the dense chain's helpers included (the banded
// chains use the first RC<NP>::NT and the rest end at once, rec_dispatch)
template <int NP>
constexpr int kFbNT = kRbHelpers<NP>::NT;

// Level L (0..5) of the DPP reduction of a wave to lane 63: the four in-row levels (quad_perm x2,
// row_ror:4, row_ror:8: every lane of a row holds the row's value), then row_bcast:15 and
// row_bcast:31.  One v_add_f32_dpp / v_max_f32_dpp each, all of them the compiler's own
// instructions, so its hazard recognizer pads a level only when fewer than two instructions
// separate it from the write of its source (a DPP read of a VGPR a VALU just wrote: 2 wait
// states), and no opaque asm block stands between the levels and the work around them.
// The two row_bcast levels run with every row enabled and bound_ctrl: a row without a source
// row (row 0; rows 0, 1) combines with 0 and holds a value nobody reads.  The result is taken
// from lane 63 alone, and the lanes it descends from (lane 31 after row_bcast:15, lane 63)
// always have a source: ((r3 + r2) + (r1 + r0)), as with the row masks 0xa / 0xc.
//
// The forms F of the reduction (HMM355_RED_FORM, a set of the bits red::kA and red::kB; 0 is the
// six levels above).  The two wait states belong to the register a level reads THROUGH DPP; its
// other operand is forwarded like any VALU operand.  So a pair of dependent levels becomes three
// shifts of one settled register into a fresh accumulator, which wait once, for that register:
//   kA  t = op(x, x >> 1); t = op(t, x >> 2); t = op(t, x >> 3)     in the place of the quad_perms
//   kB  r = op(t, t >> 4); r = op(r, t >> 8); r = op(r, t >> 12)    in the place of the row_rors
// (row_shr with bound_ctrl).  Lane 15 of each row ends with the row's 16 values, all of them from
// inside the row; the lanes that shifted a 0 in are never among the sources of lane 15, and the
// row_bcast levels read lanes 15, 31, 47 and 63 only.  A sum associates (((x15 + x14) + x13) + x12)
// ... where form 0 has ((x0 + x1) + (x2 + x3)) ...; a maximum is the same bits in every form.
// The hazard recognizer pads a DPP instruction for ANY operand a VALU instruction of the
// compiler's wrote less than two slots ago, not only the shifted one, so the second and third
// shift of a triple are one asm statement, inside which nothing is padded.  The first shift is the
// compiler's own: it is padded for the triple's source by what the fillers ahead of it leave, and
// once it may read the source the two behind it may.  The compiler takes the statement's result
// for a VALU write, so it pads the level behind the triple as it pads any other.
namespace red {
constexpr int kA = 1, kB = 2;
// the stages (a level or a triple) of form F, and the form-0 level stage S stands in the place of
constexpr int stages(int F) { return 6 - (F & kA ? 1 : 0) - (F & kB ? 1 : 0); }
constexpr bool triple_at(int F, int L) { return (L == 0 && (F & kA)) || (L == 2 && (F & kB)); }
constexpr int level(int F, int S) {
  int L = 0;
  for (int s = 0; s < S; ++s) L += triple_at(F, L) ? 2 : 1;
  return L;
}
}  // namespace red
// op(acc, src >> SHR within the row), the compiler's instruction
template <bool MAX, int SHR>
__device__ __forceinline__ float red_shr(float acc, float src) {
  const float o = __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, src), 0x110 + SHR, 0xF, 0xF, true));
  return MAX ? fmaxf(acc, o) : acc + o;
}
// acc = op(op(acc, src >> S2), src >> S3), unpadded: src is settled, acc is no DPP source.
// PIN (wave_red_fill): a volatile statement, which keeps its place among the sched_barriers as
// fill_pin keeps a level's -- an empty asm behind this one would cost the one-state pad the
// compiler puts between an asm statement's result and its first reader.
#define HMM355_RED_SHR2(VOL, OP)                                                            \
  asm VOL(OP " %0, %1, %0 row_shr:%2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"           \
          OP " %0, %1, %0 row_shr:%3 row_mask:0xf bank_mask:0xf bound_ctrl:1"               \
          : "+v"(acc) : "v"(src), "n"(S2), "n"(S3))
template <bool MAX, int S2, int S3, bool PIN>
__device__ __forceinline__ float red_shr2_asm(float acc, float src) {
  if constexpr (MAX && PIN) HMM355_RED_SHR2(volatile, "v_max_f32_dpp");
  else if constexpr (MAX) HMM355_RED_SHR2(, "v_max_f32_dpp");
  else if constexpr (PIN) HMM355_RED_SHR2(volatile, "v_add_f32_dpp");
  else HMM355_RED_SHR2(, "v_add_f32_dpp");
  return acc;
}
#undef HMM355_RED_SHR2
// stage S of form F (form 0: level S)
template <bool MAX, int S, int F = 0, bool PIN = false>
__device__ __forceinline__ float wave_red_level(float x) {
  constexpr int L = red::level(F, S);
  if constexpr (red::triple_at(F, L)) {
    constexpr int K = L == 0 ? 1 : 4;
    return red_shr2_asm<MAX, 2 * K, 3 * K, PIN>(red_shr<MAX, K>(x, x), x);
  } else {
    constexpr int CTRL = L == 0 ? 0xB1 : L == 1 ? 0x4E : L == 2 ? 0x124 : L == 3 ? 0x128 : L == 4 ? 0x142 : 0x143;
    const float o = __builtin_bit_cast(
        float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, L >= 4));
    return MAX ? fmaxf(x, o) : x + o;
  }
}
__device__ __forceinline__ float wave_lane63(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}

// Sum / max over all 64 lanes with DPP only, read from lane 63: wave-uniform.
template <int F = 0>
__device__ __forceinline__ float wave_sum_bcast(float x) {
  static_for<0, red::stages(F)>([&](auto S) { x = wave_red_level<false, decltype(S)::value, F>(x); });
  return wave_lane63(x);
}
template <int F = 0>
__device__ __forceinline__ float wave_max_bcast(float x) {
  static_for<0, red::stages(F)>([&](auto S) { x = wave_red_level<true, decltype(S)::value, F>(x); });
  return wave_lane63(x);
}

// The same reductions with filler work: a lone wave issues in order, so each of the six
// dependent levels waits two issue slots for the one before it, v_readlane one for the last
// level, and the first VALU read of the SGPR two for v_readlane.  fill(integral_constant<G>)
// is called in gap G and issues instructions of the caller's that do not read the reduction:
// G = 0..5 ahead of level G, 6 ahead of v_readlane, 7 behind it (fill_slots slots each); in form
// F, ahead of each of its red::stages(F) stages (a triple waits once, ahead of its first shift:
// 9 instructions and 11 slots in form kA | kB against 7 and 15), then the same two.
// sched_barrier pins the fillers there: the scheduler does not model these hazards as latency
// and leaves the later levels back to back, padded with s_nop.  (The empty asm ties each level
// to its place among the barriers: the DPP intrinsics have no side effects, and instruction
// selection otherwise emits a level behind the next gap's fillers.)  A gap left short is padded
// by the compiler.  Same operations in the same order as the plain forms: identical bits.
constexpr int fill_gaps(int F) { return red::stages(F) + 2; }
constexpr int fill_slots(int F, int G) { return G == fill_gaps(F) - 2 ? 1 : 2; }
// the gap that holds the wait for the next step's emission row (band_chain, PW): form 0 ahead of
// row_bcast:15, else ahead of row_bcast:31, which a step with eight
// fillers still leaves empty where it fills the one ahead of row_bcast:15
constexpr int emis_wait_gap(int F) {
#ifdef HMM355_EMIS_WAIT_GAP
  return HMM355_EMIS_WAIT_GAP;
#else
  return F == 0 ? 4 : red::stages(F) - 1;
#endif
}
// The fillers of gap G when the caller has NU of them: whole gaps first, the gap behind
// v_readlane, then gaps 0, 1, 2 ... (a gap filled by half still costs its s_nop: of the
// allocations measured -- in proportion to the slots, from the back, from the front -- this one
// ran fastest); what exceeds all slots goes behind v_readlane too.
constexpr int fill_cnt(int G, int NU, int F = 0) {
  const int NG = fill_gaps(F);
  int rem = NU, all = 0;
  for (int i = 0; i < NG; ++i) all += fill_slots(F, i);
  for (int i = 0; i < NG; ++i) {
    const int g = i == 0 ? NG - 1 : i - 1;
    const int c = fill_slots(F, g) < rem ? fill_slots(F, g) : rem;
    if (g == G) return c + (G == NG - 1 && NU > all ? NU - all : 0);
    rem -= c;
  }
  return 0;
}
// fillers [fill_lo(G), fill_lo(G + 1)) go to gap G: in the caller's order
constexpr int fill_lo(int G, int NU, int F = 0) {
  int lo = 0;
  for (int g = 0; g < G; ++g) lo += fill_cnt(g, NU, F);
  return lo;
}
__device__ __forceinline__ void fill_pin(float& x) { asm volatile("" : "+v"(x)); }
template <bool MAX, int F = 0, typename FILL>
__device__ __forceinline__ float wave_red_fill(float x, FILL&& fill) {
  constexpr int NS = red::stages(F);
  static_for<0, NS>([&](auto S) {
    __builtin_amdgcn_sched_barrier(0);
    fill(S);
    __builtin_amdgcn_sched_barrier(0);
    x = wave_red_level<MAX, decltype(S)::value, F, true>(x);
    if constexpr (!red::triple_at(F, red::level(F, decltype(S)::value))) fill_pin(x);
  });
  __builtin_amdgcn_sched_barrier(0);
  fill(std::integral_constant<int, NS>{});
  __builtin_amdgcn_sched_barrier(0);
  x = wave_lane63(x);
  __builtin_amdgcn_sched_barrier(0);
  fill(std::integral_constant<int, NS + 1>{});
  __builtin_amdgcn_sched_barrier(0);
  return x;
}

#if HMM355_RED_PROBE
// diagnostic builds (tools/probe_wave_reduce.py): one wave per 64-lane vector of `in`;
// out[v][F] the maximum and out[v][4 + F] the sum of vector v by form F = 0 .. 3
static __global__ void red_probe_kernel(const float* in, float* out, int n) {
  const int v = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
  if (v >= n) return;
  const float x = in[(size_t)v * kWave + (threadIdx.x & (kWave - 1))];
  static_for<0, 4>([&](auto F) {
    const float m = wave_max_bcast<decltype(F)::value>(x), s = wave_sum_bcast<decltype(F)::value>(x);
    if ((threadIdx.x & (kWave - 1)) == 0) {
      out[(size_t)v * 8 + decltype(F)::value] = m;
      out[(size_t)v * 8 + 4 + decltype(F)::value] = s;
    }
  });
}
#endif

// The banded FB step sums NB products p_j * e_j (the input of the normaliser's reduction) that
// are also needed one by one.  Left to fp contraction (hipcc's default is fast) the backend
// fuses ONE product of the first pair into an fma with the other, and which one depends on the
// order the instructions reach it: any rescheduling of the step changed output bits.  So the
// form is written out, with contraction off:
//   prod_j = p_j * e_j for every j;  t = fma(p_a, e_a, prod_b);  t = fma(p_j, e_j, t), j = 2 ..
// FIRST: (a, b) = (0, 1), else (1, 0) -- per instantiation what the compiler had chosen before
// the form was pinned (band_chain: kSumFirst), so the bits stay what they were.
template <int NB>
__device__ __forceinline__ void prods(const float (&p)[NB], const float (&e)[NB], float (&prod)[NB]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < NB; ++j) prod[j] = p[j] * e[j];
}
template <int NB, bool FIRST>
__device__ __forceinline__ float prod_sum(const float (&p)[NB], const float (&e)[NB], const float (&prod)[NB]) {
#pragma clang fp contract(off)
  if constexpr (NB == 1) {
    return prod[0];
  } else {
    float t = FIRST ? fmaf(p[0], e[0], prod[1]) : fmaf(p[1], e[1], prod[0]);
#pragma unroll
    for (int j = 2; j < NB; ++j) t = fmaf(p[j], e[j], t);
    return t;
  }
}
// the same sum of finished values (no product in reach: across a loop's back edge)
template <int NB>
__device__ __forceinline__ float plain_sum(const float (&v)[NB]) {
#pragma clang fp contract(off)
  float t = v[0];
#pragma unroll
  for (int j = 1; j < NB; ++j) t = t + v[j];
  return t;
}

// v_writelane_b32: lane LANE of dst takes the (wave-uniform) value v; the lane is an inline
// constant (no s_mov: a single wave issues one instruction per issue cycle whatever its type).
template <int LANE>
__device__ __forceinline__ void writelane_c(float& dst, float v) {
  asm("v_writelane_b32 %0, %1, %2" : "+v"(dst) : "s"(v), "i"(LANE));
}

// ---- one-instruction shifted window terms (DPP on src0; a lane whose DPP source falls off
// the 64-lane wave is disabled and keeps the destination's previous value)
#define HMM355_DPP_OP(name, op, ctrl)                                                         \
  __device__ __forceinline__ void name(float& dst, float src, float w) {                      \
    asm("s_nop 1\n\t" op " %0, %1, %2 " ctrl " row_mask:0xf bank_mask:0xf" : "+v"(dst) : "v"(src), "v"(w)); \
  }
HMM355_DPP_OP(dpp_add_shr1, "v_add_f32_dpp", "wave_shr:1")    // dst = src[l-1] + w  (lane 0 keeps)
HMM355_DPP_OP(dpp_add_shl1, "v_add_f32_dpp", "wave_shl:1")    // dst = src[l+1] + w  (lane 63 keeps)
HMM355_DPP_OP(dpp_add_ror1, "v_add_f32_dpp", "wave_ror:1")    // dst = src[l-1 mod 64] + w
HMM355_DPP_OP(dpp_add_rol1, "v_add_f32_dpp", "wave_rol:1")    // dst = src[l+1 mod 64] + w
HMM355_DPP_OP(dpp_mul_shr1, "v_mul_f32_dpp", "wave_shr:1")
HMM355_DPP_OP(dpp_mul_shl1, "v_mul_f32_dpp", "wave_shl:1")
HMM355_DPP_OP(dpp_mul_ror1, "v_mul_f32_dpp", "wave_ror:1")
HMM355_DPP_OP(dpp_mul_rol1, "v_mul_f32_dpp", "wave_rol:1")
HMM355_DPP_OP(dpp_fmac_shr1, "v_fmac_f32_dpp", "wave_shr:1")  // dst += src[l-1] * w (lane 0 keeps)
HMM355_DPP_OP(dpp_fmac_shl1, "v_fmac_f32_dpp", "wave_shl:1")  // dst += src[l+1] * w (lane 63 keeps)
#undef HMM355_DPP_OP

// dst = dst (op) src[perm(lane)] as ONE VALU instruction, for the in-row reductions of the
// register-blocked dense chain (hipcc emits a separate v_mov_b32_dpp plus a zeroed "old"
// operand for each of these)
#define HMM355_DPP_RED(name, op, ctrl)                                                        \
  __device__ __forceinline__ void name(float& dst, float src) {                               \
    asm("s_nop 1\n\t" op " %0, %1, %0 " ctrl " row_mask:0xf bank_mask:0xf" : "+v"(dst) : "v"(src)); \
  }
HMM355_DPP_RED(red_add_mirror, "v_add_f32_dpp", "row_mirror")
HMM355_DPP_RED(red_add_hmirror, "v_add_f32_dpp", "row_half_mirror")
HMM355_DPP_RED(red_add_q3210, "v_add_f32_dpp", "quad_perm:[3,2,1,0]")
HMM355_DPP_RED(red_add_q1032, "v_add_f32_dpp", "quad_perm:[1,0,3,2]")
HMM355_DPP_RED(red_max_mirror, "v_max_f32_dpp", "row_mirror")
HMM355_DPP_RED(red_max_hmirror, "v_max_f32_dpp", "row_half_mirror")
HMM355_DPP_RED(red_max_q3210, "v_max_f32_dpp", "quad_perm:[3,2,1,0]")
HMM355_DPP_RED(red_max_q1032, "v_max_f32_dpp", "quad_perm:[1,0,3,2]")
#undef HMM355_DPP_RED

// The reduce-scatter of the four output partials of rec_run_rb over the 16 lanes of a row
// (mirror, half mirror, two quad permutations: slot 0 of every lane of quad x ends with output
// 4g + x), written as one block with only the wait states the DPP-read hazard needs (a DPP
// source written by one of the two previous VALU instructions: 2 wait states).  The separate
// helpers above pad every DPP op with "s_nop 1"; here the forward-backward form interleaves the
// all-reduce of the scale c with the outputs' tree, so most reads are two instructions away
// from their writes (tools/mb_dense.hip: 297 -> 279 ns per FB step).  Same operations in the same
// order as the helpers: identical bits.
__device__ __forceinline__ void red4_add_with_c(float& s0, float& s1, float s2, float s3, float& c) {
  asm("s_nop 1\n\t"
      "v_add_f32_dpp %2, %2, %2 row_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %0, %3, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %1, %4, %1 row_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %2, %2 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 0\n\t"
      "v_add_f32_dpp %0, %1, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %2, %2 quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 0\n\t"
      "v_add_f32_dpp %0, %0, %0 quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf\n\t"
      "v_add_f32_dpp %2, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 0\n\t"
      "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
      : "+v"(s0), "+v"(s1), "+v"(c)
      : "v"(s3), "v"(s2));
}
__device__ __forceinline__ void red4_max(float& s0, float& s1, float s2, float s3) {
  asm("s_nop 1\n\t"
      "v_max_f32_dpp %0, %2, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
      "v_max_f32_dpp %1, %3, %1 row_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 0\n\t"
      "v_max_f32_dpp %0, %1, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 quad_perm:[3,2,1,0] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\t"
      "v_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
      : "+v"(s0), "+v"(s1)
      : "v"(s3), "v"(s2));
}

// Window term of slot offset DD in {-1, +1} for state vector v (state 64*blk + lane), weights
// w: Viterbi -> t = v(s + DD) + w (neutral -inf past the ends); FB -> acc += v(s + DD) * w.
template <int NB, bool FB, int DD>
__device__ __forceinline__ void win_term1(const float (&v)[NB], const float (&w)[NB], float (&acc)[NB]) {
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    const bool edge = DD < 0 ? blk == 0 : blk == NB - 1;  // no neighbouring block
    if (FB) {
      if (edge) {
        if (DD < 0) dpp_fmac_shr1(acc[blk], v[blk], w[blk]);
        else dpp_fmac_shl1(acc[blk], v[blk], w[blk]);
      } else {
        float t;
        if (DD < 0) { dpp_mul_ror1(t, v[blk - 1], w[blk]); dpp_mul_shr1(t, v[blk], w[blk]); }
        else { dpp_mul_rol1(t, v[blk + 1], w[blk]); dpp_mul_shl1(t, v[blk], w[blk]); }
        acc[blk] += t;
      }
    } else {
      float t = -INFINITY;
      if (!edge) {
        if (DD < 0) dpp_add_ror1(t, v[blk - 1], w[blk]);
        else dpp_add_rol1(t, v[blk + 1], w[blk]);
      }
      if (DD < 0) dpp_add_shr1(t, v[blk], w[blk]);
      else dpp_add_shl1(t, v[blk], w[blk]);
      acc[blk] = fmaxf(acc[blk], t);
    }
  }
}

// Whole-vector lane shifts of a state vector held as v[blk] = state 64*blk + lane (DPP
// wave_shr:1 / wave_shl:1; the lane that falls off a 64-block takes the neighbouring block's
// edge value through wave_ror:1 / wave_rol:1 passed as the DPP "old" operand).
// out(s) = v(s - 1) (shr) or v(s + 1) (shl); states outside [0, NB*64) read `edge`.
template <int NB>
__device__ __forceinline__ void vec_shr1(const float (&v)[NB], float (&out)[NB], float edge) {
#pragma unroll
  for (int blk = NB - 1; blk >= 0; --blk) {
    const int carry = blk > 0 ? __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v[blk - 1]), 0x13C, 0xF, 0xF, false)
                              : __builtin_bit_cast(int, edge);
    out[blk] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(carry, __builtin_bit_cast(int, v[blk]), 0x138, 0xF, 0xF, false));
  }
}
template <int NB>
__device__ __forceinline__ void vec_shl1(const float (&v)[NB], float (&out)[NB], float edge) {
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
    const int carry = blk < NB - 1 ? __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v[blk + 1]), 0x134, 0xF, 0xF, false)
                                   : __builtin_bit_cast(int, edge);
    out[blk] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(carry, __builtin_bit_cast(int, v[blk]), 0x130, 0xF, 0xF, false));
  }
}
// window slots k = 0..TW-1 <-> states s + TD0 + k, from registers
template <int NB, int TD0, int TW>
__device__ __forceinline__ void vec_window(const float (&v)[NB], float (&win)[NB][TW > 0 ? TW : 1], float edge) {
  float neg[3][NB], pos[3][NB];
  // negative offsets: successive right shifts; positive: successive left shifts
  if constexpr (TD0 < 0) {
    vec_shr1<NB>(v, neg[0], edge);
    if constexpr (TD0 < -1) vec_shr1<NB>(neg[0], neg[1], edge);
    if constexpr (TD0 < -2) vec_shr1<NB>(neg[1], neg[2], edge);
  }
  if constexpr (TD0 + TW - 1 > 0) {
    vec_shl1<NB>(v, pos[0], edge);
    if constexpr (TD0 + TW - 1 > 1) vec_shl1<NB>(pos[0], pos[1], edge);
    if constexpr (TD0 + TW - 1 > 2) vec_shl1<NB>(pos[1], pos[2], edge);
  }
#pragma unroll
  for (int k = 0; k < TW; ++k) {
    const int dd = TD0 + k;
#pragma unroll
    for (int blk = 0; blk < NB; ++blk)
      win[blk][k] = dd == 0 ? v[blk] : (dd < 0 ? neg[-dd - 1][blk] : pos[dd - 1][blk]);
  }
}

struct RecArgs {
  const float* obs;   // (B,T,N) emissions
  const float* mat;   // (N,N) log transition matrix
  const float* init;  // (N) log_p0 (FB alpha, Viterbi) / unused (FB beta)
  float* rows;        // stored rows: FB -> (B,T,NP) scaled alpha/beta; Viterbi -> (B,T,N) delta
  float* ls;          // (B,T) log-scales (FB) or null
  float* loglik;      // (B) sequence log-likelihood (FB alpha) or null
  int B, T, N, obs_mode, row_stride;
  const BandDesc* band;  // banded decomposition (band.h) or null: dense chain
  const float* binit;    // backward only: (B,NP) terminal vector (max-normalised) or null = ones
  const float* bscale;   // backward only: (B) log-scale of binit
  uint8_t* psi;          // Viterbi, fused banded chain only: (B,T,NP) argmax pointers (kVitFused)
  const float* rmax;     // FB with OBS_LOG: (B,T) row maxima M_t (e_t = exp(lo_t - M_t)), else null
  float* out_exp;        // FB: (B,T,N) forward (alpha) / backward (beta) output written at flush, or null
  // Viterbi with psi followers (dense chains, vit_kern.h): chunk maps, path, final score
  uint8_t* G;            // (B, nchunks, NP) chunk maps
  int64_t* states;       // (B,T) decoded path
  float* final_score;    // (B) max of the last trellis row, or null
  int nchunks;
  // Viterbi, dense chain with psi followers (HMM355_VIT_PLAN_DENSE, vit_kern.h): the helpers
  // publish the blocks they have flushed in prog[b * kProgSlots + h]; the follower workgroups
  // (blockIdx >= B) mark the chunks they finished in done[b * nchunks + c]
  int* prog;
  uint8_t* done;
  // FB: (B,T) the normaliser of each step, by time (alpha: cs[t] = c with u_{t+1} = A^T u_t e_{t+1} / c;
  // beta: cs[t] = c with v_{t-1} = A (e_t v_t) / c), written beside LS for the adjoint
  // (autograd.py), or null
  float* cs;
  // Banded chains with followers (follow.h): the helpers' row flushes (FB: U / V rows) and psi
  // row copies (fused Viterbi) are write-through (sc1) stores, and one lane publishes how many
  // 16-step blocks of them are complete in pub[b * 2 + direction] (FB) / pub[b] (Viterbi):
  // blocks [0, pub) done while the chain runs, nblocks + 1 once everything (rows, psi, the last
  // trellis row) is stored; the fused Viterbi chain leaves the path's end state and score in
  // the word kVitEndWord ints past its count before that.  Null: no publishing.
  int* pub;
  // Viterbi with OBS_PROB emissions and log leaders (follow.h vit_lead): lobuf (B,T,N) holds
  // log(x + 1e-8) of 16-step blocks [4, lready[b]) of sequence b, written by the leaders; the
  // staging helpers load a block from there when it is ready (checked two blocks ahead), else
  // the raw emissions, and take the log themselves
  const float* lobuf;
  const int* lready;
  float* lik_ref;        // FB alpha with publishing: (B) the reference's compute_likelihood value
  uint8_t* path;         // Viterbi decode follower: (B, nchunks, NP, 64) chunk paths (follow.h)
  unsigned token;        // the published counts' call token (common.h poll_count / publish_count)
  // FB end rows (post.h kEndBlocks; publishing chains only): the partner chain's rows (alpha: V,
  // beta: U), the posterior output, and kEndsOn | kEndsOddLeft (0: the followers form every row)
  const float* prow;
  float* post;
  unsigned ends;
  int vit_table;         // Viterbi decode follower: keep the end-state table (follow.h; it fits the LDS)
};
constexpr int kProgSlots = 8;  // >= kRbHelpers<NP>::NH

// The banded Viterbi chain computes the argmax pointers psi itself (helper waves on the idle
// SIMDs, from the delta rows still in its LDS ring), so the psi pass only composes the
// 64-step chunk maps from them.  Enabled where the helpers have the issue slots: NP >= 128.
constexpr int kPsiChunk = 64;
template <int NP>
constexpr bool kVitFused = RC<NP>::NW >= 6;
// threads of the Viterbi chain kernel: the fused banded chain runs 16 waves (rec_band: two
// staging helpers and two psi waves on each of SIMDs 1..3); the dense chains use the first
// RC<NP>::NW waves and the rest exit at once
template <int NP>
constexpr int kVitNT = kVitFused<NP> ? (1024 > kRbHelpers<NP>::NT ? 1024 : kRbHelpers<NP>::NT)
                                     : kRbHelpers<NP>::NT;

template <int KIND>
__device__ __forceinline__ int rec_tau(int q, int T) {
  return KIND == kFbBeta ? T - 1 - q : q;
}

// the log table (logcr.h g_logcr_tab): each wave that stages Viterbi emissions copies it into LDS
// itself (identical values from every copier, so no barrier: a wave's own LDS writes precede its reads)
template <int NP>
__device__ __forceinline__ void rec_logt_fill(float* lds, int l) {
  double* t = reinterpret_cast<double*>(lds + RC<NP>::OFF_LOGT);
#pragma unroll
  for (int k = 0; k < 4; ++k) t[l + 64 * k] = g_logcr_tab[l + 64 * k];
}

// ---- emission staging: lane l of wave w holds 4 consecutive states of one step
// r[0..3]: the emissions; r[4]: the step's row maximum M_t (FB with OBS_LOG; the load reads an
// address of the same row otherwise, so the staging stays branch-free, and is not used)
// Viterbi: r[4] is the block's emission form, 1 = log-emissions (OBS_LOG, or rows the log
// leaders converted: `obs` = RecArgs::lobuf), 0 = probabilities (the staging takes the log);
// vmode < 0: from a.obs_mode.
// SC1 (the fused Viterbi chain, whose rows may come from the log leaders in this launch,
// follow.h): every load is an sc1 load (L1 bypassed: no stale line of a row another workgroup
// wrote), from a buffer resource over the sequence's rows of `obs`.
template <int NP, int KIND, bool FULL = false, bool SC1 = false>
__device__ __forceinline__ void rec_load(const RecArgs& a, int b, int blk, int w, int l, float (&r)[5],
                                         const float* obs = nullptr, float vmode = -1.f) {
  const int q = blk * 16 + (l >> 2);
  const int col = 16 * w + 4 * (l & 3);
  const bool qok = q < a.T;
  const int tq = qok ? rec_tau<KIND>(q, a.T) : 0;
  const size_t bt = (size_t)b * a.T + tq;
  const float* src = (obs ? obs : a.obs) + bt * a.N;
  if constexpr (KIND != kVit) {
    const float* mp = a.rmax ? a.rmax + bt : src;  // a pointer select, not a branch
    r[4] = *mp;
  } else {
    r[4] = vmode >= 0.f ? vmode : (a.obs_mode == HMM355_OBS_LOG ? 1.f : 0.f);
  }
  if constexpr (SC1) {
    const __amdgpu_buffer_rsrc_t rs = make_rsrc((obs ? obs : a.obs) + (size_t)b * a.T * a.N, (size_t)a.T * a.N * 4);
    const int off = (tq * a.N + col) * 4;
    if constexpr (FULL) {
      const float4 v = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, kAuxSc1));
      r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = qok && col + k < a.N;
        r[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, ok ? off + 4 * k : 0, 0, kAuxSc1));
      }
    }
    return;
  }
  if constexpr (FULL) {  // full 16-B aligned rows (the caller checked): one 16-B load
    const float4 v = *reinterpret_cast<const float4*>(src + col);
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool ok = qok && col + k < a.N;
    r[k] = src[ok ? col + k : 0];  // no select: the wait lands at the first (masked) use
  }
}

// PERBLK (the fused Viterbi chain with log leaders): the emission form is r[4] of the block's
// registers (rec_load); otherwise a.obs_mode
template <int NP, int KIND, bool PERBLK = false>
__device__ __forceinline__ void rec_stage(const RecArgs& a, float* lds, int blk, int w, int l, const float (&r)[5]) {
  using C = RC<NP>;
  const int sq = l >> 2;
  const int col = 16 * w + 4 * (l & 3);
  const bool qok = blk * 16 + sq < a.T;
  // one uniform branch on the emission mode per call, selects inside: per-element branches
  // bloat the helpers' unrolled code (three block copies x HV virtual waves) and end in
  // waitcnt joins
  float e[4];
  // (Viterbi: the form travels with the block's registers, r[4]; uniform across the wave)
  const bool lg = (KIND == kVit && PERBLK) ? __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, r[4])) != 0
                                          : a.obs_mode == HMM355_OBS_LOG;
  if (lg) {
    // FB: e = exp(lo - M_t) with the row maximum M_t (log-emissions of -100 .. -400 would
    // underflow exp); M_t is carried into the log-scales by rec_flush
    const float m = KIND == kVit ? 0.f : (a.rmax ? r[4] : 0.f);
    if (KIND != kVit && w == 0 && (l & 3) == 0) lds[C::OFF_M + ((blk * 16 + sq) & (C::MRING - 1))] = m;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = qok && col + k < a.N;
      e[k] = KIND == kVit ? (ok ? r[k] : -INFINITY) : (ok ? __expf(r[k] - m) : 0.f);
    }
  } else {
    // Viterbi: log(x + 1e-8) correctly rounded (logcr.h; the fp32 sum as hmm.py:152 forms it)
    const double* lt = reinterpret_cast<const double*>(lds + C::OFF_LOGT);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = qok && col + k < a.N;
      // (diagnostic builds: no log, timing only)
      const float lv = (kAbl & abl::kStageNoLog) ? r[k] + 1e-8f : logcr_fast(r[k] + 1e-8f, lt);
      e[k] = KIND == kVit ? (ok ? lv : -INFINITY) : (ok ? r[k] + 1e-8f : 0.f);
    }
  }
  *reinterpret_cast<float4*>(lds + C::OFF_EMIS + ((blk % 3) * 16 + sq) * NP + col) = make_float4(e[0], e[1], e[2], e[3]);
}

// ---- the Rabiner log-scales of the 16 rows of staging block `blk` (FB):
// LS_rho = LS_{rho-1} + log c_{rho-1}, a 16-lane inclusive scan with the running base in
// double.  Every flushing wave computes it (so each knows its rows' log-scales for the exp
// outputs and keeps its own `base`); the one with write_ls stores LA / LB.  Lane j < 16
// returns LS of row 16*blk + j.
template <int NP, int KIND>
__device__ __forceinline__ float rec_ls_scan(const RecArgs& a, const float* lds, int b, int blk, double& base,
                                             bool write_ls) {
  using C = RC<NP>;
  if constexpr (KIND == kVit) return 0.f;
  const int lane = threadIdx.x & 63, j = lane & 15;
  const int rho = blk * 16 + j;
  const float c = lds[C::OFF_SC + 64 * ((rho - 1) & (C::RING - 1))];  // unconditional (see rec_flush)
  const bool live = lane < 16 && rho >= 1 && rho < a.T;
  float x = live ? __logf(c) : 0.f;
  // the step's normaliser by time for the adjoint (alpha: time rho - 1; beta: time T - rho)
  if (write_ls && a.cs && live)
    a.cs[(size_t)b * a.T + (KIND == kFbBeta ? a.T - rho : rho - 1)] = c;
  if (a.obs_mode == HMM355_OBS_LOG) {
    // shifted emissions: alpha row rho used M_{tau(rho)}, beta row rho used M_{tau(rho)+1}
    // (the row staged as rho - 1); beta row 0 (the terminal vector) none
    const int src = KIND == kFbBeta ? rho - 1 : rho;
    const float m = lds[C::OFF_M + (src & (C::MRING - 1))];
    x += (lane < 16 && src >= 0 && rho < a.T) ? m : 0.f;
  }
  x += dpp_f<0x111>(x);  // row_shr:1
  x += dpp_f<0x112>(x);  // row_shr:2
  x += dpp_f<0x114>(x);  // row_shr:4
  x += dpp_f<0x118>(x);  // row_shr:8
  const float lsv = (float)(base + (double)x);
  if (write_ls && lane < 16 && rho < a.T) a.ls[(size_t)b * a.T + rec_tau<KIND>(rho, a.T)] = lsv;
  base += (double)__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 15));
  return lsv;
}

// ---- flush the 16 stored rows of staging block `blk`; FB with a.out_exp also writes the
// reference's output row exp(log x + LS) (forward = exp(log alpha) for alpha, backward for
// beta, hmm.py:127-128) from the same LDS row, so the posterior pass only forms the posterior.
// lsv: rec_ls_scan's vector (LS of row j in lane j).  A row whose log-scale is below -110 is
// exactly 0 (x <= N <= 256 < e^6 and e^-104 is below the smallest fp32 denormal), as the
// reference's exp underflows: no transcendentals for it.
// (WHAT: 1 the stored rows, 2 the exp outputs, 3 both)
template <int NP, int KIND, int WHAT = 3>
__device__ __forceinline__ void rec_flush(const RecArgs& a, const float* lds, int b, int blk, int tid, float lsv) {
  using C = RC<NP>;
  const int q_base = blk * 16;
  if (a.row_stride == NP) {
    constexpr int PER_ROW = NP / 4;
    const int row = tid / PER_ROW, c4 = (tid % PER_ROW) * 4;
    const int q = q_base + row;
    // the LDS read is unconditional (only the store is guarded): a read under the guard
    // ends in an s_waitcnt vmcnt(0) join that drains the helper's emission prefetches
    const float4 v = *reinterpret_cast<const float4*>(lds + C::OFF_RING + (q & (C::RING - 1)) * NP + c4);
    const size_t tr = (size_t)b * a.T + rec_tau<KIND>(q, a.T);
    if ((WHAT & 1) && q < a.T) {
      if (a.pub && !(kFAbl & fabl::kPlainStores)) {
        // followers read these rows in this launch: write-through (sc1) 16-B stores (follow.h)
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            a.rows + (size_t)b * a.T * NP, (short)0, (int)((size_t)a.T * NP * 4), 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), rs,
                                               (rec_tau<KIND>(q, a.T) * NP + c4) * 4, 0, kAuxSc1);
      } else {
        *reinterpret_cast<float4*>(a.rows + tr * NP + c4) = v;
      }
    }
    if constexpr (KIND != kVit && (WHAT & 2)) {
      if (a.out_exp) {
        const float ls = __shfl(lsv, row);
        // (common.h: a NaN log-scale or a NaN / inf entry of this lane's four gives zeros)
        const bool live = ls >= -110.f && finite_bits(ls) && finite_bits((v.x + v.y) + (v.z + v.w));
        float ov[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) ov[k] = live ? __expf(__logf(ov[k]) + ls) : 0.f;
        if (q < a.T) {
          if (a.N == NP) {
            *reinterpret_cast<float4*>(a.out_exp + tr * NP + c4) = make_float4(ov[0], ov[1], ov[2], ov[3]);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (c4 + k < a.N) a.out_exp[tr * a.N + c4 + k] = ov[k];
          }
        }
      }
    }
  } else {
    for (int idx = tid; idx < 16 * a.N; idx += C::NT) {
      const int row = idx / a.N, col = idx - row * a.N;
      const int q = q_base + row;
      float* dst = a.rows + ((size_t)b * a.T + rec_tau<KIND>(q, a.T)) * a.row_stride + col;
      const float v = lds[C::OFF_RING + (q & (C::RING - 1)) * NP + col];
      if ((WHAT & 1) && q < a.T) {
        if (a.pub && !(kFAbl & fabl::kPlainStores)) __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (sc1)
        else *dst = v;
      }
    }
  }
}

// ---- what the dense and banded chains share ------------------------------------------------

// the staged emission of step rho, state idx (the 3-slot ring of 16-step blocks, rec_stage)
template <int NP>
__device__ __forceinline__ const float& rec_emis(const float* lds, int rho, int idx) {
  return lds[RC<NP>::OFF_EMIS + (((rho >> 4) % 3) * 16 + (rho & 15)) * NP + idx];
}

// Row 0 of state s, whose staged emission of step 0 is e0 (read only where it is used):
// alpha_0 = p0 * e_0, beta_{T-1} = binit or 1, delta_0 = init + lo_0; padded states take the
// neutral element.
template <int NP, int KIND>
__device__ __forceinline__ float rec_row0(const RecArgs& a, int b, int s, const float& e0) {
  const int N = a.N;
  const int ss = s < N ? s : 0;
  if (KIND == kFbAlpha) return s < N ? __expf(a.init[ss]) * e0 : 0.f;  // alpha_0 = p0 * e_0
  if (KIND == kFbBeta) return s < N ? (a.binit ? a.binit[(size_t)b * NP + s] : 1.f) : 0.f;  // beta_{T-1}
  return s < N ? a.init[ss] + e0 : -INFINITY;                          // delta_0 = init + lo_0
}

// Diagnostic builds (kStamp): the cycles of a dense chain wave by step segment, and its record
// in g_rec_stamps (layout above).  Every member does nothing in the product build.
struct RecStamps {
  unsigned long long acc[4] = {0, 0, 0, 0}, prev = 0, t0 = 0, steps = 0;
  long long rt0 = 0;
  __device__ __forceinline__ void begin() {
    if (kStamp) { t0 = stamp(); prev = t0; rt0 = __builtin_amdgcn_s_memrealtime(); }
  }
  // the cycles since the last mark belong to segment k
  __device__ __forceinline__ void mark(int k) {
    if (kStamp) { const unsigned long long t = stamp(); acc[k] += t - prev; prev = t; }
  }
  // lane 0 writes the wave's record into slot `slot`
  __device__ __forceinline__ void finish(unsigned slot) {
    if (kStamp && (threadIdx.x & 63) == 0) {
      const unsigned long long t1 = stamp();
      const long long rt1 = __builtin_amdgcn_s_memrealtime();
      unsigned long long* o8 = g_rec_stamps + ((size_t)slot % kStampWaves) * 8;
      o8[0] = acc[0]; o8[1] = acc[1]; o8[2] = acc[2]; o8[3] = acc[3];
      o8[4] = steps; o8[5] = t1 - t0; o8[6] = t1 - t0; o8[7] = (unsigned long long)(rt1 - rt0);
    }
  }
};

// c_{T-1}, the sum of the last row (the log-likelihood's last term), from each lane's share ys
// of it: one wave forms it and leaves it where rec_loglik reads it
template <int NP>
__device__ __forceinline__ void rec_keep_c_last(float* lds, int T, float ys) {
  const float cs = wave_sum_bcast(ys);
  if ((threadIdx.x & 63) == 0) lds[RC<NP>::OFF_SC + 64 * ((T - 1) & (RC<NP>::RING - 1))] = cs;
}
// loglik = LS_{T-1} + log c_{T-1}, for the wave whose `base` has run through the last block
template <int NP>
__device__ __forceinline__ float rec_loglik(const float* lds, int T, double base) {
  return clean_loglik((float)(base + (double)__logf(lds[RC<NP>::OFF_SC + 64 * ((T - 1) & (RC<NP>::RING - 1))])));
}

// ---------------------------------------------------------------------------------------
// Dense chain, DPP-broadcast form (round 1; the layout of the header comment).  The product
// instantiates it at NP = 256 only: there 16 waves leave 128 VGPRs a lane, too few for the
// register-blocked slices of rec_run_rb, which serves NP <= 128 (rec_dispatch).
template <int NP, int KIND>
__device__ __forceinline__ void rec_run_dpp(const RecArgs& a, float* lds, int b) {
  using C = RC<NP>;
  constexpr bool FB = KIND != kVit;
  const int tid = threadIdx.x;
  const int w = tid >> 6, l = tid & 63, r = l >> 4, c = l & 15;
  const int o = 16 * w + c;  // output of this lane
  const int T = a.T, N = a.N;

  // matrix slice: M[blk][n] = Mat[i][o] (alpha/Viterbi) or Mat[o][i] (beta), i = 64blk+16r+n
  float M[C::NBLK][16];
#pragma unroll
  for (int blk = 0; blk < C::NBLK; ++blk)
#pragma unroll
    for (int n = 0; n < 16; ++n) {
      const int i = 64 * blk + 16 * r + n;
      const bool ok = i < N && o < N;
      const size_t idx = ok ? (KIND == kFbBeta ? (size_t)o * N + i : (size_t)i * N + o) : 0;
      const float v = a.mat[idx];
      M[blk][n] = FB ? __expf(ok ? v : -INFINITY) : (ok ? v : -INFINITY);
    }

  const int nblocks = (T + 15) / 16;
  float er0[5], er1[5];
  if (KIND == kVit) rec_logt_fill<NP>(lds, l);
  rec_load<NP, KIND>(a, b, 0, w, l, er0);
  rec_stage<NP, KIND>(a, lds, 0, w, l, er0);
  if (nblocks > 1) rec_load<NP, KIND>(a, b, 1, w, l, er1);
  lds_barrier();

  auto emis = [&](int rho, int idx) -> const float& { return rec_emis<NP>(lds, rho, idx); };
  // row 0 partials: the whole value in group 0, the identity in groups 1..3
  {
    const float v0 = rec_row0<NP, KIND>(a, b, o, emis(0, o));
    const float ident = FB ? 0.f : -INFINITY;
    if (r < 2) lds[C::OFF_PART + o * 2 + r] = r == 0 ? v0 : ident;
  }
  lds_barrier();

  double base = (KIND == kFbBeta && a.bscale) ? (double)a.bscale[b] : 0.0;
  RecStamps stamps;
  stamps.begin();
  auto mark = [&](int k) { stamps.mark(k); };
  // sum (FB) / max (Viterbi) of the four row-group partials of input 64*blk + lane
  auto gather = [&](int prv, float (&y)[C::NBLK]) {
#pragma unroll
    for (int blk = 0; blk < C::NBLK; ++blk) {
      // one conflict-free ds_read_b64 per block (2 LDS cycles per wave)
      const float2 pp = *reinterpret_cast<const float2*>(lds + C::OFF_PART + (prv * NP + 64 * blk + l) * 2);
      y[blk] = FB ? pp.x + pp.y : fmaxf(pp.x, pp.y);
    }
  };
  // wave 0 keeps the finished row rho (alpha: u, beta: v, Viterbi: delta)
  auto keep_row = [&](int rho, const float (&y)[C::NBLK]) {
    if (w == 0) {
#pragma unroll
      for (int blk = 0; blk < C::NBLK; ++blk) lds[C::OFF_RING + (rho & (C::RING - 1)) * NP + 64 * blk + l] = y[blk];
    }
  };

  auto run_block = [&](int kb, float(&ernext)[5], float(&erfree)[5]) {
    if (!(kAbl & abl::kDppNoBlockWork)) {
      // straight-line staging and loads (the tail stages a padding block and re-loads the
      // last one), as in the banded helpers: exact waitcnt counts
      rec_stage<NP, KIND>(a, lds, kb + 1, w, l, ernext);
      rec_load<NP, KIND>(a, b, kb + 2 < nblocks ? kb + 2 : nblocks - 1, w, l, erfree);
      if (kb >= 2) rec_flush<NP, KIND>(a, lds, b, kb - 2, tid, rec_ls_scan<NP, KIND>(a, lds, b, kb - 2, base, w == C::NW - 1));
    }
    const int q0 = kb * 16 < 1 ? 1 : kb * 16;
    const int q1 = (kb + 1) * 16 < T ? (kb + 1) * 16 : T;
    for (int q = q0; q < q1; ++q) {
      const int prv = (q - 1) & 1, cur = q & 1;
      // the step's emissions are read beside the partials, off the dependent chain
      float eo = 0.f, ey[C::NBLK];
      if (KIND == kFbBeta) {
#pragma unroll
        for (int blk = 0; blk < C::NBLK; ++blk) ey[blk] = emis(q - 1, 64 * blk + l);
      } else {
        eo = emis(q, o);
      }
      float y[C::NBLK];
      if (kStamp) mark(3);
      gather(prv, y);
      if (kStamp) { keep(y[0]); mark(0); }
      keep_row(q - 1, y);
      if (KIND == kFbBeta) {  // beta's product input is y = v * e (hmm.py:113-115)
#pragma unroll
        for (int blk = 0; blk < C::NBLK; ++blk) y[blk] *= ey[blk];
      }
      float part;
      if (FB) {
        // 32 (NP=128) v_fmac_f32_dpp into four accumulators, with the DPP wave sum of the
        // product input (c_{q-1}, the Rabiner normaliser) interleaved stage by stage: issue is
        // in order within a wave, so a sum issued as one block would add its full dependent
        // latency to the step.  sched_barrier pins the interleave.
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        float cx = y[0];
#pragma unroll
        for (int blk = 1; blk < C::NBLK; ++blk) cx += y[blk];
        float cs = 0.f;
        constexpr int G = 4 * C::NBLK;  // groups of 4 fmacs
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const int blk = g >> 2, n0 = 4 * (g & 3);
          if (kAbl & abl::kDppNoProducts) {
            if ((g & 3) == 0) a0 += y[blk];
          } else {
            switch (n0) {
              case 0:  fmac_bcast<0>(a0, y[blk], M[blk][0]);   fmac_bcast<1>(a1, y[blk], M[blk][1]);
                       fmac_bcast<2>(a2, y[blk], M[blk][2]);   fmac_bcast<3>(a3, y[blk], M[blk][3]);   break;
              case 4:  fmac_bcast<4>(a0, y[blk], M[blk][4]);   fmac_bcast<5>(a1, y[blk], M[blk][5]);
                       fmac_bcast<6>(a2, y[blk], M[blk][6]);   fmac_bcast<7>(a3, y[blk], M[blk][7]);   break;
              case 8:  fmac_bcast<8>(a0, y[blk], M[blk][8]);   fmac_bcast<9>(a1, y[blk], M[blk][9]);
                       fmac_bcast<10>(a2, y[blk], M[blk][10]); fmac_bcast<11>(a3, y[blk], M[blk][11]); break;
              default: fmac_bcast<12>(a0, y[blk], M[blk][12]); fmac_bcast<13>(a1, y[blk], M[blk][13]);
                       fmac_bcast<14>(a2, y[blk], M[blk][14]); fmac_bcast<15>(a3, y[blk], M[blk][15]); break;
            }
          }
          // wave-sum stages spread over the groups (all eight done by the last group)
#pragma unroll
          for (int st = (g * 8) / G; st < ((g + 1) * 8) / G; ++st) {
            switch (st) {
              case 0: cx += dpp_f<0xB1>(cx); break;   // quad_perm [1,0,3,2]
              case 1: cx += dpp_f<0x4E>(cx); break;   // quad_perm [2,3,0,1]
              case 2: cx += dpp_f<0x124>(cx); break;  // row_ror:4
              case 3: cx += dpp_f<0x128>(cx); break;  // row_ror:8
              case 4:
                cx += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, cx), 0x142, 0xA, 0xF, false));
                break;                                // row_bcast:15
              case 5:
                cx += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, cx), 0x143, 0xC, 0xF, false));
                break;                                // row_bcast:31
              case 6: cs = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cx), 63)); break;
              default: break;
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        const float scale = __builtin_amdgcn_rcpf(cs);
        if (tid == 0) lds[C::OFF_SC + 64 * ((q - 1) & (C::RING - 1))] = cs;
        float h0 = (a0 + a1) + (a2 + a3), h1 = h0;
        permlane32_swap(h0, h1);  // rows {0,2} / {1,3} summed: lanes 0..31 hold both halves
        const float acc = h0 + h1;
        // alpha: u_q = z * e_q / c_{q-1};  beta: v_q = z / c_{q-1}
        part = KIND == kFbAlpha ? acc * (scale * eo) : acc * scale;
      } else {
        float m0 = -INFINITY, m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
#pragma unroll
        for (int blk = 0; blk < C::NBLK; ++blk) {
          if (kAbl & abl::kDppNoProducts) { m0 = fmaxf(m0, y[blk]); continue; }
          m0 = fmaxf(m0, fmaxf(row_bcast<0>(y[blk]) + M[blk][0], row_bcast<1>(y[blk]) + M[blk][1]));
          m1 = fmaxf(m1, fmaxf(row_bcast<2>(y[blk]) + M[blk][2], row_bcast<3>(y[blk]) + M[blk][3]));
          m2 = fmaxf(m2, fmaxf(row_bcast<4>(y[blk]) + M[blk][4], row_bcast<5>(y[blk]) + M[blk][5]));
          m3 = fmaxf(m3, fmaxf(row_bcast<6>(y[blk]) + M[blk][6], row_bcast<7>(y[blk]) + M[blk][7]));
          m0 = fmaxf(m0, fmaxf(row_bcast<8>(y[blk]) + M[blk][8], row_bcast<9>(y[blk]) + M[blk][9]));
          m1 = fmaxf(m1, fmaxf(row_bcast<10>(y[blk]) + M[blk][10], row_bcast<11>(y[blk]) + M[blk][11]));
          m2 = fmaxf(m2, fmaxf(row_bcast<12>(y[blk]) + M[blk][12], row_bcast<13>(y[blk]) + M[blk][13]));
          m3 = fmaxf(m3, fmaxf(row_bcast<14>(y[blk]) + M[blk][14], row_bcast<15>(y[blk]) + M[blk][15]));
        }
        float h0 = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3)), h1 = h0;
        permlane32_swap(h0, h1);
        // delta_q = max(...) + lo_q: adding lo to each partial max is exact (monotone)
        part = fmaxf(h0, h1) + eo;
      }
      if (kStamp) { keep(part); mark(1); }
      if (l < 32) lds[C::OFF_PART + (cur * NP + o) * 2 + r] = part;
      if (kStamp) { mark(2); ++stamps.steps; }
      step_barrier();
    }
  };
  for (int k = 0; k < nblocks; k += 2) {
    run_block(k, er1, er0);
    if (k + 1 < nblocks) run_block(k + 1, er0, er1);
  }
  stamps.finish(blockIdx.x * C::NW + w);
  // final row T-1 (its partials were written by the last step, or are the init for T == 1)
  float y[C::NBLK];
  gather((T - 1) & 1, y);
  keep_row(T - 1, y);
  if (KIND == kFbAlpha && a.loglik && w == C::NW - 1) {
    float ys = y[0];
#pragma unroll
    for (int blk = 1; blk < C::NBLK; ++blk) ys += y[blk];
    rec_keep_c_last<NP>(lds, T, ys);  // (loglik only)
  }
  lds_barrier();
  if (nblocks >= 2)
    rec_flush<NP, KIND>(a, lds, b, nblocks - 2, tid, rec_ls_scan<NP, KIND>(a, lds, b, nblocks - 2, base, w == C::NW - 1));
  rec_flush<NP, KIND>(a, lds, b, nblocks - 1, tid, rec_ls_scan<NP, KIND>(a, lds, b, nblocks - 1, base, w == C::NW - 1));
  if (KIND == kFbAlpha && a.loglik && tid == C::NT - 64) {
    // loglik = LS_{T-1} + log c_{T-1}; `base` (wave NW-1) now holds LS_{T-1}
    a.loglik[b] = clean_loglik((float)(base + (double)__logf(lds[C::OFF_SC + 64 * ((T - 1) & (C::RING - 1))])));
  }
}

// ---------------------------------------------------------------------------------------
// Dense chain helpers (round 4).  The per-16-step block work of the register-blocked chain --
// the next block's emission staging (exp / log), the global loads two blocks ahead, the log-scale
// scan and the flush of the rows two blocks back (rows + the exp(log x + LS) output) -- costs the
// chain waves ~55 ns per step when they do it themselves between two steps
// (tools/mb_dense.hip: 229 -> 285 ns per FB step, 267 -> 325 Viterbi, prefetched), since every
// wave waits at the next barrier for the slowest.  kRbHelpers<NP>::NH extra waves (launched
// beside the NW chain waves) do it instead, one item per step, each item small enough to finish
// inside the step they share a barrier with:
//   item 0, 1    stage block kb + 1, column slices 2h, 2h + 1 (from registers loaded a block ago)
//   item 2, 3    load block kb + 2 (clamped), the same slices
//   item 4       the log-scale scan of block kb - 2 (every helper keeps its own running base;
//                the last one writes LS)
//   item 5, 6    flush block kb - 2, rows 0..7 and 8..15
//   (Viterbi with psi followers: item 0 also publishes the blocks flushed a block earlier,
//   once per chunk)
// Barriers: the helpers pass exactly the chain's barriers (two before the loop, one per step,
// one after), so the s_barrier counts of all waves agree.  The last two blocks are flushed by
// the helpers after the loop, and the FB log-likelihood (which needs the running base) is
// written by the last helper.
// items per block.  (An eighth, empty item per block measured 58 ns per step slower on the
// dense FB chain, 828 -> 944 us per op, profiles/r4k_ops.log: the publish rides on item 0.)
template <int KIND>
constexpr int kRbItems = 7;


template <int NP, int KIND>
__device__ __forceinline__ void rec_rb_helper(const RecArgs& a, float* lds, int b) {
  using C = RC<NP>;
  constexpr int NH = kRbHelpers<NP>::NH;
  const int tid = threadIdx.x;
  const int h = (tid >> 6) - C::NW, l = tid & 63, th = tid - C::NT;
  const int T = a.T;
  const int kb0 = 0;
  const int nblocks = (T + 15) / 16;
  // register sets: [set = block & 1][slice 0/1][5]
  float er[2][2][5];
  if (KIND == kVit) rec_logt_fill<NP>(lds, l);
  if (nblocks > kb0 + 1) {
    rec_load<NP, KIND>(a, b, kb0 + 1, 2 * h, l, er[1][0]);
    rec_load<NP, KIND>(a, b, kb0 + 1, 2 * h + 1, l, er[1][1]);
  }
  lds_barrier();  // (the chain's: block 0 staged)
  lds_barrier();  // (the chain's: row 0 written)
  double base = (KIND == kFbBeta && a.bscale) ? (double)a.bscale[b] : 0.0;
  float lsv = 0.f;
  // psi followers (Viterbi, vit_kern.h): the count of flushed blocks, published once per 64-step
  // chunk.  Every helper waits for its own flush stores (a workgroup-scope release: vmcnt(0), no
  // cache maintenance) before the step barrier; one lane of helper 0 then, after the barrier,
  // makes them visible to the other XCDs (an agent-scope release: this XCD's L2 written back)
  // and stores the count.  Agent-scope releases are L2-wide: per block and helper they slowed
  // the whole chip (Viterbi op 0.77 -> 1.79 ms), so there is one per chunk and sequence.
  const bool follow = KIND == kVit && a.prog;
  auto flushed = [&]() {
    if (follow) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  };
  auto publish = [&](int blocks) {
    if (follow && h == 0 && l == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      __hip_atomic_store(a.prog + (size_t)b * kProgSlots, blocks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  };
  // item it of block kb; `set` = kb & 1 as a template-free pair of branches over er[0] / er[1]
  auto item = [&](int kb, int it, float(&cur)[2][5], float(&nxt)[2][5]) {
    // cur: block kb + 1's rows (loaded a block ago); nxt: block kb + 2's (loaded now)
    switch (it) {
      case 0:
        if (kb + 1 < nblocks) rec_stage<NP, KIND>(a, lds, kb + 1, 2 * h, l, cur[0]);
        // (Viterbi with psi followers) blocks 0 .. kb - 3 were flushed in block kb - 1, before
        // the barriers since: publish them once per chunk
        if (kb >= kb0 + 3 && ((kb - 2) & 3) == 0) publish(kb - 2);
        break;
      case 1: if (kb + 1 < nblocks) rec_stage<NP, KIND>(a, lds, kb + 1, 2 * h + 1, l, cur[1]); break;
      case 2: rec_load<NP, KIND>(a, b, kb + 2 < nblocks ? kb + 2 : nblocks - 1, 2 * h, l, nxt[0]); break;
      case 3: rec_load<NP, KIND>(a, b, kb + 2 < nblocks ? kb + 2 : nblocks - 1, 2 * h + 1, l, nxt[1]); break;
      case 4: if (kb >= kb0 + 2) lsv = rec_ls_scan<NP, KIND>(a, lds, b, kb - 2, base, h == NH - 1); break;
      case 5: if (kb >= kb0 + 2) rec_flush<NP, KIND>(a, lds, b, kb - 2, th, lsv); break;
      case 6:
        if (kb >= kb0 + 2) {
          rec_flush<NP, KIND>(a, lds, b, kb - 2, th + NH * kWave, lsv);
          flushed();
        }
        break;
      default: break;
    }
  };
  const int qend = nblocks * 16 < T ? nblocks * 16 : T;
  auto run_block = [&](int kb, float(&cur)[2][5], float(&nxt)[2][5]) {
    const int q0 = kb * 16 < 1 ? 1 : kb * 16;
    const int q1 = (kb + 1) * 16 < qend ? (kb + 1) * 16 : qend;
    int it = 0;
    for (int q = q0; q < q1; ++q, ++it) {
      if (it < kRbItems<KIND>) item(kb, it, cur, nxt);
      step_barrier();
    }
    for (; it < kRbItems<KIND>; ++it) item(kb, it, cur, nxt);  // (a short last block)
  };
  // block kb stages block kb + 1 from set (kb + 1) & 1 and loads block kb + 2 into set kb & 1
  for (int k = kb0; k < nblocks; k += 2) {
    run_block(k, er[1], er[0]);
    if (k + 1 < nblocks) run_block(k + 1, er[0], er[1]);
  }
  lds_barrier();  // (the chain's: the last rows and c_{T-1} written)
  static_assert(2 * NH * kWave == C::NT, "two flush passes cover the block");
  if (nblocks >= kb0 + 2) {
    lsv = rec_ls_scan<NP, KIND>(a, lds, b, nblocks - 2, base, h == NH - 1);
    rec_flush<NP, KIND>(a, lds, b, nblocks - 2, th, lsv);
    rec_flush<NP, KIND>(a, lds, b, nblocks - 2, th + NH * kWave, lsv);
  }
  lsv = rec_ls_scan<NP, KIND>(a, lds, b, nblocks - 1, base, h == NH - 1);
  rec_flush<NP, KIND>(a, lds, b, nblocks - 1, th, lsv);
  rec_flush<NP, KIND>(a, lds, b, nblocks - 1, th + NH * kWave, lsv);
  if (follow) {
    flushed();
    __syncthreads();  // (the chain waves have ended: the helpers alone)
    publish(nblocks);
  }
  if (KIND == kFbAlpha && a.loglik && h == NH - 1 && l == 0) {
    a.loglik[b] = clean_loglik((float)(base + (double)__logf(lds[C::OFF_SC + 64 * ((T - 1) & (C::RING - 1))])));
  }
}

// ---------------------------------------------------------------------------------------
// Dense chain, register-blocked form (round 3; NP <= 128 in the product).  The round-2
// register-operand form (removed) gave each lane ONE output and 16 inputs
// per 64-block, so every step moved NP * NP * 4 bytes out of LDS (64 KiB at NP = 128:
// 64 ds_read_b128 = 256 LDS-array cycles, the largest term of its ~830-cycle step).
// Here each lane owns FOUR outputs and NP/16 inputs, so the same products
// need a quarter of the LDS traffic (2 ds_read_b128 per lane at NP = 128):
//   * wave w, row r (lane >> 4) owns output group g = 4w + r, i.e. outputs 4g .. 4g+3; lane
//     c (lane & 15) of the row owns inputs 64m + 4c .. 64m + 4c + 3 (m < NP/64), read as one
//     float4 per block (the four rows of a wave read the same addresses: broadcasts; the 16
//     lanes of each ds_read_b128 lane group read 16 distinct 16-B slots: conflict-free);
//   * the 4 x NP/16 products per lane run as packed fp32 (v_pk_fma_f32 over input pairs;
//     Viterbi v_pk_add_f32 + v_max3_f32) into four per-output accumulators;
//   * the 16 lanes of a row are reduced by a reduce-scatter of DPP adds / maxes with no
//     selects: register slot k of lane c holds output k ^ (c >> 2) (the matrix slice is loaded
//     in that order), so row_mirror (c <-> 15 - c) pairs slots {0,1} with the partner's {3,2},
//     row_half_mirror (c <-> c ^ 7) slot 0 with the partner's slot 1, and two quad_perms finish:
//     5 DPP operations, after which quad c >> 2 holds output 4g + (c >> 2);
//   * lane (c & 3) == 0 of each quad writes it straight into the row ring (the ring row q is
//     both the exchange buffer the next step reads and the row that is flushed), so a step is
//     2 reads, ~25 (FB) / ~37 (Viterbi) VALU operations, 1 write and one s_barrier.
// Forward-backward keeps Rabiner scaling: c_{q-1} = sum of the step's input vector, formed
// by each row from its 16 lanes' partial sums (4 more DPP adds beside the products, the same
// bits in every row).  Beta's product input v * e sits in Pv[2][NP] (OFF_PART).
template <int NP, int KIND>
__device__ __forceinline__ void rec_run_rb(const RecArgs& a, float* lds, int b) {
  using C = RC<NP>;
  constexpr bool FB = KIND != kVit;
  constexpr int NM = NP / 64;  // float4 input blocks per lane
  typedef float f2 __attribute__((ext_vector_type(2)));
  const int tid = threadIdx.x;
  if (tid >= C::NT) {  // the block-work helpers (kRbHelpers)
    rec_rb_helper<NP, KIND>(a, lds, b);
    return;
  }
  // the chain waves issue first: a helper takes the SIMD only while they wait (LDS, barrier)
  // (one priority for all chain waves: the younger half one level above the older half,
  // MI355X_MICROARCH.md "Two waves per SIMD" item 4, measured the same, round 5)
  __builtin_amdgcn_s_setprio(2);
  const int w = tid >> 6, l = tid & 63, r = l >> 4, c = l & 15;
  const int g = 4 * w + r;      // output group
  const int x = c >> 2;         // register slot k holds output 4g + (k ^ x)
  const int o = 4 * g + x;      // the output this lane's quad finishes
  const int T = a.T, N = a.N;
  float* ring = lds + C::OFF_RING;
  float* Pv = lds + C::OFF_PART;  // [2][NP] beta: product input v * e

  // matrix slice: Mk[k][m][p] = (Mat[i][ok], Mat[i+1][ok]) for inputs i = 64m + 4c + 2p,
  // output ok = 4g + (k ^ x); beta takes Mat[ok][i]; FB stores exp(log P)
  f2 Mk[4][NM][2];
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 64 * m + 4 * c + e, ok = 4 * g + (k ^ x);
        const bool in = i < N && ok < N;
        const size_t idx = in ? (KIND == kFbBeta ? (size_t)ok * N + i : (size_t)i * N + ok) : 0;
        const float v = a.mat[idx];
        Mk[k][m][e >> 1][e & 1] = FB ? __expf(in ? v : -INFINITY) : (in ? v : -INFINITY);
      }

  const int qend = T;
  const int nblocks = (qend + 15) / 16;
  {
    float er0[5];
    if (KIND == kVit) rec_logt_fill<NP>(lds, l);
    rec_load<NP, KIND>(a, b, 0, w, l, er0);
    rec_stage<NP, KIND>(a, lds, 0, w, l, er0);
  }
  lds_barrier();  // (block 1 on: the helpers stage)

  auto emis = [&](int rho, int idx) -> const float& { return rec_emis<NP>(lds, rho, idx); };
  const bool writer = (c & 3) == 0;
  {
    const float v0 = rec_row0<NP, KIND>(a, b, o, emis(0, o));
    if (writer) {
      ring[o] = v0;
      if (KIND == kFbBeta) Pv[o] = v0 * emis(0, o);
    }
  }
  lds_barrier();

  RecStamps stamps;
  stamps.begin();
  auto mark = [&](int k) { stamps.mark(k); };

  // one step q of the chain (ring row q from row q - 1)
  auto stepq = [&](int q) {
    if (kStamp) mark(3);
    const float* src = KIND == kFbBeta ? Pv + ((q - 1) & 1) * NP : ring + ((q - 1) & (C::RING - 1)) * NP;
    // alpha / Viterbi: emission of output o; beta: of v_q -> P.  Read first and pinned below:
    // used only by the writer lanes, it would otherwise sink behind the reduction into their
    // branch and put an LDS round trip on the chain
    float eo = emis(q, o);
    f2 yin[NM][2];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      const float4 v4 = *reinterpret_cast<const float4*>(src + 64 * m + 4 * c);
      yin[m][0] = f2{v4.x, v4.y};
      yin[m][1] = f2{v4.z, v4.w};
    }
    keep(eo);
    if (kStamp) { keep(yin[0][0]); mark(0); }
    float s0, s1, s2, s3;
    float cs = 0.f;
    if (FB) {
      f2 acc[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = f2{0.f, 0.f};
      f2 ysum = f2{0.f, 0.f};
#pragma unroll
      for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
          for (int k = 0; k < 4; ++k) acc[k] = __builtin_elementwise_fma(yin[m][p], Mk[k][m][p], acc[k]);
          ysum += yin[m][p];
        }
      // c_{q-1}: the row's 16 lanes hold all NP inputs; an all-reduce of their sums (every
      // lane, every row and every wave ends with the same bits), interleaved with the outputs'
      // reduction (issue is in order within a wave)
      float cx = ysum.x + ysum.y;
      s0 = acc[0].x + acc[0].y; s1 = acc[1].x + acc[1].y;
      s2 = acc[2].x + acc[2].y; s3 = acc[3].x + acc[3].y;
      red4_add_with_c(s0, s1, s2, s3, cx);
      cs = cx;
    } else {
      // the four packed sums of one input pair first, then their max3 folds: no max waits on
      // the packed add just issued (tools/mb_dense.hip: 329 -> 291 ns per step), and the first
      // pair initialises the maxima (no max against -inf)
      float mx[4];
#pragma unroll
      for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          f2 t[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) t[k] = yin[m][p] + Mk[k][m][p];
#pragma unroll
          for (int k = 0; k < 4; ++k)
            mx[k] = (m == 0 && p == 0) ? fmaxf(t[k].x, t[k].y) : fmaxf(fmaxf(mx[k], t[k].x), t[k].y);
        }
      s0 = mx[0]; s1 = mx[1]; s2 = mx[2]; s3 = mx[3];
      red4_max(s0, s1, s2, s3);
    }
    if (kStamp) { keep(s0); mark(1); }
    float val, pval = 0.f;
    if (FB) {
      const float scale = __builtin_amdgcn_rcpf(cs);
      // (every lane holds the same c: wave 0 writes it, a wave-uniform branch)
      if (w == 0) lds[C::OFF_SC + 64 * ((q - 1) & (C::RING - 1))] = cs;
      val = KIND == kFbAlpha ? s0 * (scale * eo) : s0 * scale;  // alpha: u_q = z e_q / c;  beta: v_q = z / c
      if (KIND == kFbBeta) pval = val * eo;
    } else {
      val = s0 + eo;  // delta_q = max(...) + lo_q (exact: monotone)
    }
    // The four lanes of a quad hold the same bits (the last two reduction levels are
    // all-reduces of commutative pairs), so all of them store: no divergent writer branch
    // (tools/mb_dense.hip: 291 -> 268 ns per Viterbi step, 255 -> 229 ns FB)
    ring[(q & (C::RING - 1)) * NP + o] = val;
    if (KIND == kFbBeta) Pv[(q & 1) * NP + o] = pval;
    if (kStamp) { mark(2); ++stamps.steps; }
    step_barrier();
  };
  auto run_block = [&](int kb) {
    const int q0 = kb * 16 < 1 ? 1 : kb * 16;
    const int q1 = (kb + 1) * 16 < qend ? (kb + 1) * 16 : qend;
    if (q0 == kb * 16 && q1 == q0 + 16) {
      // a whole 16-step block, unrolled: the ring / staging indices of every step are the
      // block's plus a constant, so no per-step scalar index arithmetic (round 5: the rolled
      // loop spent ~20 SALU instructions per step on them; the dense FB op 714 -> 646 us,
      // Viterbi 788 -> 764 us alone at B=32, T=2000, N=128, tools/ab.py, profiles/r5j_ab.log)
#pragma unroll
      for (int i = 0; i < 16; ++i) stepq(kb * 16 + i);
    } else {
      for (int q = q0; q < q1; ++q) stepq(q);
    }
  };
  for (int k = 0; k < nblocks; ++k) run_block(k);
  stamps.finish(blockIdx.x * C::NW + w);
  if (KIND == kFbAlpha && a.loglik && w == C::NW - 1) {
    float ys = 0.f;
#pragma unroll
    for (int m = 0; m < NM; ++m) ys += ring[((T - 1) & (C::RING - 1)) * NP + 64 * m + l];
    rec_keep_c_last<NP>(lds, T, ys);  // (loglik only)
  }
  lds_barrier();  // the last blocks' flush and the log-likelihood: the helpers
}

// Window term n of a register-window chain (band_chain, TW > 0: NB states per lane, offsets
// TD0 + k): state j = n % NB, slot k = n / NB.  Its source NB*l + j + TD0 + k lies in another
// lane -- one or two DPP lane shifts -- when this holds.
constexpr bool win_term_shifted(int n, int NB, int TD0) { return (n % NB + TD0 + n / NB + 4 * NB) / NB != 4; }
// its source as one number: register jj of the lane qq lanes on, NB * (qq + 4) + jj
constexpr int win_term_src(int n, int NB, int TD0) { return n % NB + TD0 + n / NB + 4 * NB; }
// the m-th distinct shifted source behind the first terms (k >= 1) of NWIN, as the first term
// that reads it (two terms may read the same one: offsets 0 .. +2 at two states per lane);
// m < 0: how many there are
constexpr int win_shift_term(int m, int NB, int NWIN, int TD0) {
  int c = 0;
  for (int n = NB; n < NWIN; ++n) {
    bool first = win_term_shifted(n, NB, TD0);
    for (int p = NB; p < n; ++p) first = first && win_term_src(p, NB, TD0) != win_term_src(n, NB, TD0);
    if (first && c++ == m) return n;
  }
  return c;
}

// The banded chain wave (wave 0 of rec_band; waves 0 and 1 of the forward-backward pair
// kernel, fbpair.h): the whole recursion of one sequence in one wave, one lds_barrier per
// 16-step block and one after the last row, matching the helpers' barriers.  `lds` is the
// chain's own RC<NP> layout.
// EDGE: the loop over whole blocks of round 12 (run_edge below), whose barrier stands EA steps
// before the block's end; rec_band's chains take it, the pair kernel's (fbpair.h: EA = 1, two
// layouts in a workgroup) keep run_blocks, the loop they had.
template <int NP, int KIND, int WP, int TD0 = 0, int TW = 0, int EA = emis_ahead(KIND), bool EDGE = false>
__device__ __forceinline__ void band_chain(const RecArgs& a, float* lds, int b, const BandDesc* __restrict__ d) {
  using C = RC<NP>;
  constexpr int NB = C::NBLK;
  constexpr bool FB = KIND != kVit;
  constexpr bool FUSE = KIND == kVit && kVitFused<NP>;
  const int l = threadIdx.x & 63;
  const int T = a.T, N = a.N;
  const int nblocks = (T + 15) / 16;
  // ------------------------------------------------------------------ chain wave
  // Lane l holds the consecutive states s = NB*l + j (j < NB): a window offset of +-1 is
  // then another register of the same lane or ONE DPP lane shift (zero-filled at the wave
  // edge, where the window weight is the neutral element).  The compiler folds the shift into
  // the instruction that consumes it where that is a VOP2 when the DPP combiner runs: Viterbi's
  // add (v_add_f32_dpp) and the forward-backward window sum's first term, a product
  // (v_mul_f32_dpp, see `term` below).  The sum's later terms are fmas then (VOP3, no DPP form;
  // they become v_fmac only afterwards), so their shifts stay a v_mov_b32_dpp each (NP = 128
  // listings).  A wave issues one instruction per ~4 cycles, so the step is
  // written for instruction count: 16-step blocks fully unrolled (no scalar address math),
  // the emission read EA steps ahead (emis_ahead), the block's normalisers collected by v_writelane and
  // stored once per block.
  constexpr int WW = TW > 0 ? TW : WP;  // window slots per state
  int lo[NB];
  float wv[NB][WW], fl[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int s = NB * l + j;
    lo[j] = KIND == kFbBeta ? d->rlo[s] : d->clo[s];
#pragma unroll
    for (int k = 0; k < WW; ++k) {
      if (TW > 0)
        wv[j][k] = KIND == kVit ? d->tL[s][k] : (KIND == kFbAlpha ? d->tD[s][k] : d->tR[s][k]);
      else
        wv[j][k] = KIND == kVit ? d->cL[s][k] : (KIND == kFbAlpha ? d->cD[s][k] : d->rD[s][k]);
    }
    fl[j] = KIND == kVit ? d->rfl[s] : d->afl[s];
  }
  const bool uafl = d->uafl != 0;  // one floor for every row: weighted sum = afl0 * plain sum
  const float afl0 = d->afl[0];
  auto erow = [&](int rho) { return lds + C::OFF_EMIS + (((rho >> 4) % 3) * 16 + (rho & 15)) * NP + NB * l; };
  auto ld = [&](const float* p, float(&v)[NB]) {
    if constexpr (NB == 1) v[0] = p[0];
    else if constexpr (NB == 2) { const float2 t = *reinterpret_cast<const float2*>(p); v[0] = t.x; v[1] = t.y; }
    else { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
  };
  // one empty asm over a whole register set: the compiler's wait for its read stands ahead of it
  auto pin_all = [&](float(&v)[NB]) {
    if constexpr (NB == 1) asm volatile("" : "+v"(v[0]));
    else if constexpr (NB == 2) asm volatile("" : "+v"(v[0]), "+v"(v[1]));
    else asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
  };
  auto st = [&](float* p, const float(&v)[NB]) {
    if constexpr (NB == 1) p[0] = v[0];
    else if constexpr (NB == 2) *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    else *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  };
  float y[NB];
  {
    float e0[NB];
    ld(erow(0), e0);
#pragma unroll
    for (int j = 0; j < NB; ++j) y[j] = rec_row0<NP, KIND>(a, b, NB * l + j, e0[j]);
  }
  float* ybuf = lds + C::OFF_PART;  // beta's LDS window source [2][NP] (LDS-window mode)
  constexpr int EL = KIND == kFbBeta ? 1 : 0;
  // the coming steps' emissions (alpha / Viterbi e_q, beta e_{q-1}), read EA steps ahead inside
  // an unrolled block: step jj takes slot jj % EA and refills it with the row of step jj + EA
  float en[EA][NB];
  // the step sum's pinned form (prod_sum): which product of the first pair is fused.  What the
  // compiler chose per instantiation before the form was written out: the first one for four
  // states per lane and for two with a Toeplitz window of offsets 0 .. +1 or 0 .. +2, else the
  // second (read from the NP = 128 / 256 listings; LDS-window chains of NP = 128: the second)
  constexpr bool kSumFirst = NB == 4 || (NB == 2 && TW >= 2 && TD0 >= 0);
  float pp[NB], ee[NB];  // alpha: the factors of the row's products y_j = pp_j * ee_j, for the next step's sum
  float gprev = -INFINITY;  // (abl::kBandReducePrev)

  // the value of state s + dd (s = NB*l + j) from register vector v
  auto at = [&](const float(&v)[NB], int j, int dd) -> float {
    const int t = j + dd + 4 * NB;
    const int qq = t / NB - 4, jj = t % NB;
    const int x = __builtin_bit_cast(int, v[jj]);
    if (qq == 0) return v[jj];
    if (qq == -1) return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x138, 0xF, 0xF, true));
    if (qq == 1) return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, x, 0x130, 0xF, 0xF, true));
    if (qq == -2) {
      const int t1 = __builtin_amdgcn_update_dpp(0, x, 0x138, 0xF, 0xF, true);
      return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, t1, 0x138, 0xF, 0xF, true));
    }
    const int t1 = __builtin_amdgcn_update_dpp(0, x, 0x130, 0xF, 0xF, true);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, t1, 0x130, 0xF, 0xF, true));
  };

  // UA: uniform floor (alpha), a compile-time branch: a runtime one splits every unrolled
  // step into basic blocks whose joins wait for all outstanding LDS reads
  // Per-step LDS addresses come from per-block bases (row / emission slots of step jj are
  // base + jj * NP: immediate offsets), and the step's normaliser c (FB) / floor maximum M
  // (fused Viterbi psi) goes into lane jj of `blk` by v_writelane, stored once per block
  // (lanes < 16, after the last step): no per-step address arithmetic or scalar-to-vector
  // moves on the chain.
  //
  // A lone wave issues one instruction per ~4 cycles in order, and each of the six dependent
  // DPP levels of the step's wave reduction may read its source only two issue slots after the
  // level before wrote it.  Whatever the step holds that does not read the reduction (its
  // `units`) is issued around it, where the slots would otherwise be s_nop pads: the row store
  // and the next emission load, the window reads (LDS-window mode) and the window terms
  // themselves -- FB: every fma into acc, the normaliser enters only in the closing fma; Viterbi:
  // the adds v + w of the closing max.  (With per-row floors the alpha window sum starts from the
  // second reduction, the weighted sum, so its fmas stay behind.)
  // Units, in issue order (loads early, their consumers late):
  //   0 the window source's store | the window reads | beta, LDS mode: the row store |
  //   the emission load | the window terms (beta, register windows: the first terms | the lane
  //   shifts of the later terms | the later terms)
  // beta and Viterbi pin them inside the reduction (wave_red_fill).  alpha issues them ahead of
  // the plain reduction and leaves the placing to the compiler: pinned, its step measured slower
  // under every allocation tried.
  // (The v_writelane of the normaliser is an asm statement, which the hazard recognizer does not
  // count as a slot: inside a gap it would be padded as if it were not there, so it stays behind
  // v_readlane.)
  // FP (alpha): the previous step ran in the same unrolled block, so its products are in reach
  // of this step's sum; else the sum of the finished row
  // RL (beta): the step's input row came across a loop's back edge -- every step of the rolled
  // loop (the partial blocks) and step 0 of an unrolled block -- where the compiler had fused
  // the first product whatever the window
  // ES: the slot of `en` the step takes its emission from and reads enext into (no_read: nothing
  // left to read in this block)
  // PW (EA = 2, the chains whose reduction is filled): the wait for the NEXT step's row, read a
  // step ago, stands in gap emis_wait_gap of this step's reduction, where it takes the place of a
  // wait state the level behind it needs anyway; left to the compiler it stands ahead of the
  // row's first use, an issue slot of its own in every step
  auto step = [&](int q, int jj, bool no_read, auto UA, auto FP, auto RL, auto ES, auto PW, float* row, const float* enext,
                  float& blk, auto wlane) {
    constexpr bool FILLED = KIND != kFbAlpha;
    constexpr int RF = red_form(KIND);  // the form of the step's reductions (wave_red_level)
    constexpr bool LW = TW == 0;                                     // LDS-window mode
    constexpr bool WFILL = !(KIND == kFbAlpha && !decltype(UA)::value);  // the window terms are fillers
    constexpr int NWIN = NB * WW;
    // SPLIT (beta, register windows): a lane shift that no instruction can take in (below) is a
    // unit of its own, ahead of the terms that read it, so a gap of the reduction can hold it alone
    constexpr bool SPLIT = FILLED && FB && !LW;
    constexpr int NSH = SPLIT ? win_shift_term(-1, NB, NWIN, TD0) : 0;
    constexpr int O_LD = 1, O_ST2 = O_LD + (LW ? NWIN : 0), O_EN = O_ST2 + (LW && KIND == kFbBeta ? 1 : 0);
    constexpr int O_T = O_EN + 1, O_SH = O_T + (SPLIT ? NB : 0), NU = O_T + (WFILL ? NWIN + NSH : 0);
    float eo[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) eo[j] = en[decltype(ES)::value][j];
    float acc[NB], src[NB], wl[NB][WW], tv[NB][WW], sh[5 * NB];
    float cs = 0.f, scale = 1.f;
    const float* wsrc = KIND == kFbBeta ? ybuf + ((q - 1) & 1) * NP : row;
    // window term n: (k, j) in the order of the plain loops (k ascending for every j).
    // FB, window sum from 0 (WFILL): term k = 0 is the product v * w, the later ones fmas into it.
    // fma(v, w, +0) and v * w are the same bits unless the product is -0 (-0 + +0 = +0), and none
    // is: chain values, the zero a lane shift fills in at the wave edge and window weights are all
    // >= +0.  The multiply is VOP2, so a shifted first term is one v_mul_f32_dpp; the fma from 0
    // is VOP3, which has no DPP form, and left its shift a v_mov_b32_dpp of its own.
    auto term = [&](int n) {
      const int j = LW ? n / WW : n % NB, k = LW ? n % WW : n / NB;
      float v;
      if constexpr (LW) v = wl[j][k];
      else v = (SPLIT && k > 0 && win_term_shifted(n, NB, TD0)) ? sh[win_term_src(n, NB, TD0) - 2 * NB] : at(src, j, TD0 + k);
      if (FB) {
        if (WFILL && k == 0) {
#pragma clang fp contract(off)
          acc[j] = v * wv[j][k];
        } else {
          acc[j] = fmaf(v, wv[j][k], acc[j]);
        }
      } else {
        tv[j][k] = v + wv[j][k];
      }
    };
    // the m-th lane shift behind a first term: the fmac that reads it cannot take it in (the DPP
    // combiner runs while it is still an fma), so it is a v_mov_b32_dpp wherever it stands
    auto shift = [&](int m) {
      const int n = win_shift_term(m, NB, NWIN, TD0);
      float& s = sh[win_term_src(n, NB, TD0) - 2 * NB];  // (by source: a second reader takes it from here)
      s = at(src, n % NB, TD0 + n / NB);
      fill_pin(s);
    };
    auto unit = [&](auto I) {
      constexpr int i = decltype(I)::value;
      if constexpr (i == 0) {
        // row q-1: flushed by the helpers, window source in LDS mode (beta: the products)
        if (LW && KIND == kFbBeta) st(ybuf + ((q - 1) & 1) * NP + NB * l, src);
        else st(row + NB * l, y);
      } else if constexpr (i < O_ST2) {
        wl[(i - O_LD) / WW][(i - O_LD) % WW] = wsrc[lo[(i - O_LD) / WW] + (i - O_LD) % WW];
      } else if constexpr (i < O_EN) {
        st(row + NB * l, y);
      } else if constexpr (i == O_EN) {
        // (diagnostic timing bit, wrong results: kBandEmisReg no read, the block's first row stays)
        if constexpr (!(kAbl & abl::kBandEmisReg)) {
          if (!no_read) ld(enext, en[decltype(ES)::value]);
        }
      } else if constexpr (i < O_SH) {
        term(i - O_T);  // (SPLIT) the first terms
      } else if constexpr (i < O_SH + NSH) {
        shift(i - O_SH);
      } else {
        term(i - O_T - NSH);
      }
    };
    auto fill = [&](auto G) {
      static_for<fill_lo(decltype(G)::value, NU, RF), fill_lo(decltype(G)::value + 1, NU, RF)>(unit);
      if constexpr (decltype(PW)::value && decltype(G)::value == emis_wait_gap(RF) && !(kAbl & abl::kBandEmisReg))
        pin_all(en[EA - 1 - decltype(ES)::value]);
    };
    // (diagnostic timing bits, wrong results: kBandNoReduce no reduction, kBandReducePrev the
    // reduction of the previous step's values, off the step's dependency chain)
    auto reduce = [&](auto MAXOP, float t) -> float {
      if constexpr (kAbl & abl::kBandNoReduce) {
        static_for<0, NU>(unit);
        return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t)));
      } else if constexpr (!FILLED) {
        static_for<0, NU>(unit);
        return decltype(MAXOP)::value ? wave_max_bcast<RF>(t) : wave_sum_bcast<RF>(t);
      } else if constexpr (decltype(MAXOP)::value && (kAbl & abl::kBandReducePrev)) {
        const float r = wave_red_fill<true, RF>(gprev, fill);
        gprev = t;
        return r;
      } else {
        return wave_red_fill<decltype(MAXOP)::value, RF>(t, fill);
      }
    };
    if (KIND == kFbBeta) {  // the product input is y = v * e_{q-1} (hmm.py:113-115)
      prods<NB>(y, eo, src);
      const float t = prod_sum<NB, kSumFirst || decltype(RL)::value>(y, eo, src);
      // the floor term fl_j * c is folded into the end: y_j = fl_j + (window sum) / c, one fma
      // after the reduction instead of a multiply before the window fmas and one after
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[j] = 0.f;
      cs = reduce(std::false_type{}, t);
    } else if (KIND == kFbAlpha) {
#pragma unroll
      for (int j = 0; j < NB; ++j) src[j] = y[j];
      float t;
      if constexpr (decltype(FP)::value) t = prod_sum<NB, kSumFirst>(pp, ee, y);
      else t = plain_sum<NB>(y);
      if constexpr (decltype(UA)::value) {
        // uniform floor: folded into the end as for beta, y = (afl0 + wsum / c) e
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = 0.f;
        cs = reduce(std::false_type{}, t);
      } else {
        float tw = 0.f;
#pragma unroll
        for (int j = 0; j < NB; ++j) tw = fmaf(y[j], fl[j], tw);
        cs = reduce(std::false_type{}, t);
        tw = wave_sum_bcast<RF>(tw);
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = tw;
      }
    } else {
      float g = -INFINITY;
#pragma unroll
      for (int j = 0; j < NB; ++j) { src[j] = y[j]; g = fmaxf(g, y[j] + fl[j]); }
      const float M = reduce(std::true_type{}, g);
      // fused psi: M_q = max_i fl(delta_{q-1,i} + r_i) is also psi row q's floor maximum
      if constexpr (FUSE) wlane(blk, M);
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[j] = M;
    }
    if (FB) {
      scale = __builtin_amdgcn_rcpf(cs);
      wlane(blk, cs);  // c_{q-1}
    }
    if constexpr (!WFILL) {
      static_for<0, NWIN>([&](auto I) { term(decltype(I)::value); });
    } else if constexpr (!FB) {
#pragma unroll
      for (int n = 0; n < NWIN; ++n) {
        const int j = LW ? n / WW : n % NB, k = LW ? n % WW : n / NB;
        acc[j] = fmaxf(acc[j], tv[j][k]);
      }
    }
    if constexpr (KIND == kFbAlpha) {
      // y_j = pp_j * ee_j (padded states: the staged emission is 0)
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if constexpr (decltype(UA)::value) { pp[j] = fmaf(acc[j], scale, afl0); ee[j] = eo[j]; }
        else { pp[j] = acc[j]; ee[j] = scale * eo[j]; }
      }
      prods<NB>(pp, ee, y);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      // padded states: the staged emission is 0 (FB) / -inf (Viterbi) and the floors 0
      if (KIND == kFbAlpha) continue;
      if (KIND == kFbBeta) {
        y[j] = fmaf(acc[j], scale, fl[j]);
      } else {
        y[j] = acc[j] + eo[j];
      }
    }
  };

  // (diagnostic builds: cycles at the block barriers, the whole chain, and its real time)
  // (the whole blocks by part: st_steady from the top of step 1 to behind step 15, st_edge the
  // rest -- step 0 and whatever stands between two blocks; st_bar_in: the barrier wait that
  // falls into steps 1 .. 15)
  unsigned long long st_bar = 0, st_t0 = 0, st_steady = 0, st_edge = 0, st_nsteady = 0, st_nedge = 0, st_bar_in = 0;
  long long rt0 = 0;
  if (kStamp) { st_t0 = stamp(); rt0 = __builtin_amdgcn_s_memrealtime(); }
  // (HMM355_STAMP_BAR=0: no stamps round the block barrier, whose pair stands inside steps 1 .. 15
  // of the round-12 loop and costs them a stamp's latency; the barrier's wait is then in the part
  // it stands in)
  auto block_barrier = [&]() {
    unsigned long long sb = 0;
    if (kStamp && kStampBar) sb = stamp();
    if (!(kAbl & abl::kBandNoBlockBarrier)) lds_barrier();
    if (kStamp && kStampBar) st_bar += stamp() - sb;
  };
  auto run_blocks = [&](auto UA) {
    unsigned long long s15 = 0;
    for (int kb = 0; kb < nblocks; ++kb) {
      const int q0 = kb * 16 < 1 ? 1 : kb * 16;
      const int q1 = (kb + 1) * 16 < T ? (kb + 1) * 16 : T;
      if (q0 < q1) ld(erow(q0 - EL), en[0]);
      // step jj of this block writes row 16kb + jj - 1: slot (16kb & 63) + jj - 1 for jj >= 1
      // (no wrap inside a block), slot (16kb - 1) & 63 for jj = 0; it loads the emission row
      // of step 16kb + jj + EA - EL (the rolled loop: + 1), slot (kb % 3) * 16 + jj + EA - EL of
      // the staging ring.  The rows of steps 1 .. EA - 1 are read here, behind the barrier that
      // staged this block: no read crosses a block's edge (beta's step 0 takes its row from the
      // previous block's slot, staged a block ago, and it is read here too)
      float* rbase = lds + C::OFF_RING + ((16 * kb) & (C::RING - 1)) * NP;
      float* rwrap = lds + C::OFF_RING + ((16 * kb - 1) & (C::RING - 1)) * NP;
      const float* ebase = lds + C::OFF_EMIS + ((kb % 3) * 16 + 1 - EL) * NP + NB * l;
      float blk = 0.f;
      if (q0 == kb * 16 && q1 == kb * 16 + 16) {
        static_for<1, EA>([&](auto K) { ld(ebase + (decltype(K)::value - 1) * NP, en[decltype(K)::value]); });
        static_for<0, 16>([&](auto JJ) {
          constexpr int jj = decltype(JJ)::value;
          if (kStamp && jj == 1) {
            const unsigned long long s1 = stamp();
            if (s15) { st_edge += s1 - s15; ++st_nedge; }
            s15 = s1;
          }
          step(kb * 16 + jj, jj, jj + EA > 15, UA, std::bool_constant<(jj > 0)>{}, std::bool_constant<(jj == 0)>{},
               std::integral_constant<int, jj % EA>{}, std::bool_constant<(EA == 2 && KIND != kFbAlpha && jj < 15)>{},
               jj == 0 ? rwrap : rbase + (jj - 1) * NP, ebase + (jj + EA - 1) * NP, blk,
               [](float& d, float v) { writelane_c<jj>(d, v); });
        });
        if (kStamp) {
          const unsigned long long t = stamp();
          st_steady += t - s15; ++st_nsteady;
          s15 = t;
        }
        // the block's normalisers / floor maxima: lane jj -> row 16kb + jj - 1 (entry 0 of its
        // 64-float slot, where rec_ls_scan / the psi waves / fbpair's scan read it)
        if constexpr (FB || FUSE) {
          if (l < 16) lds[C::OFF_SC + 64 * ((16 * kb + l - 1) & (C::RING - 1))] = blk;
        }
      } else {
        // first and last (partial) blocks: one store per step, as it is computed
        for (int q = q0; q < q1; ++q) {
          const int jj = q - kb * 16;
          float* sc = lds + C::OFF_SC + 64 * ((q - 1) & (C::RING - 1));
          step(q, jj, q + 1 == q1, UA, std::false_type{}, std::true_type{}, std::integral_constant<int, 0>{}, std::false_type{},
               jj == 0 ? rwrap : rbase + (jj - 1) * NP, ebase + jj * NP, blk,
               [sc](float&, float v) { *sc = v; });
        }
      }
      block_barrier();  // B_{kb+1}: block kb+1 staged by the helpers, rows of block kb-1 written
    }
  };
  // The same blocks with a hot loop that holds only whole ones (EDGE).
  // Block 0 (no step 0) and a partial last block run rolled: one step at a time, each storing its
  // normaliser word as it is computed, the block barrier behind the last.  The whole blocks 1 ..
  // T / 16 - 1 run in a loop that tests its trip count and nothing else:
  //  - its bases (emission slot, the next block's, row-ring slot, the wrapped row, the normaliser
  //    word) advance by an add and a wrap each; no % 3, no multiply, no q0 / q1;
  //  - the emission rotation runs on across the edge: step jj reads the row of step jj + EA, and
  //    where that is a step of block kb + 1 it reads that block's slot, so a block starts with its
  //    first EA rows in registers (beta's step 0 takes row 15 of the block before: still this
  //    block's slot).  For that the wave meets its block barrier B_{kb+1} (block kb + 1 staged)
  //    behind step 15 - EA, at the end of that step, when the step's own LDS operations have long
  //    completed, and not behind step 15.  The helpers' and psi waves' barriers stand where they
  //    stood: every wave still meets one barrier a block.
  //    Why the two (EA) steps behind the barrier are safe:
  //     * they write rows 16kb + 15 - EA .. 16kb + 14 and, behind step 15, the block's normaliser
  //       words (rows 16kb - 1 .. 16kb + 14).  Whoever reads them works two blocks behind: the
  //       helpers' block_work(k), between B_k and B_{k+1}, scans and flushes block k - 2
  //       (rec_ls_scan: words 16(k-2) - 1 .. + 14; rec_flush: rows 16(k-2) .. + 15, the last of them
  //       written by step 0 of block k - 1), the psi waves read rows and words 16(k-2) - 1 .. + 14.
  //       Block kb's are read behind B_{kb+2}, which this wave meets a block later; the 64-row
  //       rings hold four blocks, so what these steps overwrite is block kb - 4's, read behind
  //       B_{kb-2};
  //     * they read slot kb % 3 and slot (kb + 1) % 3 of the staging ring.  Behind B_{kb+1} the
  //       helpers stage block kb + 2 into slot (kb + 2) % 3, which held block kb - 1: this wave
  //       read its last row of it (beta's step 0 of block kb) a block ago.
  //    Behind the last whole block the rows read across the edge are a partial block's (it reads
  //    its own first row again behind its barrier) or the padding the helpers stage past the end:
  //    inside the ring either way, and not used;
  //  - every lane stores the block's normaliser register: lane jj < 16 to entry 0 of row
  //    16kb + jj - 1's 64-word slot, as before, lanes 16 .. 63 to entries 1 .. 3 of the same slots,
  //    which nobody reads.  One add and one and per block, no exec mask.
  // Step 0's arithmetic (RL, plain_sum, rwrap) is what it was.
  auto run_edge = [&](auto UA) {
    auto rolled = [&](int kb, int q0, int q1) {
      if (q0 < q1) ld(erow(q0 - EL), en[0]);
      float* rbase = lds + C::OFF_RING + ((16 * kb) & (C::RING - 1)) * NP;
      float* rwrap = lds + C::OFF_RING + ((16 * kb - 1) & (C::RING - 1)) * NP;
      const float* ebase = lds + C::OFF_EMIS + ((kb % 3) * 16 + 1 - EL) * NP + NB * l;
      float none = 0.f;
      for (int q = q0; q < q1; ++q) {
        const int jj = q - kb * 16;
        float* sc = lds + C::OFF_SC + 64 * ((q - 1) & (C::RING - 1));
        step(q, jj, q + 1 == q1, UA, std::false_type{}, std::true_type{}, std::integral_constant<int, 0>{}, std::false_type{},
             jj == 0 ? rwrap : rbase + (jj - 1) * NP, ebase + jj * NP, none,
             [sc](float&, float v) { *sc = v; });
      }
      block_barrier();
    };
    rolled(0, 1, T < 16 ? T : 16);
    const int nfull = T / 16 - 1;  // whole blocks behind block 0
    if (nfull > 0) {
      // (behind B_1: block 1 is staged; the only rows of a whole block read at its top)
      static_for<0, EA>([&](auto K) { ld(erow(16 + decltype(K)::value - EL), en[decltype(K)::value]); });
      int es = 16 * NP, rb = 16 * NP;  // block 1's staging slot and first row, in floats
      int scw = 64 * ((15 + (l & 15)) & (C::RING - 1)) + (l >> 4);
      float blk = 0.f;
      unsigned long long s15 = 0;
      for (int kb = 1; kb <= nfull; ++kb) {
        const int esn = es == 32 * NP ? 0 : es + 16 * NP;
        float* rbase = lds + C::OFF_RING + rb;
        float* rwrap = lds + C::OFF_RING + ((rb - NP) & (C::RING * NP - 1));
        const float* ebase = lds + C::OFF_EMIS + es + (1 - EL) * NP + NB * l;
        const float* nbase = lds + C::OFF_EMIS + esn + NB * l;
        static_for<0, 16>([&](auto JJ) {
          constexpr int jj = decltype(JJ)::value;
          constexpr int p = jj + EA - EL;  // the row this step reads, counted from the block's slot
          if (kStamp && jj == 1) {
            const unsigned long long s1 = stamp();
            if (s15) { st_edge += s1 - s15; ++st_nedge; }
            s15 = s1;
          }
          step(kb * 16 + jj, jj, false, UA, std::bool_constant<(jj > 0)>{}, std::bool_constant<(jj == 0)>{},
               std::integral_constant<int, jj % EA>{}, std::bool_constant<(EA == 2 && KIND != kFbAlpha)>{},
               jj == 0 ? rwrap : rbase + (jj - 1) * NP, p < 16 ? ebase + (jj + EA - 1) * NP : nbase + (p - 16) * NP, blk,
               [](float& d, float v) { writelane_c<jj>(d, v); });
          if constexpr (jj == 15 - EA) {  // B_{kb+1}
            const unsigned long long b0 = st_bar;
            block_barrier();
            st_bar_in += st_bar - b0;
          }
        });
        if (kStamp) {
          const unsigned long long t = stamp();
          st_steady += t - s15; ++st_nsteady;
          s15 = t;
        }
        if constexpr (FB || FUSE) {
          lds[C::OFF_SC + scw] = blk;
          scw = (scw + 16 * 64) & (C::RING * 64 - 1);
        }
        es = esn;
        rb = (rb + 16 * NP) & (C::RING * NP - 1);
      }
    }
    if (T > 16 && (T & 15)) rolled(T / 16, T & ~15, T);
  };
  auto run = [&](auto UA) {
    if constexpr (EDGE) run_edge(UA);
    else run_blocks(UA);
  };
  if constexpr (KIND == kFbAlpha) {
    if (uafl) run(std::true_type{});
    else run(std::false_type{});
  } else {
    run(std::false_type{});
  }
  if (kStamp && l == 0) {
    const unsigned long long t1 = stamp();
    const long long rt1 = __builtin_amdgcn_s_memrealtime();
    unsigned long long* o8 = g_rec_stamps + ((size_t)blockIdx.x * 16 % kStampWaves) * 8;
    o8[0] = (unsigned long long)rt0; o8[1] = (unsigned long long)rt1; o8[3] = st_bar;
    o8[4] = T; o8[5] = t1 - st_t0; o8[6] = t1 - st_t0; o8[7] = (unsigned long long)(rt1 - rt0);
    // the whole blocks by part, in the record of wave 4 (which has ended): steps 1 .. 15, their
    // count, the rest (step 0 and the edge), its count, the barrier wait inside steps 1 .. 15
    unsigned long long* e8 = g_rec_stamps + (((size_t)blockIdx.x * 16 + 4) % kStampWaves) * 8;
    e8[0] = st_steady; e8[1] = st_nsteady; e8[2] = st_edge; e8[3] = st_nedge; e8[4] = st_bar_in;
  }
  float* row = lds + C::OFF_RING + ((T - 1) & (C::RING - 1)) * NP;
  st(row + NB * l, y);
  if (KIND == kFbAlpha && a.loglik) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < NB; ++j) t += y[j];
    rec_keep_c_last<NP>(lds, T, t);
  }
  lds_barrier();
}

// ---------------------------------------------------------------------------------------
// Banded chain (band.h).  Wave 0 runs the whole recursion; lane l owns states
// s = 64*blk + l.  Per step: the previous row goes to the LDS ring (it is both the window
// source and the row that is flushed), one DPP wave reduction (sum / weighted sum / max)
// runs beside the W window reads, then W fma / add+max per state.  No s_barrier inside the
// 16-step block: LDS accesses of one wave complete in order.  Waves 1..NW-1 are helpers:
// during block kb they stage the emissions of block kb+1 (log / +1e-8 transform included),
// issue the global loads of block kb+3 and flush the rows and log-scales of block kb-2, so
// the chain wave issues no global memory operation and no transcendental of the staging.
// All waves meet at one s_barrier per 16 steps.
template <int NP, int KIND, int WP, int TD0 = 0, int TW = 0>
__device__ __forceinline__ void rec_band(const RecArgs& a, float* lds, int b, const BandDesc* __restrict__ d) {
  using C = RC<NP>;
  constexpr int NB = C::NBLK;
  // Waves 1..3 are the helpers (forward-backward); waves 4.. exit at once, so the chain wave
  // is alone on its SIMD (a workgroup's waves are spread over the 4 SIMDs).  Ended waves do
  // not take part in s_barrier.
  // The Viterbi staging also takes the emission log (logcr.h), so it runs on a fourth helper,
  // wave 4, beside the chain on SIMD 0: measured alone, 3 helpers 259 us, 4 helpers 238 us,
  // the separate log pass 248 us (B=32, T=2000, N=128); 3 of the 8 virtual waves on wave 4
  // and 5 on waves 1..3 was slower (262 us).
  // Round 3, fused-psi Viterbi (kVitFused, NP >= 128): the workgroup has 16 waves (kVitWideNT).
  // With the chain's step down to ~95 ns its helpers had become the limit (one process,
  // B=32 T=2000 N=128: Viterbi op 242 us; without the emission log 209, without the psi rows
  // 195, neither 189; tools/ablate.py, profiles/r3g_ablate.log), so SIMDs 1..3 each carry
  // TWO staging helpers (waves 1,2,3 and 9,10,11) and TWO psi waves (5,6,7 and 13,14,15), and
  // nothing shares the chain's SIMD: waves 4, 8, 12 (w = 0 mod 4, the chain's SIMD) exit.
  // Round 6, forward-backward (FBW): every wave of the launch off the chain's SIMD stages
  // (waves 1,2,3, 5,6,7, 9,10,11 of kFbNT<128>: one virtual staging wave each).  With three
  // helpers of three virtual waves, helper 1's block work took ~3.4 k cycles, the chain's 16
  // steps ~3.2 k, and the chains waited 18 (beta) / 28 (alpha) cycles a step at the block
  // barrier (tools/band_stamps.py).
  constexpr bool FUSE = KIND == kVit && kVitFused<NP>;
  constexpr bool WIDE = FUSE;
  constexpr bool FBW = KIND != kVit;
  constexpr int NWB = kFbNT<NP> / kWave;  // (FBW) the launch's waves
  constexpr int NH = WIDE ? 6 : FBW ? (NWB / 4) * 3 + (NWB % 4 > 1 ? NWB % 4 - 1 : 0)
                                    : ((KIND == kVit && C::NW >= 8) ? 4 : 3);  // (NP = 64: a 4-wave workgroup)
  constexpr int HV = (C::NW + NH - 1) / NH;  // virtual staging waves per helper
  const int tid = threadIdx.x;
  const int w = tid >> 6, l = tid & 63;
  // role of wave w: staging helper index hi (0 .. NH-1), psi wave index, or neither (exit)
  const int grp = (w >> 3) * 3 + (w & 3) - 1;  // WIDE: waves 1,2,3 / 5,6,7 -> 0,1,2; 9,.. / 13,.. -> 3,4,5
  const bool stager = WIDE ? ((w & 4) == 0 && (w & 3) != 0) : FBW ? (w & 3) != 0 : (w > 0 && w <= NH);
  const bool psiw = WIDE && (w & 4) != 0 && (w & 3) != 0;
  const int hi = WIDE ? grp : FBW ? (w >> 2) * 3 + (w & 3) - 1 : w - 1;
  auto vw_of = [&](int h) -> int { return hi + h * NH; };  // virtual staging wave h of this helper
  constexpr bool FB = KIND != kVit;
  if (w != 0 && !stager && !psiw) return;  // ended waves take no part in s_barrier
  const int T = a.T, N = a.N;
  const int nblocks = (T + 15) / 16;
  double base = (KIND == kFbBeta && a.bscale) ? (double)a.bscale[b] : 0.0;

  // prologue: the helpers stage block 0 and load blocks 1 and 2
  // three register sets: the loads of block kb+3 are issued during block kb, so each has two
  // blocks (~3 us) to land before it is staged
  float er0[HV][5], er1[HV][5], er2[HV][5];
  if (stager) {
    if (KIND == kVit) rec_logt_fill<NP>(lds, l);
#pragma unroll
    for (int h = 0; h < HV; ++h) {
      const int vw = vw_of(h);
      if (vw < C::NW) {
        float er[5];
        rec_load<NP, KIND>(a, b, 0, vw, l, er);
        rec_stage<NP, KIND, FUSE>(a, lds, 0, vw, l, er);
        if (nblocks > 1) rec_load<NP, KIND>(a, b, 1, vw, l, er1[h]);
        if (nblocks > 2) rec_load<NP, KIND>(a, b, 2, vw, l, er2[h]);
      }
    }
  }
  lds_barrier();

  if (w == 0) {
    band_chain<NP, KIND, WP, TD0, TW, emis_ahead(KIND), true>(a, lds, b, d);
    return;
  }
  // ---------------------------------------------------------------- helper waves
  // Fused psi (vit_psi_kernel's banded rule, psi_band_rows in viterbi.hip), on the
  // psi-only waves 5..7 and 13..15 (SIMDs 1..3, so neither the chain nor the staging helpers
  // lose issue slots).  With g_i = fl(delta_{t-1,i} + r_i) and M = max g (the chain's own floor
  // term, left in LDS), i1 = first index with g_i == M is a ballot + s_ff1, and psi_t[o] is the
  // first index attaining max(M, window values), i1 when M attains it.  The window is the
  // chain's: Toeplitz offsets TD0.. (TW > 0) or the column windows clo_o .. clo_o + WP.
  // Lane l owns outputs o = NB*l + j.  Rows r == grp (mod 6) of the block; a wave's rows are
  // computed without branches so their latencies overlap.  The rows go to the LDS ring OFF_PSR
  // (the last 64 steps); the staging helpers copy each block of them to HBM (psi_copy).
    constexpr int PWN = TW > 0 ? TW : WP;  // window slots per output
    [[maybe_unused]] float prf[NB];
    [[maybe_unused]] int plo[NB];
    [[maybe_unused]] float pcl[NB][PWN];
    if constexpr (FUSE) {
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int o = NB * l + j;
        prf[j] = o < N ? d->rfl[o] : -INFINITY;  // -inf: padded states never attain M
        plo[j] = TW > 0 ? o + TD0 : d->clo[o];
#pragma unroll
        for (int kk = 0; kk < PWN; ++kk) {
          const int i = plo[j] + kk;
          pcl[j][kk] = (i >= 0 && i < N && o < N) ? (TW > 0 ? d->tL[o][kk] : d->cL[o][kk]) : -INFINITY;
        }
      }
      // resolve the table loads here, once: left pending, the waitcnt pass would re-wait for
      // them inside the loop with a vmcnt that also drains in-flight memory operations
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        keep(prf[j]);
        keep(plo[j]);
#pragma unroll
        for (int kk = 0; kk < PWN; ++kk) keep(pcl[j][kk]);
      }
    }
    auto psi_rows = [&](int bk) {
      if constexpr (FUSE) {
        if (bk < 0 || (kAbl & abl::kNoPsiRows)) return;
        constexpr int NPW = WIDE ? 6 : 3, PR = (16 + NPW - 1) / NPW;
        const int hw = grp;
#pragma unroll
        for (int m = 0; m < PR; ++m) {
          const int r = hw + NPW * m;
          int t = 16 * bk + (r < 16 ? r : 15);
          t = t < T ? t : T - 1;
          const int rho = (t - 1) & (C::RING - 1);
          const float* drow = lds + C::OFF_RING + rho * NP;
          // no guards around the LDS reads (out-of-range slots carry -inf in prf / pcl): a
          // read under a guard ends in an s_waitcnt vmcnt(0) join
          float yv[NB], xw[NB][PWN];
          if constexpr (NB == 2) {
            const float2 v2 = *reinterpret_cast<const float2*>(drow + NB * l);
            yv[0] = v2.x; yv[1] = v2.y;
          } else {
            const float4 v4 = *reinterpret_cast<const float4*>(drow + NB * l);
            yv[0] = v4.x; yv[1] = v4.y; yv[2] = v4.z; yv[3] = v4.w;
          }
          const float M = lds[C::OFF_SC + 64 * rho];  // the chain's floor maximum of row rho (broadcast read)
#pragma unroll
          for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int kk = 0; kk < PWN; ++kk) {
              const int i = plo[j] + kk;
              xw[j][kk] = drow[i < 0 ? 0 : (i < NP ? i : NP - 1)];
            }
          int i1 = 0x7fffffff;
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const float g = yv[j] + prf[j];
            const unsigned long long hit = __ballot(g == M);
            const int c = NB * (__ffsll((long long)hit) - 1) + j;
            i1 = (hit && c < i1) ? c : i1;
          }
          unsigned pk = 0;
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            float v = M, val[PWN];
#pragma unroll
            for (int kk = 0; kk < PWN; ++kk) {
              val[kk] = xw[j][kk] + pcl[j][kk];  // -inf outside [0, N)
              v = fmaxf(v, val[kk]);
            }
            int arg = M == v ? i1 : 0x7fffffff;
#pragma unroll
            for (int kk = 0; kk < PWN; ++kk)
              if (val[kk] == v && plo[j] + kk < arg) arg = plo[j] + kk;
            arg = (NB * l + j < N && t > 0) ? arg : 0;  // psi_0 = 0 (hmm.py:156 zeros)
            pk |= (unsigned)arg << (8 * j);
          }
          if (r < 16 && 16 * bk + r < T) {
            // the LDS ring of the last 64 rows; the staging helpers copy whole blocks of it to
            // HBM with 16-B stores (psi_copy)
            uint8_t* ldst = reinterpret_cast<uint8_t*>(lds + C::OFF_PSR) + (t & (C::PSR - 1)) * NP + NB * l;
            if constexpr (NB == 2) *reinterpret_cast<uint16_t*>(ldst) = (uint16_t)pk;
            else *reinterpret_cast<uint32_t*>(ldst) = pk;
          }
        }
      }
    };
    // Publishing (a.pub, follow.h): the flushes of the rows (FB: U / V, Viterbi: delta) and the
    // copies of the psi rows are write-through stores, and a wave's vector-memory counter retires
    // in issue order, so the compiler's wait for a register set's loads at its staging also
    // retires every store issued before those loads.  The loads of block k + 4 are issued in
    // block_work(k + 1), after block_work(k)'s flush of block k - 2 and psi copy of block k - 3, and
    // they are staged (waited for) in block_work(k + 3): after the barrier that ends it those
    // stores are complete in every helper, and in block_work(k + 4) one lane publishes the count.
    // (The stores are never waited for sooner: a write-through store retires late, and a helper
    // stalled on it stalls the chain at the next barrier.)
    const bool pubon = a.pub != nullptr;
    int* const pubp = pubon ? a.pub + (FB ? 2 * b + (KIND == kFbBeta) : b) * kPubStride : nullptr;
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t psi_rs =
        FUSE ? make_rsrc(a.psi + (size_t)b * T * NP, (size_t)T * NP) : make_rsrc(a.obs, 0);
    // copy the 16 psi rows of block bk from the LDS ring to HBM, one 16-B sc1 store per lane
    // (the last helpers' lanes: 16 * NP / 16 of them)
    [[maybe_unused]] auto psi_copy = [&](int bk) {
      if constexpr (FUSE) {
        constexpr int PER = NP / 16;  // 16-B pieces per row
        const int hidx = (NH - 1 - hi) * 64 + l;
        const int r = hidx / PER, pc = hidx % PER;
        const int t = 16 * bk + r;
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const uint8_t*>(lds + C::OFF_PSR) +
                                                            (t & (C::PSR - 1)) * NP + 16 * pc);
        if (bk >= 0 && hidx < 16 * PER && t < T)
          __builtin_amdgcn_raw_buffer_store_b128(v, psi_rs, t * NP + 16 * pc, 0, (kFAbl & fabl::kPlainStores) ? 0 : kAuxSc1);
      }
    };
    // Straight-line block work (no branch around the staging or the loads: the tail stages
    // a block past the end as padding and re-loads the last block), so the waitcnt pass
    // keeps exact counts and never drains the in-flight prefetches or the flush stores.
    // Viterbi with log leaders: `lp` holds the leaders' count word as polled three blocks ago, and
    // takes this block's poll.  The word is kept as loaded and decoded (poll_count's rule) only
    // where it is read, three blocks on, where the staging's wait has already retired that poll.
    // Decoded where it was polled -- as it stood until round 9 -- the compiler waited for the
    // load on the spot with vmcnt(0), which also drains the write-through flush and psi stores
    // issued just before it: ~800 of a block's ~2900 cycles in every staging helper (stamps by
    // item), and the chain waited for its helpers.  The poll is a
    // buffer load (sc1, as the atomic load was) so that it needs no branch: without leaders the
    // resource is empty and the load returns 0, which decodes to count 0.
    const bool lpon = KIND == kVit && a.lready;
    const __amdgpu_buffer_rsrc_t lp_rs =
        make_rsrc(lpon ? static_cast<const void*>(a.lready + b * kPubStride) : static_cast<const void*>(a.obs), lpon ? 8 : 0);
    auto lp_count = [&](const u32x2_t& v) -> int {
      const unsigned lo = __builtin_amdgcn_readfirstlane(v[0]), hi32 = __builtin_amdgcn_readfirstlane(v[1]);
      const unsigned c = lo ^ count_mix(a.token);
      return (hi32 == a.token && c <= (unsigned)nblocks) ? (int)c : 0;
    };
    // (diagnostic builds: a helper's cycles of block work and at the barrier)
    // (hs_item: the work by item -- staging and loads | row flush | psi copy | polls and publish;
    // the log-scale scan is in the whole but in no item)
    unsigned long long hs_work = 0, hs_wait = 0, hs_item[4] = {0, 0, 0, 0};
    // Forward-backward end rows (post.h kEndBlocks): the rows of the chain's last two blocks are
    // still in the LDS ring when the chain ends, and were they left to the followers they would
    // be flushed, published, seen by a polling lane and read back before their posterior could
    // be formed.  The helpers form it here instead, helper hi rows hi, hi + NH .. of the two
    // blocks, in the followers' lane layout with the followers' function (post_row_lanes): the
    // own row from the ring (the values rec_flush stores), the partner chain's row -- written
    // near that chain's start -- by sc1 loads issued while the chain runs its last block
    // (end_load: the helpers only wait for the last barrier then), behind ONE poll of the
    // partner's count.  Rows whose partner rows were not counted (a partner dispatched late) or
    // that kEndsOddLeft names are left to the followers: the helper's bits go to its left-over
    // word in LDS and helper 0 publishes the union right after the last barrier (follow.h reads
    // it).  The chain workgroup polls once and never spins.
    constexpr int KL = NP / 64;                               // states per lane in the followers' layout
    constexpr int RE = (16 * kEndBlocks + NH - 1) / NH;       // end rows per helper
    [[maybe_unused]] float epr[RE][KL];
    [[maybe_unused]] int eok = 0;
    const bool endson = FB && stager && pubon && (a.ends & kEndsOn) && a.prow && a.post;
    const int qend0 = 16 * (nblocks - kEndBlocks);            // the first end row (chain order)
    // end row m of this helper: chain row q, live when it exists
    auto end_row = [&](int m, int& q) -> bool {
      q = qend0 + hi + NH * m;
      return q < T;
    };
    [[maybe_unused]] auto end_load = [&]() {
      if constexpr (FB) {
        const int* ppub = a.pub + (2 * b + (KIND == kFbAlpha)) * kPubStride;
        const int cnt = __builtin_amdgcn_readfirstlane(poll_count(ppub, a.token, nblocks + 1));
        // (the partner's rows of times tau(q), q >= qend0, are its own rows < T - qend0)
        const bool counted = cnt > nblocks || 16 * cnt >= T - qend0;
        int leftmask = 0;
#pragma unroll
        for (int m = 0; m < RE; ++m) {
          int q;
          const bool live = end_row(m, q);
          const bool ok = counted && !((a.ends & kEndsOddLeft) && ((q >> 4) & 1));
          eok |= (int)ok << m;
          if (live && !ok) leftmask |= 1 << (nblocks - 1 - (q >> 4));
          int tq = live ? rec_tau<KIND>(q, T) : 0;
          asm volatile("" : "+v"(tq) : "s"(cnt));  // (the loads stay behind the count's poll)
          post_row_load<KL>(make_rsrc(a.prow + (size_t)b * T * NP, (size_t)T * NP * 4), tq, l, epr[m]);
        }
        if (l == 0) reinterpret_cast<int*>(lds + C::OFF_LEFT)[hi] = leftmask;
      }
    };
    [[maybe_unused]] auto end_post = [&]() {
      if constexpr (FB) {
        const bool endvec = N == NP && (reinterpret_cast<uintptr_t>(a.post) % (4 * KL)) == 0;
#pragma unroll
        for (int m = 0; m < RE; ++m) {
          int q;
          const bool on = end_row(m, q) && ((eok >> m) & 1);
          const int tq = on ? rec_tau<KIND>(q, T) : 0;
          float own[KL];
          const float* rp = lds + C::OFF_RING + (q & (C::RING - 1)) * NP + KL * l;  // (unconditional read)
          if constexpr (KL == 1) {
            own[0] = rp[0];
          } else if constexpr (KL == 2) {
            const float2 y = *reinterpret_cast<const float2*>(rp);
            own[0] = y.x; own[1] = y.y;
          } else {
            const float4 y = *reinterpret_cast<const float4*>(rp);
            own[0] = y.x; own[1] = y.y; own[2] = y.z; own[3] = y.w;
          }
          float* dst = a.post + ((size_t)b * T + tq) * N;
          if (KIND == kFbAlpha) post_row_lanes<KL>(own, epr[m], dst, N, l, endvec, on);
          else post_row_lanes<KL>(epr[m], own, dst, N, l, endvec, on);
        }
      }
    };
    auto block_work = [&](int kb, float(&ernext)[HV][5], float(&erfree)[HV][5], u32x2_t& lp, auto FULLC) {
      asm volatile("" ::: "memory");  // (block_work(kb - 1)'s stores stay ahead of this block's loads)
      unsigned long long hs0 = 0;
      if (kStamp) hs0 = stamp();
      const int kload = kb + 3 < nblocks ? kb + 3 : nblocks - 1;
      // the block's log-scales once per helper (its own base); helper 1 writes LA / LB
      float lsv = 0.f;
      if (!(kAbl & abl::kBandNoFlush) && kb >= 2) lsv = rec_ls_scan<NP, KIND>(a, lds, b, kb - 2, base, w == 1);
      // Viterbi: the block's source -- the leaders' log rows when they are ready, else the raw
      // emissions (the staging takes the log)
      const bool fromlog = KIND == kVit && a.lobuf && kload >= 4 && lp_count(lp) >= kload + 1;
      const float* src = fromlog ? a.lobuf : a.obs;
      const float vmode = (fromlog || a.obs_mode == HMM355_OBS_LOG) ? 1.f : 0.f;
      unsigned long long hi0 = hs0, hi1 = 0;  // (diagnostic builds: the block work by item)
#pragma unroll
      for (int h = 0; h < HV; ++h) {
        const int vw = vw_of(h);
        if (vw < C::NW && !(kAbl & abl::kBandNoHelperWork)) {
          if (!(kAbl & abl::kBandNoStage)) {
            rec_stage<NP, KIND, FUSE>(a, lds, kb + 1, vw, l, ernext[h]);
            rec_load<NP, KIND, decltype(FULLC)::value, FUSE>(a, b, kload, vw, l, erfree[h], src, vmode);
          }
          if (kStampItems) { hi1 = stamp(); hs_item[0] += hi1 - hi0; hi0 = hi1; }
          if (!(kAbl & abl::kBandNoFlush) && kb >= 2) rec_flush<NP, KIND>(a, lds, b, kb - 2, l + 64 * vw, lsv);
          if (kStampItems) { hi1 = stamp(); hs_item[1] += hi1 - hi0; hi0 = hi1; }
        }
      }
      psi_copy(kb - 3);
      if (kStampItems) { hi1 = stamp(); hs_item[2] += hi1 - hi0; hi0 = hi1; }
      if constexpr (KIND == kVit) lp = __builtin_amdgcn_raw_buffer_load_b64(lp_rs, 0, 0, kAuxSc1);
      // every fourth block (Viterbi: whole 64-step chunks of psi rows), after this block's loads
      // (so the stores it signals are never waited for sooner than three blocks on); with end
      // rows every block of the chain's last kLateBlocks, so that what the followers still have
      // to form when the chain ends is one pass of theirs, not two
      if (pubon && !(kFAbl & fabl::kNoBlockPublish) && hi == 0 && l == 0) {
        const int cnt = FB ? kb - 5 : kb - 6;
        const bool late = FB && (a.ends & kEndsOn) && kb >= nblocks - kLateBlocks;
        if (cnt > 0 && ((cnt & 3) == 0 || late)) publish_count(pubp, cnt, a.token);
      }
      unsigned long long hs1 = 0;
      if (kStamp) { hs1 = stamp(); hs_work += hs1 - hs0; hs_item[3] += kStampItems ? hs1 - hi0 : 0; }
      if (!(kAbl & abl::kBandNoBlockBarrier)) lds_barrier();
      if (kStamp) hs_wait += stamp() - hs1;
    };
    if constexpr (FUSE) {
      if (psiw) {  // psi-only waves: one compact loop, same barrier count as the helpers
        for (int kb = 0; kb < nblocks; ++kb) {
          unsigned long long ps0 = 0, ps1 = 0;
          if (kStampItems) ps0 = stamp();
          psi_rows(kb - 2);
          if (kStampItems) { ps1 = stamp(); hs_work += ps1 - ps0; }
          if (!(kAbl & abl::kBandNoBlockBarrier)) lds_barrier();
          if (kStampItems) hs_wait += stamp() - ps1;
        }
        if (kStampItems && l == 0) {
          unsigned long long* o8 = g_rec_stamps + (((size_t)blockIdx.x * 16 + w) % kStampWaves) * 8;
          o8[0] = hs_work; o8[1] = hs_wait; o8[4] = (unsigned long long)nblocks;
        }
        lds_barrier();  // the chain's last row
        psi_rows(nblocks - 2);
        psi_rows(nblocks - 1);
        lds_barrier();  // the last psi rows are in the ring (the helpers copy them)
        return;
      }
    }
    u32x2_t lp0 = {0u, 0u}, lp1 = lp0, lp2 = lp0;  // the leaders' polls (block kb's is read at kb + 3)
    auto helper_loop = [&](auto FULLC) {
      for (int kb = 0; kb < nblocks; kb += 3) {
        block_work(kb, er1, er0, lp0, FULLC);
        if (kb + 1 < nblocks) block_work(kb + 1, er2, er1, lp1, FULLC);
        if (kb + 2 < nblocks) block_work(kb + 2, er0, er2, lp2, FULLC);
      }
    };
    if (a.N == NP && (reinterpret_cast<uintptr_t>(a.obs) & 15) == 0 &&
        (!a.lobuf || (reinterpret_cast<uintptr_t>(a.lobuf) & 15) == 0))
      helper_loop(std::true_type{});
    else
      helper_loop(std::false_type{});
    if (kStamp && l == 0 && stager) {
      unsigned long long* o8 = g_rec_stamps + (((size_t)blockIdx.x * 16 + w) % kStampWaves) * 8;
      o8[0] = hs_work; o8[1] = hs_wait; o8[4] = (unsigned long long)nblocks;
      o8[3] = hs_item[0]; o8[5] = hs_item[1]; o8[6] = hs_item[2]; o8[7] = hs_item[3];
    }
    if (endson) end_load();  // (the chain runs its last block: the helpers only wait for it)
    lds_barrier();  // the chain's last row and c_{T-1}
    if (endson && hi == 0 && l == 0) {
      // every helper's left-over blocks were decided before the barrier: their union
      int m = 0;
      for (int h = 0; h < NH; ++h) m |= reinterpret_cast<const int*>(lds + C::OFF_LEFT)[h];
      publish_count(const_cast<int*>(pubp) + kLeftWord, m | (int)kLeftValid, a.token);
    }
    if constexpr (FUSE) {
      // The decode's end state (follow.h vit_decode_follow): the first arg-max of the last trellis
      // row, taken here from the LDS ring with the reduction and the state-to-lane mapping the
      // follower used (ties resolve as they did there), stored as the end word beside the count
      // (post.h kVitEndWord) well ahead of the final publish: the follower polls it with the
      // count and neither loads the row nor reduces it.
      if (pubon && hi == 0) {
        const float* dl = lds + C::OFF_RING + ((T - 1) & (C::RING - 1)) * NP;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < NP / 64; ++k) {
          const int j = l + 64 * k;
          const float v = dl[j];
          if (j < N) argmax_combine(bv, bi, v, j);
        }
        wave_argmax_dpp(bv, bi);
        if (l == 0)
          __hip_atomic_store(reinterpret_cast<unsigned long long*>(pubp + kVitEndWord),
                             ((unsigned long long)__builtin_bit_cast(unsigned, bv) << 32) | (vit_end_tag(a.token) << 8) |
                                 (unsigned)(bi < N ? bi : 0),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (FB && pubon && nblocks > 6) {
      // the loop's flushes (blocks < nblocks - 2) retired: published now, so the followers form
      // those rows while the last two blocks are flushed (the final count comes after them)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();  // (the chain wave has ended: the helpers alone)
      if (hi == 0 && l == 0) publish_count(pubp, nblocks - 2, a.token);
    }
    const float lsv2 = nblocks >= 2 ? rec_ls_scan<NP, KIND>(a, lds, b, nblocks - 2, base, w == 1) : 0.f;
    const float lsv1 = rec_ls_scan<NP, KIND>(a, lds, b, nblocks - 1, base, w == 1);
    if (FB && pubon) {
      // the last two blocks' rows first, then completion published, then their exp outputs
      // (the followers read only the rows)
#pragma unroll
      for (int h = 0; h < HV; ++h) {
        const int vw = vw_of(h);
        if (vw < C::NW) {
          if (nblocks >= 2) rec_flush<NP, KIND, 1>(a, lds, b, nblocks - 2, l + 64 * vw, lsv2);
          rec_flush<NP, KIND, 1>(a, lds, b, nblocks - 1, l + 64 * vw, lsv1);
        }
      }
      if (endson) end_post();  // (the end rows' posterior while those stores retire)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();  // (the chain wave has ended: the helpers alone)
      if (hi == 0 && l == 0) publish_count(pubp, nblocks + 1, a.token);
      if (kStamp && hi == 0 && l == 0) g_rec_stamps[((size_t)blockIdx.x * 16 % kStampWaves) * 8 + 2] = __builtin_amdgcn_s_memrealtime();
    }
#pragma unroll
    for (int h = 0; h < HV; ++h) {
      const int vw = vw_of(h);
      if (vw < C::NW) {
        if (FB && pubon) {
          if (nblocks >= 2) rec_flush<NP, KIND, 2>(a, lds, b, nblocks - 2, l + 64 * vw, lsv2);
          rec_flush<NP, KIND, 2>(a, lds, b, nblocks - 1, l + 64 * vw, lsv1);
        } else {
          if (nblocks >= 2) rec_flush<NP, KIND>(a, lds, b, nblocks - 2, l + 64 * vw, lsv2);
          rec_flush<NP, KIND>(a, lds, b, nblocks - 1, l + 64 * vw, lsv1);
        }
        if (KIND == kFbAlpha && a.loglik && vw == C::NW - 1 && l == 0)
          a.loglik[b] = rec_loglik<NP>(lds, T, base);
      }
    }
    if constexpr (KIND == kFbAlpha) {
      // the reference's compute_likelihood, logsumexp_j log(forward_{T-1}[j] + 1e-8)
      // (hmm.py:206), from the last row in LDS and its log-scale: post.h's arithmetic
      if (a.lik_ref && hi == 0) {
        const float ls = __shfl(lsv1, (T - 1) & 15);
        const float* u = lds + C::OFF_RING + ((T - 1) & (C::RING - 1)) * NP;
        float lv[NB], m = -INFINITY;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          const int j = l + 64 * k;
          lv[k] = j < N ? __logf(__expf(__logf(u[j]) + ls) + 1e-8f) : -INFINITY;
          m = fmaxf(m, lv[k]);
        }
        m = wave_max(m);
        float e = 0.f;
#pragma unroll
        for (int k = 0; k < NB; ++k) e += (l + 64 * k < N) ? __expf(lv[k] - m) : 0.f;
        e = wave_sum(e);
        if (l == 0) a.lik_ref[b] = m + __logf(e);
      }
    }
    if constexpr (FUSE) {
      // the psi rows of the last three blocks (the loop copied up to block nblocks - 4)
      psi_copy(nblocks - 3);
      lds_barrier();  // the psi waves' last rows
      psi_copy(nblocks - 2);
      psi_copy(nblocks - 1);
    }
    if (!FB && pubon) {
      // everything stored: every helper's stores retired, then one lane publishes completion
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();  // (the chain and psi waves have ended: the helpers alone)
      if (hi == 0 && l == 0) publish_count(pubp, nblocks + 1, a.token);
      if (kStamp && hi == 0 && l == 0) g_rec_stamps[((size_t)blockIdx.x * 16 % kStampWaves) * 8 + 2] = __builtin_amdgcn_s_memrealtime();
    }
    if (kStamp && hi == 0) {
      // (diagnostic builds: when helper 0's last stores have retired -- the chain workgroup's exit,
      // in entry 2 of its wave's record; tools/band_stamps.py)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (l == 0) g_rec_stamps[(((size_t)blockIdx.x * 16 + w) % kStampWaves) * 8 + 2] = __builtin_amdgcn_s_memrealtime();
    }
}

// Which chain serves a recursion (band.h): Toeplitz register windows when the window is a
// fixed offset range instantiated below (code 16*TW + TD0 + 2), else banded with LDS windows
// of the padded width (2/4/8), else the dense chain (0).
template <int KIND, int NP>
__device__ __forceinline__ int rec_band_code(const RecArgs& a) {
  if (!a.band) return 0;
  const BandDesc* d = a.band;
  const int W = KIND == kFbBeta ? d->wr : d->wc;
  if (W > kBandMax) return 0;
  const int tw = KIND == kFbBeta ? d->trw : d->tcw;
  const int td0 = KIND == kFbBeta ? d->trd0 : d->tcd0;
  if (NP <= 128 && tw > 0) {
    const int code = 16 * tw + td0 + 2;
    switch (code) {
      case 16 * 1 + 0 + 2: case 16 * 2 - 1 + 2: case 16 * 2 + 0 + 2:
      case 16 * 3 - 2 + 2: case 16 * 3 - 1 + 2: case 16 * 3 + 0 + 2: return code;
      default: break;
    }
  }
  return KIND == kFbBeta ? d->wrp : d->wcp;
}

template <int NP, int KIND>
__device__ __forceinline__ void rec_dispatch(const RecArgs& a, float* lds, int b) {
  const int code = rec_band_code<KIND, NP>(a);
  // the banded chains are written for RC<NP>::NT threads (the fused Viterbi form for 1024)
  constexpr int kBandNT = (KIND == kVit && kVitFused<NP>) ? 1024 : (KIND != kVit ? kFbNT<NP> : RC<NP>::NT);
  if (code != 0 && threadIdx.x >= kBandNT) return;
  switch (code) {
    case 2: rec_band<NP, KIND, 2>(a, lds, b, a.band); break;
    case 4: rec_band<NP, KIND, 4>(a, lds, b, a.band); break;
    case 8: rec_band<NP, KIND, 8>(a, lds, b, a.band); break;
    case 16 * 1 + 0 + 2: rec_band<NP, KIND, 2, 0, 1>(a, lds, b, a.band); break;
    case 16 * 2 - 1 + 2: rec_band<NP, KIND, 2, -1, 2>(a, lds, b, a.band); break;
    case 16 * 2 + 0 + 2: rec_band<NP, KIND, 2, 0, 2>(a, lds, b, a.band); break;
    case 16 * 3 - 2 + 2: rec_band<NP, KIND, 2, -2, 3>(a, lds, b, a.band); break;
    case 16 * 3 - 1 + 2: rec_band<NP, KIND, 2, -1, 3>(a, lds, b, a.band); break;
    case 16 * 3 + 0 + 2: rec_band<NP, KIND, 2, 0, 3>(a, lds, b, a.band); break;
    default:
      // dense: the register-blocked chain for NP <= 128; NP = 256 keeps the DPP-broadcast chain
      // (16 waves leave 128 VGPRs a lane, too few for the register-blocked slices)
      if constexpr (NP <= 128) {
        if (threadIdx.x >= kRbHelpers<NP>::NT) return;  // (waves beyond the chain and its helpers)
        rec_run_rb<NP, KIND>(a, lds, b);
      } else {
        if (threadIdx.x >= RC<NP>::NT) return;
        rec_run_dpp<NP, KIND>(a, lds, b);
      }
      break;
  }
}

}  // namespace hmm355
