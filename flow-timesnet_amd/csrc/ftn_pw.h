// Shared between stage_a.hip and the stage-C units: the pointwise argument block, the grid-pixel decode of every
// pixel-major kernel, and the launch entries of stage_a.hip (gfx950 only).
#pragma once
#include "ftn_common.h"

struct FinalizeArgs;   // ftn_finalize.h

struct PwArgs {
  const float* x;        // [B][L][C] (when XIN)
  const float* in;       // [N][KIN]  (when !XIN)
  const float* W;        // [16*n_ot][KIN]
  const float* bias;     // [16*n_ot]
  float* out;            // [N][OUTC]
  float* R;              // [N][RC] (EPI 1: read, add, store back)
  const FtnDesc* desc;
  int B, L, C, KIN, n_ot, OUTC, RC;
  // stage A also publishes the sanitised descriptor copy every later launch reads (guard_desc below); it does
  // not need the descriptor itself, so this costs no extra launch
  const FtnDesc* guard_src; FtnDesc* guard_dst; int guard_groups, guard_px;
  int* range_flag;       // EPI 3 (f16x2 pieces): set when an output leaves the fp16 range; may be null
};

// ---------------------------------------------------------------- pixel decode
struct Px {
  int n;          // clamped flat pixel index
  bool ok;        // lane holds a real pixel
  const float* xrow;  // &x[b][t][0] or nullptr for t >= L (live zero pixel, :1017)
};

__device__ __forceinline__ Px decode_px(const FtnDesc* __restrict__ d, const float* __restrict__ x, int B, int L,
                                        int C, int n, int N) {
  Px p;
  p.ok = n < N;
  p.n = p.ok ? n : N - 1;
  const int G = d->n_groups;
  // the whole prefix table in one batch of scalar loads (fixed trip count), then a select chain:
  // a data-dependent loop here costs one scalar-memory round trip per group on every workgroup's
  // critical path
  int off[FTN_KMAX + 1];
#pragma unroll
  for (int i = 0; i <= FTN_KMAX; ++i) off[i] = d->g_px_off[i];
  int lo = 0, hi = off[1];
#pragma unroll
  for (int gg = 1; gg < FTN_KMAX; ++gg) {
    const bool in = gg < G && p.n >= B * off[gg];
    lo = in ? off[gg] : lo;
    hi = in ? off[gg + 1] : hi;
  }
  const int P = hi - lo;
  const int rem = p.n - B * lo;
  const int b = rem / P, t = rem - b * P;
  p.xrow = (t < L) ? x + ((size_t)b * L + t) * C : nullptr;
  return p;
}

// The same for the 16 CONSECUTIVE pixels n0 + j of one MFMA pixel unit (n0 wave-uniform).  They almost always lie
// in one period group, which a scalar walk over the (at most 16) prefix sums finds: the per-lane part is then a
// division by a uniform P.  decode_px's per-lane 16-way select chain is ~150 VALU + SALU instructions, a tenth of
// what a stage-C wave executes for its unit.  Units that straddle a group boundary take the general path.
__device__ __forceinline__ Px decode_px16(const FtnDesc* __restrict__ d, const float* __restrict__ x, int B, int L,
                                          int C, int n0, int j, int N) {
  const int G = d->n_groups;
  const int first = __builtin_amdgcn_readfirstlane(n0);
  const int last = first + 15 < N ? first + 15 : N - 1;
  int off[FTN_KMAX + 1];                                          // one batch of scalar loads, then SALU selects
#pragma unroll
  for (int i = 0; i <= FTN_KMAX; ++i) off[i] = d->g_px_off[i];
  int lo = 0, hi = off[1];
#pragma unroll
  for (int gg = 1; gg < FTN_KMAX; ++gg) {
    const bool in = gg < G && first >= B * off[gg];
    lo = in ? off[gg] : lo;
    hi = in ? off[gg + 1] : hi;
  }
  if (first < N && last < B * hi) {                              // whole unit inside one group (uniform branch)
    Px p;
    const int n = first + j;
    p.ok = n < N;
    p.n = p.ok ? n : N - 1;
    const int P = hi - lo;
    const int rem = p.n - B * lo;
    const int b = rem / P, t = rem - b * P;
    p.xrow = (t < L) ? x + ((size_t)b * L + t) * C : nullptr;
    return p;
  }
  return decode_px(d, x, B, L, C, n0 + j, N);
}

// Launch entries of stage_a.hip; act 0 GELU / 1 ReLU, epi = FtnForms.stage_a_epi.
// Stage A (k_pw), or with fa the fused selector finalize + stage A (k_finalize_pw; part: see there)
int ftn_launch_stage_a(const PwArgs& pa, const FinalizeArgs* fa, int part, int act, int epi, bool xvec, hipStream_t st);
// FTN_FORM_C_GENERIC: stage C as pointwise launches; pg: x, desc, B, L, C, in = m, out = a' (pieces as epi says), R; G = hidden
int ftn_launch_stagec_generic(PwArgs pg, const FtnPlan* pl, const float* wb, float* G, long long Nmax, int act, int epi, bool xvec,
                              hipStream_t st);
// merged-conv plans: stage A is a zero-extended copy of x (k_embed); pa: x, out, B, L, C and the guard_* fields
int ftn_launch_embed(const PwArgs& pa, int CP, hipStream_t st);
// out = LayerNorm_C(x + (nw - x)) per row (k_resid_ln); in place allowed
int ftn_launch_resid_ln(const float* x, const float* nw, float* out, const float* g, const float* b, float eps, long long rows,
                        int C, hipStream_t st);
