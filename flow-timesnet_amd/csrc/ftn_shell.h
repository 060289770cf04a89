// What the model-shell units share - the kernel units shell.hip (d_model <= 128), shell_wide.hip (128 < d_model <= 512)
// and timeproj.hip, and the host entry layer shell_api.hip: the argument blocks, the heads' softplus, the two widths,
// and the form and launch functions the kernel units define for the entry layer.
#pragma once
#include "ftn_common.h"

// softplus(beta=1, threshold=20) as torch evaluates it (x > 20 -> x, else log1p(exp(x))), in the
// overflow-free form max(x,0) + log1p(exp(-|x|)).  exp2/log2 are the raw hardware ops (1 ulp).  Two roundings would
// each cost more than those: t = -|x| log2(e) rounded to fp32 is a relative error of |x| 2^-24 in e (5 ulp of the
// result at x = -10), so t is carried as hi + lo and the lo part applied to e; and 1 + e rounded is a relative error
// of 2^-24 / e in log(1 + e) (32 ulp just above e = 2^-6), so the rounding error of the sum is handed back through
// log(u + d) = log(u) + d / u.  Below 2^-6 the series replaces the logarithm.  |x| is clamped at 128 (e = 0 in fp32
// from |x| = 104 on) so that an infinite x does not meet inf - inf in the lo part; a NaN stays a NaN.
__device__ __forceinline__ float softplus20(float x) {
  if (x > 20.f) return x;
  const float ax = fabsf(x);
  const float a = ax > 128.f ? -128.f : -ax;
  const float th = a * 1.44269504088896341f;
  const float tl = fmaf(a, 1.44269504088896341f, -th) + a * 1.925963033500011e-8f;
  float e = __builtin_amdgcn_exp2f(th);
  e = fmaf(e, tl * 0.69314718055994531f, e);
  const float series = e * (1.f - e * (0.5f - e * (0.33333333333f - 0.25f * e)));
  const float u = 1.f + e;
  const float lg = fmaf(__builtin_amdgcn_logf(u), 0.69314718055994531f, (e - (u - 1.f)) * __builtin_amdgcn_rcpf(u));
  return fmaxf(x, 0.f) + (e < 0.015625f ? series : lg);
}

// softplus20's derivative as torch's backward takes it: sigmoid(x) up to the threshold, 1 above
__device__ __forceinline__ float sigmoid20(float x) {
  return x > 20.f ? 1.f : __builtin_amdgcn_rcpf(1.f + __expf(-x));
}

struct HeadArgs {
  const float* hidden;   // [rows][D]
  const float* wmu;      // [N][D]
  const float* bmu;      // [N]
  const float* wsg;
  const float* bsg;
  const float* tail;     // element (b, s, n) at tail[b * tail_bs + min(s, hist-1) * N + n]
  const float* late;     // optional, element (b, s, n) at late[b * late_bs + s * N + n]
  const float* floorv;   // optional [N]
  float* rate;           // [rows][N]
  float* disp;
  int* bad;              // |= 1 if a rate is not finite-positive, |= 2 for a dispersion
  float* sig_mu;         // optional [rows][N] (both or neither, ftn_head_fit_forward): softplus' derivative at the two
  float* sig_sg;         // pre-activations, for the heads' backward (headfit.hip)
  long long rows, tail_bs, late_bs;
  int S, D, N, hist;
  float floor_s;
};

// The norm over d_model that closes an embedding row: a field of the argument blocks, not a template argument - the
// kernel forms are the same for all three.
enum { FTN_NORM_NONE = 0, FTN_NORM_LAYER = 1, FTN_NORM_RMS = 2 };

struct EmbedArgs {
  const float* x;
  const float* W;        // [D][N]
  const float* add;      // optional
  const float* ln_g;     // gamma / beta of the norm epilogue ("layer" and "rms" modes)
  const float* ln_b;
  float* out;            // row (b, l) at out + b * out_bs + l * D
  long long x_bs, add_bs, out_bs;
  int B, L, N, D;
  float ln_eps;
  int norm;              // FTN_NORM_*
};

struct RingArgs {
  const float* V;        // [B][L][D]
  const float* add;      // optional, row (b, t) at add + b * add_bs + t * D
  const float* ln_g;
  const float* ln_b;
  float* out;            // [B][L][D]
  long long add_bs;
  int B, L, D, head;
  float ln_eps;
  int norm;              // FTN_NORM_*
};

struct TimeProjArgs {
  const float* seq;      // [B][L][D]; with rows: the item store [n_items][L][D]
  const long long* rows; // null, or [B]: batch row b reads item rows[b] clamped into 0 .. n_items - 1
  long long n_items;
  const float* wt;       // [S][L], base only 4-byte aligned when it is a row slice at L % 4 != 0
  const float* bt;       // [S]
  float* hid;            // [B][S][D]
  int B, L, D, S;
};

// The two widths of the shell.  An exported entry names its width and hands it to the shared body (shell_api.hip);
// nothing picks it from d_model, so ftn_embed_forward rejects 132 and ftn_embed_wide_forward rejects 128.  The two
// flags are checks only the wide entries make.  That is deliberate: the narrow entries accept what they accepted
// before the wide ones existed.
struct ShellWidth {
  bool wide;
  int d_min, d_max;      // d_model: a multiple of 4 in [d_min, d_max]
  const char* range;     // how the message about d_model names the range
  bool rows_fit_grid;    // embedding, embedding rows, ring: B * L <= 0x7fffffff
  bool align4;           // embedding, embedding rows: x and W 4-byte aligned; heads: every operand besides hidden
                         // and the weights (those are 16-byte aligned at either width)
  bool d_ok(int D) const { return D >= d_min && D <= d_max && D % 4 == 0; }
};
inline constexpr ShellWidth kShellNarrow = {false, 4, 128, "<= 128", false, false};
inline constexpr ShellWidth kShellWide = {true, 132, 512, "> 128 and <= 512", true, true};

// gridDim.y of the head kernels: a workgroup's four waves take a 16-row tile each, up to the form's cap (form >> 16)
static inline unsigned head_grid_y(long long rows, int form) {
  const long long rtiles = (rows + 15) / 16, want = form >> 16;
  const long long gy = (rtiles + 3) / 4;
  return (unsigned)(gy > want ? want : gy);
}

// What the kernel units define for the entry layer: the form rules and one launch per operation and width, taking
// the filled and checked argument block.  Internal to the library, so kept out of its dynamic symbol table.
#pragma GCC visibility push(hidden)
int head_form(int N, int D, long long tail_bs, long long late_bs, unsigned misalign);               // shell.hip
int embed_form(int N, int D, long long x_bs, unsigned misalign);
int head_launch(const HeadArgs& a, hipStream_t st);
int embed_launch(const EmbedArgs& a, hipStream_t st);
int ring_launch(const RingArgs& a, hipStream_t st);
int head_wide_form(int N, int D, long long tail_bs, long long late_bs, unsigned misalign);          // shell_wide.hip
int embed_wide_form(int N, int D, long long x_bs, unsigned misalign);
int head_wide_launch(const HeadArgs& a, hipStream_t st);
int embed_wide_launch(const EmbedArgs& a, hipStream_t st);
int ring_wide_launch(const RingArgs& a, hipStream_t st);
int timeproj_form(int L, int S, unsigned wt_misalign);                                               // timeproj.hip
int timeproj_launch(const TimeProjArgs& a, const ShellWidth& w, hipStream_t st);
#pragma GCC visibility pop
