// Context front end of the model shell (include/flowtimes.h, "context front end"): what TimesNet.forward computes
// from the series rows before the value embedding and the heads see it.
//   k_context_rows        static projection | id embedding -> context_norm -> coefficients, constant bias, late bias
//   k_through_small /     the contraction over series of the two context terms with the value weight
//   k_through_chunks
//   k_embed_add           add[Ba][L][D]: positional (+ time-feature) term, "decoupled" norm, value bias, context terms
// Plain fp32 arithmetic on the VALU: latency- and bandwidth-bound, no MFMA, no workspace, no atomics.  Every sum is a
// chain of FMAs in index order or a fixed tree whose shape depends on the sizes alone, so an output's bits are a
// function of its own row's inputs, the parameters and the sizes - not of the batch, of its position in the grid or
// of which rows share the call.
#include "ftn_common.h"

#include "ftn_ctxrow.h"          // CTX_MAX, CTX_SLOTS, wave_sum, wave_layernorm, dot_chain (shared with latefit.hip)

#define CTX_RMAX 32
#define ADD_DMAX 512
#define ADD_TMAX 64

// ---------------------------------------------------------------------------------------------
// Series rows
// ---------------------------------------------------------------------------------------------
struct RowsArgs {
  FtnContextParams p;
  const float* st;
  const long long* ids;
  long long st_bs, ids_bs;
  int N;
  float *rows, *coeff, *cbias, *late;
};

// One wave owns one row (bc, n).  The row's vectors live in LDS for the dot products (every lane walks a whole
// vector: an output element is one lane's chain) and four to a lane for the LayerNorms.
__global__ __launch_bounds__(64) void k_context_rows(RowsArgs a) {
  __shared__ float xs[CTX_MAX];        // the static features, later late_bias_norm(c)
  __shared__ float cs[CTX_MAX];        // cat(s, e), then c
  const FtnContextParams& p = a.p;
  const int lane = threadIdx.x;
  const long long row = blockIdx.x;
  const long long bc = row / a.N;
  const int n = (int)(row - bc * a.N);
  const int ctx = p.Ws + p.Ed;
  const float qnan = __uint_as_float(0x7fc00000u);
  bool bad = false;
  if (p.Ws > 0) {
    const float* __restrict__ sp = a.st + bc * a.st_bs + (long long)n * p.F;
    for (int k = lane; k < p.F; k += 64) xs[k] = sp[k];
    __syncthreads();
    float v[CTX_SLOTS];
#pragma unroll
    for (int j = 0; j < CTX_SLOTS; ++j) {
      const int o = lane + 64 * j;
      v[j] = o < p.Ws ? dot_chain(p.w_s + (size_t)o * p.F, xs, p.F) + p.b_s[o] : 0.f;
    }
    if (p.sn_g) wave_layernorm(v, p.Ws, lane, p.sn_g, p.sn_b, p.sn_eps);
#pragma unroll
    for (int j = 0; j < CTX_SLOTS; ++j)
      if (lane + 64 * j < p.Ws) cs[lane + 64 * j] = v[j];
  }
  if (p.Ed > 0) {
    const long long id = a.ids[bc * a.ids_bs + n];
    bad = id < 0 || id >= (long long)p.V;              // never read outside the table: the row's outputs are NaN
    for (int k = lane; k < p.Ed; k += 64) cs[p.Ws + k] = bad ? 0.f : p.emb[(size_t)id * p.Ed + k];
  }
  __syncthreads();
  float c[CTX_SLOTS];
#pragma unroll
  for (int j = 0; j < CTX_SLOTS; ++j) c[j] = lane + 64 * j < ctx ? cs[lane + 64 * j] : 0.f;
  wave_layernorm(c, ctx, lane, p.cn_g, p.cn_b, p.cn_eps);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < CTX_SLOTS; ++j) {
    const int k = lane + 64 * j;
    if (k < ctx) {
      cs[k] = c[j];
      if (a.rows) a.rows[row * ctx + k] = bad ? qnan : c[j];
    }
  }
  __syncthreads();
  // lanes 0 .. R - 1: the coefficients; lane R: the constant bias
  const int R = a.coeff ? p.R : 0;
  if (lane < R || (lane == R && a.cbias)) {
    const bool co = lane < R;
    const float v = dot_chain(co ? p.w_c + (size_t)lane * ctx : p.w_p, cs, ctx) + (co ? p.b_c[lane] : p.b_p[0]);
    *(co ? a.coeff + row * R + lane : a.cbias + row) = bad ? qnan : v;
  }
  if (a.late) {
    wave_layernorm(c, ctx, lane, p.ln_g, p.ln_b, p.ln_eps);
#pragma unroll
    for (int j = 0; j < CTX_SLOTS; ++j)
      if (lane + 64 * j < ctx) xs[lane + 64 * j] = c[j];
    __syncthreads();
    for (int s = lane; s < p.steps; s += 64) {
      const float v = p.gate[s] * (dot_chain(p.w_l + (size_t)s * ctx, xs, ctx) + p.b_l[s]);
      a.late[(bc * p.steps + s) * a.N + n] = bad ? qnan : v;
    }
  }
}

static inline int cdiv64(int v) { return (v + 63) / 64; }

extern "C" int ftn_context_rows_form(int F, int Ws, int Ed, int R, int steps) {
  FTN_CHECK_ARG(F >= 0 && F <= CTX_MAX && Ws >= 0 && Ws <= CTX_MAX && Ed >= 0 && Ed <= CTX_MAX && Ws + Ed >= 1 &&
                    Ws + Ed <= CTX_MAX && (Ws == 0 || F >= 1) && R >= 0 && R <= CTX_RMAX && steps >= 0,
                "ftn_context_rows_form: F=%d Ws=%d Ed=%d R=%d steps=%d", F, Ws, Ed, R, steps);
  const int passes = cdiv64(steps);
  return cdiv64(Ws + Ed) | cdiv64(Ws) << 4 | (passes > 255 ? 255 : passes) << 8;
}

extern "C" int ftn_context_rows(const FtnContextParams* params, const float* static_dev_or_null,
                                long long static_bstride, const long long* ids_dev_or_null, long long ids_bstride,
                                int Bc, int N, float* rows_out_or_null, float* coeff_out_or_null,
                                float* cbias_out_or_null, float* late_out_or_null, void* stream) {
  FTN_CHECK_ARG(params != nullptr, "ftn_context_rows: null parameter block");
  const FtnContextParams& p = *params;
  FTN_CHECK_ARG(p.Ws >= 0 && p.Ed >= 0 && p.Ws + p.Ed >= 1, "ftn_context_rows: Ws=%d Ed=%d: no context", p.Ws, p.Ed);
  FTN_CHECK_ARG(p.Ws + p.Ed <= CTX_MAX && p.Ws <= CTX_MAX && p.Ed <= CTX_MAX,
                "ftn_context_rows: ctx=%d (Ws=%d Ed=%d) exceeds %d", p.Ws + p.Ed, p.Ws, p.Ed, CTX_MAX);
  FTN_CHECK_ARG(p.Ws == 0 || (p.F >= 1 && p.F <= CTX_MAX), "ftn_context_rows: F=%d outside [1, %d]", p.F, CTX_MAX);
  FTN_CHECK_ARG(Bc >= 1 && N >= 1 && (long long)Bc * N <= 0x7fffffffLL, "ftn_context_rows: bad shape Bc=%d N=%d", Bc, N);
  FTN_CHECK_ARG(p.Ws == 0 || (static_dev_or_null && p.w_s && p.b_s),
                "ftn_context_rows: null pointer (static features, static_proj weight or bias)");
  FTN_CHECK_ARG((p.sn_g == nullptr) == (p.sn_b == nullptr), "ftn_context_rows: static_norm needs both gamma and beta");
  FTN_CHECK_ARG(p.Ed == 0 || (ids_dev_or_null && p.emb && p.V >= 1),
                "ftn_context_rows: null pointer (ids or embedding table) or V=%d", p.V);
  FTN_CHECK_ARG(p.cn_g && p.cn_b, "ftn_context_rows: null pointer (context_norm gamma / beta)");
  FTN_CHECK_ARG(rows_out_or_null || coeff_out_or_null || cbias_out_or_null || late_out_or_null,
                "ftn_context_rows: null pointer (no output)");
  if (coeff_out_or_null) {
    FTN_CHECK_ARG(p.R >= 1 && p.R <= CTX_RMAX, "ftn_context_rows: R=%d outside [1, %d]", p.R, CTX_RMAX);
    FTN_CHECK_ARG(p.w_c && p.b_c, "ftn_context_rows: null pointer (context_coeff weight or bias)");
  }
  FTN_CHECK_ARG(!cbias_out_or_null || (p.w_p && p.b_p), "ftn_context_rows: null pointer (context_proj weight or bias)");
  if (late_out_or_null) {
    FTN_CHECK_ARG(p.steps >= 1 && (long long)Bc * N * p.steps <= 0x7fffffffffLL, "ftn_context_rows: steps=%d", p.steps);
    FTN_CHECK_ARG(p.ln_g && p.ln_b && p.w_l && p.b_l && p.gate,
                  "ftn_context_rows: null pointer (late_bias_norm, late_bias_head or gate)");
  }
  FTN_CHECK_ARG(Bc == 1 || ((p.Ws == 0 || static_bstride >= 0) && (p.Ed == 0 || ids_bstride >= 0)),
                "ftn_context_rows: negative batch stride");
  FTN_CHECK_ARG((((uintptr_t)static_dev_or_null | (uintptr_t)p.w_s | (uintptr_t)p.b_s | (uintptr_t)p.sn_g |
                  (uintptr_t)p.sn_b | (uintptr_t)p.emb | (uintptr_t)p.cn_g | (uintptr_t)p.cn_b | (uintptr_t)p.w_c |
                  (uintptr_t)p.b_c | (uintptr_t)p.w_p | (uintptr_t)p.b_p | (uintptr_t)p.ln_g | (uintptr_t)p.ln_b |
                  (uintptr_t)p.w_l | (uintptr_t)p.b_l | (uintptr_t)p.gate | (uintptr_t)rows_out_or_null |
                  (uintptr_t)coeff_out_or_null | (uintptr_t)cbias_out_or_null | (uintptr_t)late_out_or_null) & 3) == 0 &&
                    ((uintptr_t)ids_dev_or_null & 7) == 0,
                "ftn_context_rows: fp32 operands must be 4-byte aligned, ids 8-byte aligned");
  RowsArgs a;
  a.p = p;
  a.st = p.Ws > 0 ? static_dev_or_null : nullptr;
  a.ids = p.Ed > 0 ? ids_dev_or_null : nullptr;
  a.st_bs = Bc > 1 ? static_bstride : 0;
  a.ids_bs = Bc > 1 ? ids_bstride : 0;
  a.N = N;
  a.rows = rows_out_or_null; a.coeff = coeff_out_or_null; a.cbias = cbias_out_or_null; a.late = late_out_or_null;
  hipLaunchKernelGGL(k_context_rows, dim3((unsigned)((long long)Bc * N)), dim3(64), 0, (hipStream_t)stream, a);
  FTN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// The context terms through the value weight: q_coeff[bc][r][d] = sum_n coeff[bc][n][r] w[d][n],
//                                             q_bias[bc][d]     = sum_n cbias[bc][n] w[d][n]
// ---------------------------------------------------------------------------------------------
struct ThroughArgs {
  const float *coeff, *cbias, *w;
  long long ldw;
  float *qc, *qb;
  int Bc, N, R, D;
};

#define TW_CHUNK 64          // series per chunk; N <= TW_CHUNK is one chain (k_through_small)
#define TW_DT 16             // d_model columns of a k_through_chunks workgroup
#define TW_WAVES 4
#define TW_COLS (CTX_RMAX + 1)

// N <= 64 (the pipeline layout has N = 1, where this is a scale): a thread owns (bc, d) and walks the series once per
// term, one FMA chain in n order.  Lanes run along d: the stores are coalesced, the coeff loads wave-uniform.
__global__ __launch_bounds__(256) void k_through_small(ThroughArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.Bc * a.D) return;
  const long long bc = i / a.D;
  const int d = (int)(i - bc * a.D);
  const float* __restrict__ wr = a.w + (long long)d * a.ldw;
  if (a.qc) {
    const float* __restrict__ cp = a.coeff + bc * a.N * a.R;
    for (int r = 0; r < a.R; ++r) {
      float acc = 0.f;
      for (int n = 0; n < a.N; ++n) acc = fmaf(cp[(size_t)n * a.R + r], wr[n], acc);
      a.qc[(bc * a.R + r) * a.D + d] = acc;
    }
  }
  if (a.qb) {
    const float* __restrict__ bp = a.cbias + bc * a.N;
    float acc = 0.f;
    for (int n = 0; n < a.N; ++n) acc = fmaf(bp[n], wr[n], acc);
    a.qb[bc * a.D + d] = acc;
  }
}

// N > 64: a workgroup owns (bc, 16 columns of d) and all R + 1 terms (term R is the bias).  The series are cut into
// chunks of 64; wave w takes chunks w, w + 4, ... in ascending order, each staged through LDS with coalesced loads (w
// along n, coeff as the contiguous [64][R] block it is), and lane (dl, rg) carries one FMA chain in n order per term
// rg + 4 j of column dl.  The four waves' partial sums are then added as (p0 + p1) + (p2 + p3): the tree is a function
// of N alone.
__global__ __launch_bounds__(256) void k_through_chunks(ThroughArgs a) {
  __shared__ float wt[TW_WAVES][TW_DT][TW_CHUNK + 1];
  __shared__ float ct[TW_WAVES][TW_CHUNK][TW_COLS];
  constexpr int NJ = (TW_COLS + 3) / 4;
  __shared__ float part[TW_WAVES][NJ][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, dl = lane & 15, rg = lane >> 4;
  const int d0 = blockIdx.x * TW_DT;
  const long long bc = blockIdx.y;
  const int R = a.qc ? a.R : 0;
  const int ncol = R + (a.qb ? 1 : 0);
  const int nch = (a.N + TW_CHUNK - 1) / TW_CHUNK;
  float acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
  for (int it = 0; it * TW_WAVES < nch; ++it) {
    const int n0 = (it * TW_WAVES + wave) * TW_CHUNK;
    const int nn = a.N - n0 < TW_CHUNK ? a.N - n0 : TW_CHUNK;          // <= 0: this wave has no chunk in this round
    if (nn > 0) {
#pragma unroll 4
      for (int dd = 0; dd < TW_DT; ++dd)
        wt[wave][dd][lane] = lane < nn && d0 + dd < a.D ? a.w[(long long)(d0 + dd) * a.ldw + n0 + lane] : 0.f;
      if (R > 0) {
        const float* __restrict__ cp = a.coeff + (bc * a.N + n0) * R;
        for (int f = lane; f < nn * R; f += 64) ct[wave][f / R][f % R] = cp[f];
      }
      if (a.qb && lane < nn) ct[wave][lane][R] = a.cbias[bc * a.N + n0 + lane];
    }
    __syncthreads();
    for (int n = 0; n < nn; ++n) {
      const float wv = wt[wave][dl][n];
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (rg + 4 * j < ncol) acc[j] = fmaf(ct[wave][n][rg + 4 * j], wv, acc[j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) part[wave][j][lane] = acc[j];
  __syncthreads();
  for (int j = wave; j < NJ; j += TW_WAVES) {
    const int col = rg + 4 * j, d = d0 + dl;
    if (col >= ncol || d >= a.D) continue;
    const float tot = (part[0][j][lane] + part[1][j][lane]) + (part[2][j][lane] + part[3][j][lane]);
    if (col < R) a.qc[(bc * R + col) * a.D + d] = tot;
    else a.qb[bc * a.D + d] = tot;
  }
}

extern "C" int ftn_context_through_weight(const float* coeff_dev_or_null, const float* cbias_dev_or_null, int Bc,
                                          int N, int R, const float* w_dev, long long w_rstride, int D,
                                          float* q_coeff_out_or_null, float* q_bias_out_or_null, void* stream) {
  FTN_CHECK_ARG(w_dev && (q_coeff_out_or_null || q_bias_out_or_null) &&
                    (!q_coeff_out_or_null || coeff_dev_or_null) && (!q_bias_out_or_null || cbias_dev_or_null),
                "ftn_context_through_weight: null pointer");
  FTN_CHECK_ARG(Bc >= 1 && Bc <= 0x7fffffff / ADD_DMAX && N >= 1 && D >= 1,
                "ftn_context_through_weight: bad shape Bc=%d N=%d D=%d", Bc, N, D);
  FTN_CHECK_ARG(D % 4 == 0, "ftn_context_through_weight: d_model=%d must be a multiple of 4", D);
  FTN_CHECK_ARG(D <= ADD_DMAX, "ftn_context_through_weight: d_model=%d exceeds %d", D, ADD_DMAX);
  FTN_CHECK_ARG(!q_coeff_out_or_null || (R >= 1 && R <= CTX_RMAX), "ftn_context_through_weight: R=%d outside [1, %d]",
                R, CTX_RMAX);
  FTN_CHECK_ARG(w_rstride >= N, "ftn_context_through_weight: w_rstride=%lld < N=%d", w_rstride, N);
  FTN_CHECK_ARG((((uintptr_t)coeff_dev_or_null | (uintptr_t)cbias_dev_or_null | (uintptr_t)w_dev |
                  (uintptr_t)q_coeff_out_or_null | (uintptr_t)q_bias_out_or_null) & 3) == 0,
                "ftn_context_through_weight: every operand must be 4-byte aligned");
  ThroughArgs a;
  a.coeff = coeff_dev_or_null; a.cbias = cbias_dev_or_null; a.w = w_dev; a.ldw = w_rstride;
  a.qc = q_coeff_out_or_null; a.qb = q_bias_out_or_null; a.Bc = Bc; a.N = N; a.R = R; a.D = D;
  hipStream_t st = (hipStream_t)stream;
  if (N <= TW_CHUNK) {
    const long long total = (long long)Bc * D;
    hipLaunchKernelGGL(k_through_small, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
  } else {
    FTN_CHECK_ARG(Bc <= 65535, "ftn_context_through_weight: Bc=%d exceeds the launch grid at N=%d > %d", Bc, N, TW_CHUNK);
    hipLaunchKernelGGL(k_through_chunks, dim3((D + TW_DT - 1) / TW_DT, Bc), dim3(256), 0, st, a);
  }
  FTN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// add[ba][l][:], the operand of the embedding kernels
// ---------------------------------------------------------------------------------------------
struct AddArgs {
  FtnEmbedAddParams p;
  const float *mark, *qc, *qb;
  long long mark_bs, qc_bs, qb_bs;
  float* out;
  int Ba, L, D, R;
};

template <bool VEC>
__device__ __forceinline__ f4 ld4(const float* __restrict__ p) {
  if (VEC) return *(const f4*)p;
  return f4{p[0], p[1], p[2], p[3]};
}

// One wave owns one row (ba, l); lane `lane` holds columns 4 lane + 256 o .. + 3 (o < NO): every row-shaped operand
// is read and the row is written in runs of 16 bytes a lane, 1 KB a wave.  The terms are applied left to right:
//   aux = pos (+ (mark W_t^T + b_t));  "decoupled": aux = gate * LayerNorm(aux);  t = aux + b_v;
//   t = t + scale * (basisc[l] . q_coeff[bc]);  add = t + q_bias[bc]
// VEC: 16-byte loads (every row-shaped operand 16-byte aligned); otherwise 4-byte loads, the same arithmetic (the
// only FMAs are the explicit chains).
template <int NO, bool VEC>
__global__ __launch_bounds__(256) void k_embed_add(AddArgs a) {
#pragma clang fp contract(off)                                   // the two load widths must not round differently
  const FtnEmbedAddParams& p = a.p;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + wave;
  if (row >= (long long)a.Ba * a.L) return;                    // (a whole wave: the kernel has no barrier)
  const long long b = row / a.L;
  const int l = (int)(row - b * a.L);
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  f4 t[NO];
  int dcol[NO];
  bool ok[NO];
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    dcol[o] = 4 * lane + 256 * o;
    ok[o] = dcol[o] < a.D;
    t[o] = zero;
  }
  if (p.pos) {
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      if (!ok[o]) continue;
      const int d = dcol[o];
      t[o] = ld4<VEC>(p.pos + (size_t)l * a.D + d);
      if (a.mark) {
        const float* __restrict__ mp = a.mark + b * a.mark_bs + (long long)l * p.T;
        f4 m = zero;
        for (int k = 0; k < p.T; ++k) {
          const float mk = mp[k];
#pragma unroll
          for (int e = 0; e < 4; ++e) m[e] = fmaf(mk, p.w_t[(size_t)(d + e) * p.T + k], m[e]);
        }
        t[o] = t[o] + (m + ld4<VEC>(p.b_t + d));
      }
    }
    if (p.aux_g) {
      float s = 0.f;
#pragma unroll
      for (int o = 0; o < NO; ++o)
        if (ok[o]) s += (t[o][0] + t[o][1]) + (t[o][2] + t[o][3]);
      const float mean = wave_sum(s) / (float)a.D;
      float ss = 0.f;
#pragma unroll
      for (int o = 0; o < NO; ++o)
        if (ok[o]) {
          t[o] = t[o] - mean;
          ss += (t[o][0] * t[o][0] + t[o][1] * t[o][1]) + (t[o][2] * t[o][2] + t[o][3] * t[o][3]);
        }
      const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)a.D + p.aux_eps);
#pragma unroll
      for (int o = 0; o < NO; ++o)
        if (ok[o]) {
          const int d = dcol[o];
          t[o] = ld4<VEC>(p.gate + d) * (t[o] * rstd * ld4<VEC>(p.aux_g + d) + ld4<VEC>(p.aux_b + d));
        }
    }
#pragma unroll
    for (int o = 0; o < NO; ++o)
      if (ok[o]) t[o] = t[o] + ld4<VEC>(p.b_v + dcol[o]);
  }
  if (a.qc) {
    const float sc = p.scale[0];
    const float* __restrict__ bp = p.basisc + (size_t)l * a.R;
    const float* __restrict__ qp = a.qc + b * a.qc_bs;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      if (!ok[o]) continue;
      f4 acc = zero;
      for (int r = 0; r < a.R; ++r) {
        const float bv = bp[r];
        const f4 q = ld4<VEC>(qp + (size_t)r * a.D + dcol[o]);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(bv, q[e], acc[e]);
      }
      t[o] = t[o] + acc * sc;
    }
  }
  if (a.qb) {
#pragma unroll
    for (int o = 0; o < NO; ++o)
      if (ok[o]) t[o] = t[o] + ld4<VEC>(a.qb + b * a.qb_bs + dcol[o]);
  }
#pragma unroll
  for (int o = 0; o < NO; ++o)
    if (ok[o]) *(f4*)(a.out + row * a.D + dcol[o]) = t[o];
}

// The form ftn_embed_add takes: the one place the choice is made.  misalign: the OR of the byte offsets of every
// row-shaped operand (pos, b_t, gate, aux gamma / beta, b_v, q_coeff, q_bias) from a 16-byte boundary.
static int embed_add_form(int D, long long qc_bs, long long qb_bs, unsigned misalign) {
  const bool vec = qc_bs % 4 == 0 && qb_bs % 4 == 0 && (misalign & 15) == 0;
  return (vec ? FTN_SHELL_VEC : 0) | (D <= 256 ? 1 : 2) << 4;
}

extern "C" int ftn_embed_add_form(int D, long long q_coeff_bstride, long long q_bias_bstride, int misalign_or) {
  FTN_CHECK_ARG(D >= 4 && D <= ADD_DMAX && D % 4 == 0 && misalign_ok(misalign_or),
                "ftn_embed_add_form: d_model=%d misalign=%d", D, misalign_or);
  return embed_add_form(D, q_coeff_bstride, q_bias_bstride, (unsigned)misalign_or);
}

extern "C" int ftn_embed_add(const FtnEmbedAddParams* params, const float* mark_dev_or_null, long long mark_bstride,
                             const float* q_coeff_dev_or_null, long long q_coeff_bstride, int R,
                             const float* q_bias_dev_or_null, long long q_bias_bstride, int Ba, int L, int D,
                             float* out_dev, void* stream) {
  FTN_CHECK_ARG(params != nullptr && out_dev != nullptr, "ftn_embed_add: null pointer");
  const FtnEmbedAddParams& p = *params;
  FTN_CHECK_ARG(Ba >= 1 && L >= 1 && (long long)Ba * L <= 0x7fffffffLL, "ftn_embed_add: bad shape Ba=%d L=%d", Ba, L);
  FTN_CHECK_ARG(D >= 4 && D % 4 == 0, "ftn_embed_add: d_model=%d must be a multiple of 4", D);
  FTN_CHECK_ARG(D <= ADD_DMAX, "ftn_embed_add: d_model=%d exceeds %d", D, ADD_DMAX);
  FTN_CHECK_ARG(p.pos || q_coeff_dev_or_null || q_bias_dev_or_null, "ftn_embed_add: null pointer (no term)");
  FTN_CHECK_ARG(p.pos ? p.b_v != nullptr : (!mark_dev_or_null && !p.aux_g),
                "ftn_embed_add: null pointer (the epilogue term needs pos and the value bias)");
  if (mark_dev_or_null) {
    FTN_CHECK_ARG(p.T >= 1 && p.T <= ADD_TMAX, "ftn_embed_add: time_dim=%d outside [1, %d]", p.T, ADD_TMAX);
    FTN_CHECK_ARG(p.w_t && p.b_t, "ftn_embed_add: null pointer (time-feature weight or bias)");
    FTN_CHECK_ARG(mark_bstride >= 0, "ftn_embed_add: negative mark_bstride");
  }
  FTN_CHECK_ARG(p.aux_g ? (p.aux_b && p.gate) : (!p.aux_b && !p.gate),
                "ftn_embed_add: the decoupled norm needs gamma, beta and the gate");
  if (q_coeff_dev_or_null) {
    FTN_CHECK_ARG(R >= 1 && R <= CTX_RMAX, "ftn_embed_add: R=%d outside [1, %d]", R, CTX_RMAX);
    FTN_CHECK_ARG(p.basisc && p.scale, "ftn_embed_add: null pointer (centred basis or scale)");
  }
  FTN_CHECK_ARG(q_coeff_bstride >= 0 && q_bias_bstride >= 0, "ftn_embed_add: negative batch stride");
  FTN_CHECK_ARG(((uintptr_t)out_dev & 15) == 0, "ftn_embed_add: out must be 16-byte aligned");
  FTN_CHECK_ARG((((uintptr_t)p.pos | (uintptr_t)p.w_t | (uintptr_t)p.b_t | (uintptr_t)p.aux_g | (uintptr_t)p.aux_b |
                  (uintptr_t)p.gate | (uintptr_t)p.b_v | (uintptr_t)p.basisc | (uintptr_t)p.scale |
                  (uintptr_t)mark_dev_or_null | (uintptr_t)q_coeff_dev_or_null | (uintptr_t)q_bias_dev_or_null) & 3) == 0,
                "ftn_embed_add: every operand must be 4-byte aligned");
  AddArgs a;
  a.p = p;
  a.mark = p.pos ? mark_dev_or_null : nullptr;
  a.qc = q_coeff_dev_or_null; a.qb = q_bias_dev_or_null;
  a.mark_bs = mark_bstride; a.qc_bs = q_coeff_bstride; a.qb_bs = q_bias_bstride;
  a.out = out_dev; a.Ba = Ba; a.L = L; a.D = D; a.R = R;
  const unsigned mis = (unsigned)(((uintptr_t)p.pos | (uintptr_t)(a.mark ? p.b_t : nullptr) | (uintptr_t)p.gate |
                                   (uintptr_t)p.aux_g | (uintptr_t)p.aux_b | (uintptr_t)(p.pos ? p.b_v : nullptr) |
                                   (uintptr_t)q_coeff_dev_or_null | (uintptr_t)q_bias_dev_or_null) & 15);
  const int form = embed_add_form(D, q_coeff_bstride, q_bias_bstride, mis);
  const dim3 grid((unsigned)(((long long)Ba * L + 3) / 4)), block(256);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = form & FTN_SHELL_VEC;
  if (((form >> 4) & 15) == 1) {
    if (vec) hipLaunchKernelGGL((k_embed_add<1, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_embed_add<1, false>), grid, block, 0, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_embed_add<2, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_embed_add<2, false>), grid, block, 0, st, a);
  }
  FTN_CHECK_LAUNCH();
  return 0;
}
