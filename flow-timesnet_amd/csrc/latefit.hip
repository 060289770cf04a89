// The late-bias head for a refit of the output side (include/flowtimes.h, "late-bias refit").  For one series row
// r = (bc, n) with c = rows[r][:ctx] - the frozen output of context_norm -
//   xh = (c - mean) rstd      z = xh gamma + beta      u[s] = W[s] . z + b[s]      late[bc][s][n] = gate[s] u[s]
//   k_late_fit_forward   one wave a row: k_context_rows' late section on stored rows, through ftn_ctxrow.h, so the
//                        bits are those of ftn_context_rows for the same row and parameters
//   k_late_bwd_rows      one wave a row: z, u again; Gs = d_pre (summed over the batch, b ascending, in the wide
//                        layout); du = gate Gs; dz = du^T W, one chain in s order.  The row's z, du, Gs u, dz and dz xh
//                        go to the workspace
//   k_late_bwd_mfma      a wave owns a [32 s x 32 k] tile of a chunk's partial [S][ctx + 1] (column ctx, the bias, is
//                        du times a column of ones), K = the chunk's rows, on v_mfma_f32_32x32x2_f32: a bitwise fmaf
//                        chain, no operand is split.  The workgroups behind the tiles add 64 columns each of Gs u, dz
//                        and dz xh over the chunk's rows, one chain in row order
//   k_late_bwd_reduce    adds the chunks' partials in ascending order into dW, db, dgate, dbeta, dgamma
// Rows are cut into chunks of LF_CHUNK, at most FTN_LATEFIT_CHUNKS_MAX of them (beyond that the chunk grows, to an even
// number of rows).  No atomics; every sum's order is a function of the sizes alone and every word of the workspace
// that is read was written by this call.  rows may be an item store read through a row list (store_row: clamped).
#include "ftn_common.h"
#include "ftn_ctxrow.h"

#define LF_CHUNK 256

struct LateArgs {
  const float* rows;          // [Bc N][ctx]; with list: the item store [n_items][ctx]
  const long long* list;      // null, or [Bc N]: row r reads item list[r] clamped into 0 .. n_items - 1
  long long n_items;
  const float *ln_g, *ln_b, *w, *b, *gate;
  float eps;
  int Bc, N, ctx, S;
  float* late;                // forward: [Bc][S][N]
  const float* dpre;          // backward: [B][S][N]
  int B, chunk, chunks;
  float *zs, *du, *gu, *dz, *dzx;   // workspace: [R][ctx], [R][S], [R][S], [R][ctx], [R][ctx]
  float* part;                // workspace: [chunks][S (ctx + 1) + S + 2 ctx]
  float *dgamma, *dbeta, *dw, *db, *dgate;
};

__device__ __forceinline__ size_t late_item(const LateArgs& a, long long row) {
  return (size_t)(a.list ? store_row(a.list, a.n_items, (int)row) : row);
}

__global__ __launch_bounds__(64) void k_late_fit_forward(LateArgs a) {
  __shared__ float xs[CTX_MAX];
  const int lane = threadIdx.x;
  const long long row = blockIdx.x;
  const long long bc = row / a.N;
  const int n = (int)(row - bc * a.N);
  const float* __restrict__ cp = a.rows + late_item(a, row) * a.ctx;
  float c[CTX_SLOTS];
#pragma unroll
  for (int j = 0; j < CTX_SLOTS; ++j) c[j] = lane + 64 * j < a.ctx ? cp[lane + 64 * j] : 0.f;
  wave_layernorm(c, a.ctx, lane, a.ln_g, a.ln_b, a.eps);
#pragma unroll
  for (int j = 0; j < CTX_SLOTS; ++j)
    if (lane + 64 * j < a.ctx) xs[lane + 64 * j] = c[j];
  __syncthreads();
  for (int s = lane; s < a.S; s += 64) {
    const float v = a.gate[s] * (dot_chain(a.w + (size_t)s * a.ctx, xs, a.ctx) + a.b[s]);
    a.late[((size_t)bc * a.S + s) * a.N + n] = v;
  }
}

// The row's share of the backward.  The LayerNorm is wave_layernorm's arithmetic with xh kept.
__global__ __launch_bounds__(64) void k_late_bwd_rows(LateArgs a) {
#pragma clang fp contract(off)                                   // only the chains written as fmaf are fused
  __shared__ float xs[CTX_MAX];
  const int lane = threadIdx.x, ctx = a.ctx, S = a.S;
  const long long row = blockIdx.x;
  const long long bc = row / a.N;
  const int n = (int)(row - bc * a.N);
  const float* __restrict__ cp = a.rows + late_item(a, row) * ctx;
  float xh[CTX_SLOTS];
  float s0 = 0.f;
#pragma unroll
  for (int j = 0; j < CTX_SLOTS; ++j) {
    xh[j] = lane + 64 * j < ctx ? cp[lane + 64 * j] : 0.f;
    if (lane + 64 * j < ctx) s0 += xh[j];
  }
  const float mean = wave_sum(s0) / (float)ctx;
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < CTX_SLOTS; ++j)
    if (lane + 64 * j < ctx) {
      xh[j] -= mean;
      ss = fmaf(xh[j], xh[j], ss);
    }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)ctx + a.eps);
#pragma unroll
  for (int j = 0; j < CTX_SLOTS; ++j) {
    const int k = lane + 64 * j;
    if (k < ctx) {
      xh[j] = xh[j] * rstd;
      const float z = fmaf(xh[j], a.ln_g[k], a.ln_b[k]);
      xs[k] = z;
      a.zs[(size_t)row * ctx + k] = z;
    }
  }
  __syncthreads();
  float* du_row = a.du + (size_t)row * S;
  for (int s = lane; s < S; s += 64) {
    const float u = dot_chain(a.w + (size_t)s * ctx, xs, ctx) + a.b[s];
    float gs;
    if (a.Bc == 1) {                                              // the wide layout: one block of rows serves the batch
      gs = 0.f;
      for (int b = 0; b < a.B; ++b) gs += a.dpre[((size_t)b * S + s) * a.N + n];
    } else {
      gs = a.dpre[((size_t)bc * S + s) * a.N + n];
    }
    du_row[s] = a.gate[s] * gs;
    a.gu[(size_t)row * S + s] = gs * u;
  }
  __syncthreads();                                                // du_row: written by this workgroup, read below
#pragma unroll
  for (int j = 0; j < CTX_SLOTS; ++j) {
    const int k = lane + 64 * j;
    if (k < ctx) {
      float acc = 0.f;
      for (int s = 0; s < S; ++s) acc = fmaf(du_row[s], a.w[(size_t)s * ctx + k], acc);
      a.dz[(size_t)row * ctx + k] = acc;
      a.dzx[(size_t)row * ctx + k] = acc * xh[j];
    }
  }
}

// One wave.  blockIdx.x < tiles: tile (ts, tk) of chunk blockIdx.y, A[i = s][k = row] = du, B[k = row][j] = z (1 at
// j == ctx).  Behind the tiles: 64 columns of [Gs u | dz | dz xh], a chain over the chunk's rows.
__global__ __launch_bounds__(64) void k_late_bwd_mfma(LateArgs a) {
  const int ctx = a.ctx, S = a.S, W = ctx + 1, ktiles = (W + 31) >> 5, tiles = ((S + 31) >> 5) * ktiles;
  const int lane = threadIdx.x;
  const long long R = (long long)a.Bc * a.N;
  const long long r0 = (long long)blockIdx.y * a.chunk, r1 = r0 + a.chunk < R ? r0 + a.chunk : R;
  const size_t per = (size_t)S * W + S + 2 * (size_t)ctx;
  float* out = a.part + (size_t)blockIdx.y * per;
  if ((int)blockIdx.x >= tiles) {
    const int col = ((int)blockIdx.x - tiles) * 64 + lane;
    if (col >= S + 2 * ctx) return;
    const float* __restrict__ src = col < S ? a.gu + col : col < S + ctx ? a.dz + (col - S) : a.dzx + (col - S - ctx);
    const int ld = col < S ? S : ctx;
    float acc = 0.f;
    for (long long r = r0; r < r1; ++r) acc += src[(size_t)r * ld];
    out[(size_t)S * W + col] = acc;
    return;
  }
  const int ts = blockIdx.x / ktiles, tk = blockIdx.x - ts * ktiles;
  const int kh = lane >> 5, s = ts * 32 + (lane & 31), k = tk * 32 + (lane & 31);
  const bool sok = s < S, kok = k < ctx;
  const float one = k == ctx ? 1.f : 0.f;
  f16v c;
#pragma unroll
  for (int e = 0; e < 16; ++e) c[e] = 0.f;
  for (long long r = r0 + kh; r < r1 + kh; r += 2) {              // both halves of the wave take every step
    const bool rok = r < r1;
    const float x = rok && sok ? a.du[(size_t)r * S + s] : 0.f;
    const float y = rok ? (kok ? a.zs[(size_t)r * ctx + k] : one) : 0.f;
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, c, 0, 0, 0);
  }
  // C/D: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  if (k < W) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int ss = ts * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh;
      if (ss < S) out[(size_t)ss * W + k] = c[e];
    }
  }
}

__global__ __launch_bounds__(256) void k_late_bwd_reduce(LateArgs a) {
  const int ctx = a.ctx, S = a.S, W = ctx + 1;
  const long long per = (long long)S * W + S + 2 * (long long)ctx, i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  float v = 0.f;
  for (int c = 0; c < a.chunks; ++c) v += a.part[(size_t)c * per + i];
  if (i < (long long)S * W) {
    const int s = (int)(i / W), k = (int)(i - (long long)s * W);
    if (k == ctx) a.db[s] = v;
    else a.dw[(size_t)s * ctx + k] = v;
    return;
  }
  const int col = (int)(i - (long long)S * W);
  if (col < S) a.dgate[col] = v;
  else if (col < S + ctx) a.dbeta[col - S] = v;
  else a.dgamma[col - S - ctx] = v;
}

// The shape rule of both entries and the form ftn_late_backward takes: the one place the choice is made.
static bool late_shape_ok(int Bc, int N, int ctx, int S) {
  return Bc >= 1 && N >= 1 && (long long)Bc * N <= 0x7fffffffLL && ctx >= 1 && ctx <= CTX_MAX && S >= 1 &&
         (long long)Bc * N * S <= 0x7fffffffffLL && (long long)S * (ctx + 1) <= 0x3fffffffLL;
}
static bool late_bwd_shape_ok(int B, int Bc, int N, int ctx, int S) {
  return late_shape_ok(Bc, N, ctx, S) && B >= 1 && (Bc == 1 || Bc == B) && (long long)B * N * S <= 0x7fffffffffLL;
}
static int late_bwd_chunk(long long R) {
  long long c = LF_CHUNK;
  if ((R + c - 1) / c > FTN_LATEFIT_CHUNKS_MAX) {
    c = (R + FTN_LATEFIT_CHUNKS_MAX - 1) / FTN_LATEFIT_CHUNKS_MAX;
    c += c & 1;
  }
  return (int)c;
}
static int late_bwd_form(long long R) {
  const int chunk = late_bwd_chunk(R);
  return FTN_LATEFIT_MFMA | (int)((R + chunk - 1) / chunk) << 4;
}
static size_t late_bwd_per(int ctx, int S) { return (size_t)S * (ctx + 1) + S + 2 * (size_t)ctx; }
static size_t late_bwd_row_floats(int ctx, int S) { return 2 * (size_t)S + 3 * (size_t)ctx; }

extern "C" int ftn_late_backward_form(int B, int Bc, int N, int ctx, int S) {
  FTN_CHECK_ARG(late_bwd_shape_ok(B, Bc, N, ctx, S),
                "ftn_late_backward_form: B=%d Bc=%d (1 or B) N=%d ctx=%d (1..%d) S=%d", B, Bc, N, ctx, CTX_MAX, S);
  return late_bwd_form((long long)Bc * N);
}

extern "C" size_t ftn_late_backward_workspace(int B, int Bc, int N, int ctx, int S) {
  if (!late_bwd_shape_ok(B, Bc, N, ctx, S)) return 0;
  const long long R = (long long)Bc * N;
  return ((size_t)R * late_bwd_row_floats(ctx, S) + (size_t)(late_bwd_form(R) >> 4) * late_bwd_per(ctx, S)) * sizeof(float);
}

static int late_common(const char* who, LateArgs& a, const float* rows_dev, long long n_items,
                       const long long* list_dev_or_null, int Bc, int N, int ctx, int S, const float* ln_g_dev,
                       const float* ln_b_dev, float eps, const float* w_dev, const float* b_dev, const float* gate_dev) {
  FTN_CHECK_ARG(rows_dev && ln_g_dev && ln_b_dev && w_dev && b_dev && gate_dev, "%s: null pointer", who);
  FTN_CHECK_ARG(late_shape_ok(Bc, N, ctx, S), "%s: Bc=%d N=%d ctx=%d (1..%d) S=%d", who, Bc, N, ctx, CTX_MAX, S);
  FTN_CHECK_ARG(!list_dev_or_null || n_items >= 1, "%s: n_items=%lld must be >= 1", who, n_items);
  FTN_CHECK_ARG(((uintptr_t)list_dev_or_null & 7) == 0, "%s: the row list must be 8-byte aligned", who);
  FTN_CHECK_ARG((((uintptr_t)rows_dev | (uintptr_t)ln_g_dev | (uintptr_t)ln_b_dev | (uintptr_t)w_dev | (uintptr_t)b_dev |
                  (uintptr_t)gate_dev) & 3) == 0, "%s: every fp32 operand must be 4-byte aligned", who);
  FTN_CHECK_ARG(eps == eps, "%s: eps is NaN", who);
  a.rows = rows_dev; a.list = list_dev_or_null; a.n_items = list_dev_or_null ? n_items : (long long)Bc * N;
  a.ln_g = ln_g_dev; a.ln_b = ln_b_dev; a.w = w_dev; a.b = b_dev; a.gate = gate_dev; a.eps = eps;
  a.Bc = Bc; a.N = N; a.ctx = ctx; a.S = S;
  a.late = nullptr; a.dpre = nullptr; a.B = 0; a.chunk = 0; a.chunks = 0;
  a.zs = a.du = a.gu = a.dz = a.dzx = a.part = nullptr;
  a.dgamma = a.dbeta = a.dw = a.db = a.dgate = nullptr;
  return 0;
}

extern "C" int ftn_late_fit_forward(const float* rows_dev, long long n_items, const long long* list_dev_or_null, int Bc,
                                    int N, int ctx, int S, const float* ln_g_dev, const float* ln_b_dev, float eps,
                                    const float* w_dev, const float* b_dev, const float* gate_dev, float* late_dev,
                                    void* stream) {
  const char* who = "ftn_late_fit_forward";
  LateArgs a;
  if (int rc = late_common(who, a, rows_dev, n_items, list_dev_or_null, Bc, N, ctx, S, ln_g_dev, ln_b_dev, eps, w_dev,
                           b_dev, gate_dev))
    return rc;
  FTN_CHECK_ARG(late_dev && ((uintptr_t)late_dev & 3) == 0, "%s: late is null or off the 4-byte grid", who);
  a.late = late_dev;
  hipLaunchKernelGGL(k_late_fit_forward, dim3((unsigned)((long long)Bc * N)), dim3(64), 0, (hipStream_t)stream, a);
  FTN_CHECK_LAUNCH();
  return 0;
}

extern "C" int ftn_late_backward(const float* d_pre_dev, int B, const float* rows_dev, long long n_items,
                                 const long long* list_dev_or_null, int Bc, int N, int ctx, int S,
                                 const float* ln_g_dev, const float* ln_b_dev, float eps, const float* w_dev,
                                 const float* b_dev, const float* gate_dev, float* d_ln_g_dev, float* d_ln_b_dev,
                                 float* dw_dev, float* db_dev, float* dgate_dev, void* workspace_dev,
                                 size_t workspace_bytes, void* stream) {
  const char* who = "ftn_late_backward";
  LateArgs a;
  if (int rc = late_common(who, a, rows_dev, n_items, list_dev_or_null, Bc, N, ctx, S, ln_g_dev, ln_b_dev, eps, w_dev,
                           b_dev, gate_dev))
    return rc;
  FTN_CHECK_ARG(late_bwd_shape_ok(B, Bc, N, ctx, S), "%s: B=%d Bc=%d: Bc must be 1 or B", who, B, Bc);
  FTN_CHECK_ARG(d_pre_dev && d_ln_g_dev && d_ln_b_dev && dw_dev && db_dev && dgate_dev && workspace_dev,
                "%s: null pointer", who);
  FTN_CHECK_ARG((((uintptr_t)d_pre_dev | (uintptr_t)d_ln_g_dev | (uintptr_t)d_ln_b_dev | (uintptr_t)dw_dev |
                  (uintptr_t)db_dev | (uintptr_t)dgate_dev | (uintptr_t)workspace_dev) & 3) == 0,
                "%s: every fp32 operand and the workspace must be 4-byte aligned", who);
  const long long R = (long long)Bc * N;
  const int form = late_bwd_form(R);
  a.dpre = d_pre_dev; a.B = B; a.chunk = late_bwd_chunk(R); a.chunks = form >> 4;
  const size_t per = late_bwd_per(ctx, S);
  const size_t need = ((size_t)R * late_bwd_row_floats(ctx, S) + (size_t)a.chunks * per) * sizeof(float);
  FTN_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed (ftn_late_backward_workspace)", who,
                workspace_bytes, need);
  float* ws = (float*)workspace_dev;
  a.zs = ws;  ws += (size_t)R * ctx;
  a.du = ws;  ws += (size_t)R * S;
  a.gu = ws;  ws += (size_t)R * S;
  a.dz = ws;  ws += (size_t)R * ctx;
  a.dzx = ws; ws += (size_t)R * ctx;
  a.part = ws;
  a.dgamma = d_ln_g_dev; a.dbeta = d_ln_b_dev; a.dw = dw_dev; a.db = db_dev; a.dgate = dgate_dev;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_late_bwd_rows, dim3((unsigned)R), dim3(64), 0, st, a);
  FTN_CHECK_LAUNCH();
  const int tiles = ((S + 31) / 32) * ((ctx + 1 + 31) / 32), colblocks = (S + 2 * ctx + 63) / 64;
  hipLaunchKernelGGL(k_late_bwd_mfma, dim3((unsigned)(tiles + colblocks), (unsigned)a.chunks), dim3(64), 0, st, a);
  FTN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_late_bwd_reduce, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, st, a);
  FTN_CHECK_LAUNCH();
  return 0;
}
