// Backward of the time projection (timeproj.hip) for a refit of the output side: with dH [B][S][D] the gradient of the
// loss in hidden (ftn_head_backward's d_hidden, the loss scale already in it) and seq [B][L][D] the block stack's output,
//   dW_t[s][l] = sum_b sum_d dH[b][s][d] seq[b][l][d]        db_t[s] = sum_b sum_d dH[b][s][d]
// A GEMM with M = S, N = L, K = B D whose K index d is contiguous in both operands, which is how MFMA operands lie:
// no transpose, no LDS.
//   k_timeproj_bwd_mfma    a workgroup owns a [32 s x 32 l] tile of the chunk's partial [S][L + 1] (column L, the bias,
//                          is dH times a column of ones), K = the (b, d) pairs of the chunk's batch rows, on
//                          v_mfma_f32_32x32x2_f32: a bitwise fmaf chain, no operand is split
//   k_timeproj_bwd_reduce  adds the chunks' partials in a fixed order into dW_t and db_t
// Batch rows are cut into chunks of TPB_CHUNK, at most FTN_TIMEPROJ_BWD_CHUNKS_MAX of them (beyond that the chunk
// grows).  No atomics; the order of every sum is a function of (B, L, S, D) alone and every word of the workspace that
// is read was written by this call.  Kernels, the form rule, the launch and the C entry points.
// ftn_timeproj_backward_rows reads seq through a row list (MAP below); everything else is shared.
#include "ftn_common.h"

#define TPB_CHUNK 8          // batch rows of a chunk
#define TPB_WAVES 4          // waves of a k_timeproj_bwd_mfma workgroup: the chunk's steps are dealt to them round-robin

struct TimeProjBwdArgs {
  const float* seq;          // [B][L][D]; with rows: the item store [n_items][L][D]
  const long long* rows;     // null, or [B]: batch row b reads item rows[b] clamped into 0 .. n_items - 1
  long long n_items;
  const float* dh;           // [B][S][D]
  float* part;               // [chunks][S][L + 1]
  float* dw;  float* db;     // [S][L], [S]
  int B, L, S, D, chunk, chunks;
};

// A workgroup of TPB_WAVES waves: tile (ts, tl) of one chunk.  A[i = s][k] = dH, B[k][j = l] = seq (1 at
// l == L).  A step is 32 columns of one batch row: lane (r, kh) loads the 64 bytes d = 32 step + 16 kh .. + 15 of its
// row of dH and of its row of seq (the four loads of an operand cover 128 contiguous bytes of each of 32 rows) and
// component e of load m feeds product (m, e), whose two K slots are d = 32 step + 4 m + e and that + 16.  MFMA sums
// over k and does not care which d a slot stands for; both operands use the same map.  Wave w takes steps w,
// w + TPB_WAVES, ... of the chunk (the kernel waits on memory, not on the matrix pipe: four waves keep four times the
// loads in flight), issues the next step's loads before the 16 products, and the waves' tiles meet in LDS, added in
// wave order.
// MAP (ftn_timeproj_backward_rows): seq is an item store and the step's batch row b reads item rows[b], clamped.  A
// step is the same in every lane of a wave, which the compiler cannot see from threadIdx: readfirstlane says so, and
// the index is one scalar load and two scalar selects of a step.  A step past the chunk (its loads are masked) takes
// entry b0, so nothing is read past rows[B - 1].  The instantiation without MAP is the kernel as it was.
template <bool MAP>
__global__ __launch_bounds__(64 * TPB_WAVES) void k_timeproj_bwd_mfma(TimeProjBwdArgs a) {
  __shared__ float red[(TPB_WAVES - 1) * 16 * 64];
  const int W = a.L + 1, ltiles = (W + 31) >> 5, tiles = ((a.S + 31) >> 5) * ltiles;
  // Which (chunk, tile) a workgroup takes changes no sum, only where the operands are cached: workgroups id and
  // id + 8 have been seen to share an XCD and its L2, so with a multiple of 8 chunks every tile of a chunk goes to
  // one XCD and each batch row is fetched into one L2 instead of eight.
  int chunk, tile;
  if (a.chunks % 8 == 0) {
    const int slot = blockIdx.x >> 3;
    chunk = (blockIdx.x & 7) + 8 * (slot / tiles);
    tile = slot % tiles;
  } else {
    chunk = blockIdx.x / tiles;
    tile = blockIdx.x - chunk * tiles;
  }
  const int ts = tile / ltiles, tl = tile - ts * ltiles;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, kh = lane >> 5, r = lane & 31;
  const int s = ts * 32 + r, l = tl * 32 + r;
  const int b0 = chunk * a.chunk, b1 = b0 + a.chunk < a.B ? b0 + a.chunk : a.B;
  const int nds = (a.D + 31) >> 5, steps = (b1 - b0) * nds;
  const bool sok = s < a.S, lok = l < a.L;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  const float one = l == a.L ? 1.f : 0.f;
  const f4 fill = {one, one, one, one};                         // the bias column; dH is 0 where d is past D
  auto load = [&](int t, f4 (&x)[4], f4 (&y)[4]) {
    const int b = b0 + t / nds, d = (t % nds) * 32 + 16 * kh;
    const float* __restrict__ ap = a.dh + ((size_t)b * a.S + (sok ? s : 0)) * a.D + d;
    const float* __restrict__ bp = a.seq + ((size_t)b * a.L + (lok ? l : 0)) * a.D + d;
    if (MAP) {                                                  // the item's base and the step's column: scalars
      const int tu = __builtin_amdgcn_readfirstlane(t);
      const size_t item = (size_t)store_row(a.rows, a.n_items, tu < steps ? b0 + tu / nds : b0);
      bp = a.seq + item * a.L * a.D + (tu % nds) * 32 + ((size_t)(lok ? l : 0) * a.D + 16 * kh);
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const bool dok = t < steps && d + 4 * m < a.D;            // D % 4 == 0: a quad is all inside a row or all outside
      x[m] = sok && dok ? *(const f4*)(ap + 4 * m) : zero;
      y[m] = lok && dok ? *(const f4*)(bp + 4 * m) : fill;
    }
  };
  f16v c;
#pragma unroll
  for (int e = 0; e < 16; ++e) c[e] = 0.f;
  f4 xc[4], yc[4], xn[4], yn[4];
  load(wave, xc, yc);
  for (int t = wave; t < steps; t += TPB_WAVES) {
    load(t + TPB_WAVES, xn, yn);                                // (nothing is read past the chunk)
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_32x32x2f32(xc[m][e], yc[m][e], c, 0, 0, 0);
#pragma unroll
    for (int m = 0; m < 4; ++m) { xc[m] = xn[m]; yc[m] = yn[m]; }
  }
  if (wave > 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) red[((wave - 1) * 16 + e) * 64 + lane] = c[e];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int w = 1; w < TPB_WAVES; ++w)
#pragma unroll
    for (int e = 0; e < 16; ++e) c[e] += red[((w - 1) * 16 + e) * 64 + lane];
  // C/D: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* out = a.part + (size_t)chunk * a.S * W;
  if (l < W) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int ss = ts * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh;
      if (ss < a.S) out[(size_t)ss * W + l] = c[e];
    }
  }
}

// 16 outputs per workgroup: thread (o, cl) adds chunks cl, cl + 16, ... of output o in ascending order, then the 16
// chunk lanes are added in ascending order.
__global__ __launch_bounds__(256) void k_timeproj_bwd_reduce(TimeProjBwdArgs a) {
  __shared__ float red[16][17];
  const int W = a.L + 1, o = threadIdx.x & 15, cl = threadIdx.x >> 4;
  const long long per = (long long)a.S * W, i = (long long)blockIdx.x * 16 + o;
  float v = 0.f;
  if (i < per) {
#pragma unroll 4
    for (int c = cl; c < a.chunks; c += 16) v += a.part[(size_t)c * per + i];
  }
  red[cl][o] = v;
  __syncthreads();
  if (cl > 0 || i >= per) return;
  v = red[0][o];
#pragma unroll
  for (int k = 1; k < 16; ++k) v += red[k][o];
  const int s = (int)(i / W), l = (int)(i - (long long)s * W);
  if (l == a.L) a.db[s] = v;
  else a.dw[(size_t)s * a.L + l] = v;
}

// The form ftn_timeproj_backward takes (include/flowtimes.h): the one place the choice is made - the launch below
// dispatches on this value and ftn_timeproj_backward_form exports it.  One form.  At the pipeline shape
// ([4096, 28, 64] -> 7) the 32 x 32 tile is mostly padding, but the matrix pipe's share there is about 3.4 us of the
// 17.5 us measured (profiles/output_fit_time.json: 2.1 TB/s of seq + dH); what a small-output form would have to beat
// is the wait for the operands, which dealing the steps to TPB_WAVES waves already cut from 46.6 us, so there is no
// crossover to record.  Two by two tiles per workgroup were measured too and lost at the large shapes (DESIGN
// section 4 "Output refit").  Operands off the 16-byte grid have no form: the entry rejects them.
static int tpb_chunk(int B) {
  long long c = TPB_CHUNK;
  if ((B + c - 1) / c > FTN_TIMEPROJ_BWD_CHUNKS_MAX) c = ((long long)B + FTN_TIMEPROJ_BWD_CHUNKS_MAX - 1) / FTN_TIMEPROJ_BWD_CHUNKS_MAX;
  return (int)c;
}
static bool tpb_shape_ok(int B, int L, int S, int D) {
  return B >= 1 && L >= 1 && S >= 1 && D >= 4 && D <= 512 && D % 4 == 0 && (long long)S * ((long long)L + 1) <= 0x3fffffffLL &&
         (((long long)S + 31) / 32) * (((long long)L + 32) / 32) * FTN_TIMEPROJ_BWD_CHUNKS_MAX <= 0x7fffffffLL;   // the grid
}
static int tpb_form(int B) {
  const int chunk = tpb_chunk(B);
  return FTN_TIMEPROJ_BWD_MFMA | ((B + chunk - 1) / chunk) << 4;
}

extern "C" int ftn_timeproj_backward_form(int B, int L, int S, int D, int misalign_or) {
  FTN_CHECK_ARG(tpb_shape_ok(B, L, S, D) && misalign_ok(misalign_or),
                "ftn_timeproj_backward_form: B=%d L=%d S=%d d_model=%d misalign=%d", B, L, S, D, misalign_or);
  FTN_CHECK_ARG(misalign_or == 0, "ftn_timeproj_backward_form: seq and d_hidden must be 16-byte aligned (misalign=%d)",
                misalign_or);
  return tpb_form(B);
}

extern "C" size_t ftn_timeproj_backward_workspace(int B, int L, int S, int D) {
  if (!tpb_shape_ok(B, L, S, D)) return 0;
  return (size_t)(tpb_form(B) >> 4) * S * ((size_t)L + 1) * sizeof(float);
}

// ftn_timeproj_backward (rows_dev null, n_items = B) and ftn_timeproj_backward_rows: one set of checks, one launch.
static int tpb_entry(const char* who, bool mapped, const float* seq_dev, long long n_items, const long long* rows_dev,
                     const float* d_hidden_dev, int B, int L, int S, int D, float* dw_t_dev, float* db_t_dev,
                     void* workspace_dev, size_t workspace_bytes, void* stream) {
  FTN_CHECK_ARG(seq_dev && d_hidden_dev && dw_t_dev && db_t_dev && workspace_dev && (rows_dev || !mapped),
                "%s: null pointer", who);
  FTN_CHECK_ARG(tpb_shape_ok(B, L, S, D), "%s: B=%d L=%d S=%d d_model=%d (a multiple of 4, <= 512)", who, B, L, S, D);
  FTN_CHECK_ARG(n_items >= 1, "%s: n_items=%lld must be >= 1", who, n_items);
  FTN_CHECK_ARG(((uintptr_t)rows_dev & 7) == 0, "%s: rows must be 8-byte aligned", who);
  FTN_CHECK_ARG((((uintptr_t)seq_dev | (uintptr_t)d_hidden_dev) & 15) == 0,
                "%s: seq and d_hidden must be 16-byte aligned", who);
  FTN_CHECK_ARG((((uintptr_t)dw_t_dev | (uintptr_t)db_t_dev | (uintptr_t)workspace_dev) & 3) == 0,
                "%s: dW_t, db_t and the workspace must be 4-byte aligned", who);
  const int form = tpb_form(B);
  TimeProjBwdArgs a;
  a.seq = seq_dev; a.rows = rows_dev; a.n_items = n_items; a.dh = d_hidden_dev; a.part = (float*)workspace_dev;
  a.dw = dw_t_dev; a.db = db_t_dev;
  a.B = B; a.L = L; a.S = S; a.D = D; a.chunk = tpb_chunk(B); a.chunks = form >> 4;
  const size_t need = (size_t)a.chunks * S * ((size_t)L + 1) * sizeof(float);
  FTN_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed (ftn_timeproj_backward_workspace)", who,
                workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(((S + 31) / 32) * ((L + 1 + 31) / 32)) * (unsigned)a.chunks);
  if (mapped) hipLaunchKernelGGL(k_timeproj_bwd_mfma<true>, grid, dim3(64 * TPB_WAVES), 0, st, a);
  else hipLaunchKernelGGL(k_timeproj_bwd_mfma<false>, grid, dim3(64 * TPB_WAVES), 0, st, a);
  FTN_CHECK_LAUNCH();
  const long long per = (long long)S * (L + 1);
  hipLaunchKernelGGL(k_timeproj_bwd_reduce, dim3((unsigned)((per + 15) / 16)), dim3(256), 0, st, a);
  FTN_CHECK_LAUNCH();
  return 0;
}

extern "C" int ftn_timeproj_backward(const float* seq_dev, const float* d_hidden_dev, int B, int L, int S, int D,
                                     float* dw_t_dev, float* db_t_dev, void* workspace_dev, size_t workspace_bytes,
                                     void* stream) {
  return tpb_entry("ftn_timeproj_backward", false, seq_dev, B > 0 ? B : 1, nullptr, d_hidden_dev, B, L, S, D, dw_t_dev,
                   db_t_dev, workspace_dev, workspace_bytes, stream);
}

extern "C" int ftn_timeproj_backward_rows(const float* seq_dev, long long n_items, const long long* rows_dev,
                                          const float* d_hidden_dev, int B, int L, int S, int D, float* dw_t_dev,
                                          float* db_t_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
  return tpb_entry("ftn_timeproj_backward_rows", true, seq_dev, n_items, rows_dev, d_hidden_dev, B, L, S, D, dw_t_dev,
                   db_t_dev, workspace_dev, workspace_bytes, stream);
}
