// Time projection of TimesNet.forward between the block stack and the heads (forecast_time_proj, reference
// models/timesnet.py:2063-2066):   hidden[b][s][:] = b_t[s] + sum_l W_t[s][l] seq[b][l][:]
//   k_timeproj_bf   S > 1: bf16x3 on the 16-bit matrix pipe (the product of k_embed_in_bf / k_head_bf)
//   k_timeproj_row  S == 1 (the recursive model): a weighted sum of L rows on the VALU
// HBM-bound by design: seq is read once (once per 96 output steps), nothing but hidden is written.  The K order of
// every output element is a function of (L, S, D) alone - no atomics, no split of K across workgroups - so row b of
// the result is the same bits in a batch of 1, of B, or as one rank's share of the batch.
// Kernels, the form rule and the launch (ftn_shell.h); the C entry points are in shell_api.hip.
#include "ftn_common.h"
#include "ftn_mlp.h"
#include "ftn_shell.h"

#define TP_WAVES 8       // waves of a k_timeproj_bf workgroup: the K-32 slabs of L are dealt to them round-robin

// MAP (the ftn_timeproj_*_forward_rows entries): seq is an item store [n_items][L][D] and batch row b reads item
// rows[b], clamped into 0 .. n_items - 1.  b comes from blockIdx, so the index is one scalar load and two scalar
// selects of a workgroup; nothing else of a kernel changes, and hidden stays [B][S][D].  The instantiations without
// MAP are the kernels as they were.
template <bool MAP>
__device__ __forceinline__ const float* tp_seq_row(const TimeProjArgs& a, int b) {
  return a.seq + (size_t)(MAP ? store_row(a.rows, a.n_items, b) : (long long)b) * a.L * a.D;
}

// The contraction runs over the ROW axis of seq, so neither operand of hidden[b] = W_t seq[b] has its K index
// contiguous in the lane that needs it.  MFMA sums over (q, e) pairwise and does not care which l a pair stands for,
// and a lane may feed different MFMAs from different components of one load: lane (j, q) loads the 16 bytes
// seq[b][l0 + 8 q + e][64 g + 4 j .. + 3] for e = 0..7 (every load instruction covers four whole 256-byte rows) and
// component c of the eight loads is the B operand of product c, whose column j is d = 64 g + 4 j + c.  The A operand
// is W_t as it lies: lane (i, q) holds W_t[s0 + i][l0 + 8 q .. + 7].  Accumulator c of lane (j, q) is then
// hidden[s0 + 4 q + r][64 g + 4 j + c], r = 0..3: the four products give one 16-byte store per output row.
//
// A workgroup owns (batch row b, 64-column group g, up to 16 NST output steps); its TP_WAVES waves take slab
// w, w + TP_WAVES, ... of L each, keep all NST x 4 accumulator tiles in registers, split their seq slab once and
// each W_t fragment once (W_t comes from L2: S L floats per workgroup beside the 64 L of seq), and the partial sums
// meet in LDS, one 16-step tile at a time, summed in wave order.  WV: W_t is read with 16-byte loads.
template <int NST, bool WV, bool MAP>
__global__ __launch_bounds__(64 * TP_WAVES, 2) void k_timeproj_bf(TimeProjArgs a) {
  __shared__ f4 red[TP_WAVES * 4 * 64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
  const int DG = (a.D + 63) >> 6;
  const int b = blockIdx.x / DG, g = blockIdx.x - b * DG;
  const int s0 = blockIdx.y * (16 * NST);
  const int d = 64 * g + 4 * j;
  const bool dok = d < a.D;                                     // D % 4 == 0: a quad is all inside a row or all outside
  const float* __restrict__ sp = tp_seq_row<MAP>(a, b) + d;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  auto load_x = [&](int sl, f4 (&x)[8]) {
    const int l0 = 32 * sl + 8 * q;
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = dok && l0 + e < a.L ? *(const f4*)(sp + (size_t)(l0 + e) * a.D) : zero;
  };
  f4 acc[NST][4];
#pragma unroll
  for (int t = 0; t < NST; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[t][c] = zero;
  const int nsl = (a.L + 31) >> 5;
  f4 xc[8], xn[8];
  if (wave < nsl) load_x(wave, xc);
  for (int sl = wave; sl < nsl; sl += TP_WAVES) {
    load_x(sl + TP_WAVES, xn);                                  // (zeros past L)
    bf8 xq[4][3];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float v[8] = {xc[0][c], xc[1][c], xc[2][c], xc[3][c], xc[4][c], xc[5][c], xc[6][c], xc[7][c]};
      split_pieces<3>(v, xq[c]);
    }
    const int l0 = 32 * sl + 8 * q;
#pragma unroll
    for (int t = 0; t < NST; ++t) {
      const int s = s0 + 16 * t + j;
      float v[8];
      if (WV) {                                                 // L % 4 == 0, base 16-byte aligned
        const float* __restrict__ wp = a.wt + (size_t)s * a.L + l0;
        const f4 v0 = s < a.S && l0 < a.L ? *(const f4*)wp : zero;
        const f4 v1 = s < a.S && l0 + 4 < a.L ? *(const f4*)(wp + 4) : zero;
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = v0[e]; v[4 + e] = v1[e]; }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = s < a.S && l0 + e < a.L ? a.wt[(size_t)s * a.L + l0 + e] : 0.f;
      }
      bf8 wq[3];
      split_pieces<3>(v, wq);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[t][c] = chain_bf<3>(wq, xq[c], acc[t][c]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) xc[e] = xn[e];
  }
  // the partial sums of the TP_WAVES slab sets, one tile of 16 steps at a time, added in wave order; then the bias
#pragma unroll
  for (int t = 0; t < NST; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      red[(wave * 4 + r) * 64 + lane] = f4{acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r]};
    __syncthreads();
    if (threadIdx.x < 256) {
      const int r = threadIdx.x >> 6;                           // (lane, j, q as above: threadIdx.x & 63)
      f4 sum = red[r * 64 + lane];
#pragma unroll
      for (int w = 1; w < TP_WAVES; ++w) sum = sum + red[(w * 4 + r) * 64 + lane];
      const int s = s0 + 16 * t + 4 * q + r;
      if (s < a.S && dok) {
        const float bias = a.bt[s];
        sum = sum + f4{bias, bias, bias, bias};
        __builtin_nontemporal_store(sum, (f4*)(a.hid + ((size_t)b * a.S + s) * a.D + d));
      }
    }
    __syncthreads();
  }
}

// One output row per batch row: a workgroup owns batch row b.  Thread (c, g) walks rows l = g, g + G, ... of seq[b]
// for the four columns 4 c .. 4 c + 3 with fp32 FMAs (G = 512 / (D / 4) row groups: a load instruction covers whole
// rows), W_t's row is staged in LDS 2048 entries at a time with 4-byte loads, and the G partial sums are added in
// group order.  G depends on D alone, so the order over l is fixed by (L, D).
#define TP_ROW_THREADS 512
#define TP_ROW_CHUNK 2048
template <bool MAP>
__global__ __launch_bounds__(TP_ROW_THREADS) void k_timeproj_row(TimeProjArgs a) {
  __shared__ float wl[TP_ROW_CHUNK];
  __shared__ f4 red[TP_ROW_THREADS];
  const int C = a.D >> 2, G = TP_ROW_THREADS / C;               // C <= 32: G >= 16
  const int c = threadIdx.x % C, g = threadIdx.x / C;
  const bool active = g < G;
  const float* __restrict__ sp = tp_seq_row<MAP>(a, (int)blockIdx.x) + 4 * c;
  f4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int l0 = 0; l0 < a.L; l0 += TP_ROW_CHUNK) {
    const int n = a.L - l0 < TP_ROW_CHUNK ? a.L - l0 : TP_ROW_CHUNK;
    for (int i = threadIdx.x; i < n; i += TP_ROW_THREADS) wl[i] = a.wt[l0 + i];
    __syncthreads();
    if (active) {
#pragma unroll 4
      for (int l = g; l < n; l += G) {
        const f4 v = *(const f4*)(sp + (size_t)(l0 + l) * a.D);
        const float w = wl[l];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(w, v[k], acc[k]);
      }
    }
    __syncthreads();
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < C) {
    f4 sum = red[threadIdx.x];
    for (int gg = 1; gg < G; ++gg) sum = sum + red[gg * C + threadIdx.x];
    const float bias = a.bt[0];
    *(f4*)(a.hid + (size_t)blockIdx.x * a.D + 4 * threadIdx.x) = sum + f4{bias, bias, bias, bias};
  }
}

// The form ftn_timeproj_forward takes (include/flowtimes.h): the one place the choice is made - the launch below
// dispatches on this value and ftn_timeproj_form exports it.  S == 1 is the row form (0).  Otherwise NST, the 16-step
// tiles a wave accumulates, is the smallest of 1, 2, 4, 6 that covers S (6 x 4 accumulator tiles are 96 registers:
// two waves per SIMD); beyond 96 steps gridDim.y walks chunks of 96 and seq is read once per chunk.
int timeproj_form(int L, int S, unsigned wt_misalign) {
  if (S == 1) return 0;
  const int tiles = (S + 15) / 16;
  const int nst = tiles <= 1 ? 1 : tiles <= 2 ? 2 : tiles <= 4 ? 4 : 6;
  const bool wv = L % 4 == 0 && (wt_misalign & 15) == 0;
  return FTN_SHELL_BF | (wv ? FTN_SHELL_VEC : 0) | nst << 4 | TP_WAVES << 8;
}

template <int NST, bool MAP>
static int launch_timeproj_bf(const TimeProjArgs& a, int form, hipStream_t st) {
  const dim3 grid((unsigned)((long long)a.B * ((a.D + 63) / 64)), (unsigned)((a.S + 16 * NST - 1) / (16 * NST)));
  if (form & FTN_SHELL_VEC) hipLaunchKernelGGL((k_timeproj_bf<NST, true, MAP>), grid, dim3(64 * TP_WAVES), 0, st, a);
  else hipLaunchKernelGGL((k_timeproj_bf<NST, false, MAP>), grid, dim3(64 * TP_WAVES), 0, st, a);
  FTN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// 128 < d_model <= 512 (ftn_timeproj_wide_forward)
// ---------------------------------------------------------------------------------------------
// k_timeproj_bf tiles d_model in 64-column groups and is launched as it is.  The row form needs D / 4 <= 32 threads a
// row group, so S == 1 gets a form of its own: a workgroup owns (batch row b, 128-column slab blockIdx.y), thread
// (c, g) walks rows l = g, g + 16, ... of the slab's columns 4 c .. 4 c + 3 and the 16 partial sums are added in group
// order.  The group count is fixed, so the order over l depends on L alone.
template <bool MAP>
__global__ __launch_bounds__(TP_ROW_THREADS) void k_timeproj_row_wide(TimeProjArgs a) {
  __shared__ float wl[TP_ROW_CHUNK];
  __shared__ f4 red[TP_ROW_THREADS];
  constexpr int C = 32, G = TP_ROW_THREADS / C;
  const int c = threadIdx.x % C, g = threadIdx.x / C;
  const int d = 128 * blockIdx.y + 4 * c;
  const bool active = d < a.D;                                  // D % 4 == 0: a quad is all inside a row or all outside
  const float* __restrict__ sp = tp_seq_row<MAP>(a, (int)blockIdx.x) + d;
  f4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int l0 = 0; l0 < a.L; l0 += TP_ROW_CHUNK) {
    const int n = a.L - l0 < TP_ROW_CHUNK ? a.L - l0 : TP_ROW_CHUNK;
    for (int i = threadIdx.x; i < n; i += TP_ROW_THREADS) wl[i] = a.wt[l0 + i];
    __syncthreads();
    if (active) {
#pragma unroll 4
      for (int l = g; l < n; l += G) {
        const f4 v = *(const f4*)(sp + (size_t)(l0 + l) * a.D);
        const float w = wl[l];
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(w, v[k], acc[k]);
      }
    }
    __syncthreads();
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < C && active) {
    f4 sum = red[threadIdx.x];
    for (int gg = 1; gg < G; ++gg) sum = sum + red[gg * C + threadIdx.x];
    const float bias = a.bt[0];
    *(f4*)(a.hid + (size_t)blockIdx.x * a.D + d) = sum + f4{bias, bias, bias, bias};
  }
}

// S == 1 is the row form of the width (form 0 at either); k_timeproj_bf serves both widths.  MAP: a.rows is set.
template <bool MAP>
static int timeproj_launch_as(const TimeProjArgs& a, const ShellWidth& w, hipStream_t st) {
  const int form = timeproj_form(a.L, a.S, (unsigned)((uintptr_t)a.wt & 15));
  if (!(form & FTN_SHELL_BF)) {
    if (w.wide) hipLaunchKernelGGL(k_timeproj_row_wide<MAP>, dim3((unsigned)a.B, (unsigned)((a.D + 127) / 128)), dim3(TP_ROW_THREADS), 0, st, a);
    else hipLaunchKernelGGL(k_timeproj_row<MAP>, dim3((unsigned)a.B), dim3(TP_ROW_THREADS), 0, st, a);
    FTN_CHECK_LAUNCH();
    return 0;
  }
  switch ((form >> 4) & 15) {
    case 1: return launch_timeproj_bf<1, MAP>(a, form, st);
    case 2: return launch_timeproj_bf<2, MAP>(a, form, st);
    case 4: return launch_timeproj_bf<4, MAP>(a, form, st);
    default: return launch_timeproj_bf<6, MAP>(a, form, st);
  }
}

int timeproj_launch(const TimeProjArgs& a, const ShellWidth& w, hipStream_t st) {
  return a.rows ? timeproj_launch_as<true>(a, w, st) : timeproj_launch_as<false>(a, w, st);
}
