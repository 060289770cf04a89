// Model-shell kernels for 128 < d_model <= 512 (the narrow ones, d_model <= 128, are in shell.hip):
//   k_embed_wide_bf    value embedding GEMM + add (+ LayerNorm over d_model), the row spread over the waves of a workgroup
//   k_embed_wide_ring  the embedding of a sliding window from a ring of stored x W^T rows
//   k_head_wide_bf     rate / dispersion heads, contraction over d_model, split weights of both heads in LDS
//   k_head_wide_f32    the heads for operands that are not vectorisable (plain fp32 FMAs)
// Products are bf16x3 on the 16-bit matrix pipe (split_pieces<3> / chain_bf<3>, ftn_mlp.h), the arithmetic class of
// the narrow forms.  No atomics on outputs, no split of K across workgroups: the bits of an output row are a function
// of its own operands, (N, D) and the form.
// Kernels, form rules and one launch per operation (ftn_shell.h); the C entry points are in shell_api.hip.
#include <stdlib.h>
#include "ftn_common.h"
#include "ftn_mlp.h"
#include "ftn_shell.h"

// ---------------------------------------------------------------------------------------------
// Value embedding: out[b][l][:] = x[b][l][:] W^T + add[b?][l][:]   (+ optional LayerNorm over d_model)
// ---------------------------------------------------------------------------------------------
// A workgroup of four waves owns RT tiles of 16 rows and sees their whole output row: wave w takes the column slab
// [16 NO w, 16 NO (w + 1)) of d_model - NO = 4 column tiles of 16 (64-column slabs) up to d_model 256, NO = 8
// (128-column slabs) beyond; a wave whose slab starts past d_model only stages x and takes part in the barriers.  Lane
// (j, q) of wave w ends up with columns 16 NO w + 16 o + 4 q .. + 3 of row j in tile o, the layout of the narrow
// kernels inside a slab.
#define EW_RT 4

// + add, optional LayerNorm over one row spread over the waves of a workgroup, for the GEMM epilogue and for the ring
// epilogue alike: a row assembled from stored x W^T plus `add` comes out bit-identical to the one-pass embedding.  The
// partial sums of a slab are formed in the lane and across its four q-lanes, then the slabs are added in slab order
// through LDS (red: [2][4][16] floats) - first the mean, then the centred sum of squares; a slab past d_model adds an
// exact zero.  Contraction into FMAs is off: the two callers must not round differently.  Every wave of the workgroup
// calls it (two barriers with LayerNorm).
// RMS (FTN_NORM_RMS): (v * rsqrt(mean(v^2) + eps)) * gamma + beta as embed_row_finish (shell.hip) has it, one
// reduction - the sum of squares, slabs in slab order - and so one barrier.  With a single barrier a call may no longer
// reuse the words its predecessor read: a wave can be writing its partial sum of the next row tile while another
// still adds up this one's.  `half` picks the half of red[] the call goes through; successive calls of a workgroup
// alternate it (a wave that writes half h again has passed the barrier of the call in between, which every wave
// reaches only after its reads of h).
template <int NO>
__device__ __forceinline__ void embed_wide_row_finish(f4 (&v)[NO], const float* __restrict__ ap, const float* ln_g,
                                                      const float* ln_b, float ln_eps, int D, int wave, int j, int q,
                                                      float* red, int norm, int half) {
#pragma clang fp contract(off)
  constexpr int nw = 4;
  const float invD = 1.0f / (float)D;
  const int c0 = 16 * NO * wave + 4 * q;
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    const int cb = c0 + 16 * o;
    if (ap && cb < D) v[o] = v[o] + *(const f4*)(ap + cb);      // D % 4 == 0
  }
  if (norm == FTN_NORM_RMS) {
    float* rd = red + 64 * half;
    float ss = 0.f;
#pragma unroll
    for (int o = 0; o < NO; ++o)
      if (c0 + 16 * o < D) ss += (v[o][0] * v[o][0] + v[o][1] * v[o][1]) + (v[o][2] * v[o][2] + v[o][3] * v[o][3]);
    ss += __shfl_xor(ss, 16);
    ss += __shfl_xor(ss, 32);
    if (q == 0) rd[16 * wave + j] = ss;
    __syncthreads();
    float tot = rd[j];
    for (int w = 1; w < nw; ++w) tot += rd[16 * w + j];
    const float scale = 1.0f / sqrtf(tot * invD + ln_eps);
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const int cb = c0 + 16 * o;
      if (cb < D) v[o] = (v[o] * scale) * *(const f4*)(ln_g + cb) + *(const f4*)(ln_b + cb);
    }
  } else if (ln_g) {
    float s = 0.f;
#pragma unroll
    for (int o = 0; o < NO; ++o)
      if (c0 + 16 * o < D) s += (v[o][0] + v[o][1]) + (v[o][2] + v[o][3]);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (q == 0) red[16 * wave + j] = s;
    __syncthreads();
    float tot = red[j];
    for (int w = 1; w < nw; ++w) tot += red[16 * w + j];
    const float mean = tot * invD;
    float ss = 0.f;
#pragma unroll
    for (int o = 0; o < NO; ++o)
      if (c0 + 16 * o < D) {
        const f4 dv = v[o] - mean;
        ss += (dv[0] * dv[0] + dv[1] * dv[1]) + (dv[2] * dv[2] + dv[3] * dv[3]);
      }
    ss += __shfl_xor(ss, 16);
    ss += __shfl_xor(ss, 32);
    if (q == 0) red[64 + 16 * wave + j] = ss;
    __syncthreads();
    float tot2 = red[64 + j];
    for (int w = 1; w < nw; ++w) tot2 += red[64 + 16 * w + j];
    const float rstd = 1.0f / sqrtf(tot2 * invD + ln_eps);
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const int cb = c0 + 16 * o;
      if (cb < D) v[o] = (v[o] - mean) * rstd * *(const f4*)(ln_g + cb) + *(const f4*)(ln_b + cb);
    }
  }
}

// K (= series) is walked in slabs of 32.  The x fragment of a slab (B operand: lane (j, q) holds k = 8 q .. + 7 of row
// j) is loaded from HBM and split once per workgroup - by wave t for row tile t - and shared through LDS, one slab
// ahead; every wave loads the W rows of its own column slab (A operand, from L2: W is D N floats for the whole grid)
// one slab ahead and splits a tile's fragment just before its products.  VEC: 16-byte loads of x and W (N % 4 == 0,
// batch stride % 4 == 0, both bases aligned); otherwise guarded 4-byte loads, the same arithmetic.
template <int NO, int RT, bool VEC>
__global__ __launch_bounds__(256) void k_embed_wide_bf(EmbedArgs a) {
  constexpr int KC = 32;
  __shared__ bf8 xs[2][RT][3][64];
  __shared__ float red[2 * 4 * 16];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
  const long long M = (long long)a.B * a.L;
  const long long row0 = (long long)blockIdx.x * (16 * RT);
  const int cw = 16 * NO * wave;                                // first column of this wave's slab
  const int rest = a.D - cw;
  const int nto = rest >= 16 * NO ? NO : rest <= 0 ? 0 : (rest + 15) >> 4;   // column tiles of the slab inside d_model
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  auto load8 = [&](const float* __restrict__ p, int k, f4 (&v)[2]) {
    if (VEC) {
      v[0] = k < a.N ? *(const f4*)(p + k) : zero;
      v[1] = k + 4 < a.N ? *(const f4*)(p + k + 4) : zero;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[0][e] = k + e < a.N ? p[k + e] : 0.f;
        v[1][e] = k + 4 + e < a.N ? p[k + 4 + e] : 0.f;
      }
    }
  };
  // the x rows this wave stages: row tile `wave` (RT <= 4 waves)
  const bool xload = wave < RT;
  const float* xrow;
  {
    const long long row = row0 + 16 * (xload ? wave : 0) + j;
    const long long r = row < M ? row : M - 1;
    const long long b = r / a.L;
    xrow = a.x + b * a.x_bs + (r - b * a.L) * a.N;
  }
  auto store_x = [&](int buf, const f4 (&xr)[2]) {
    const float v[8] = {xr[0][0], xr[0][1], xr[0][2], xr[0][3], xr[1][0], xr[1][1], xr[1][2], xr[1][3]};
    bf8 pc[3];
    split_pieces<3>(v, pc);
#pragma unroll
    for (int pz = 0; pz < 3; ++pz) xs[buf][wave][pz][lane] = pc[pz];
  };
  auto load_w = [&](int kc, f4 (&wv)[NO][2]) {
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const int col = cw + 16 * o + j;
      wv[o][0] = zero; wv[o][1] = zero;
      if (col < a.D) load8(a.W + (size_t)col * a.N, kc + 8 * q, wv[o]);
    }
  };
  f4 acc[RT][NO];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[t][o] = zero;
  f4 wc[NO][2], wn[NO][2], xr[2];
  const int nch = (a.N + KC - 1) / KC;
  if (xload) {
    load8(xrow, 8 * q, xr);
    store_x(0, xr);
  }
  load_w(0, wc);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const int buf = c & 1;
    const bool more = c + 1 < nch;
    if (more) {
      if (xload) load8(xrow, (c + 1) * KC + 8 * q, xr);
      load_w((c + 1) * KC, wn);
    }
    bf8 xq[RT][3];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int pz = 0; pz < 3; ++pz) xq[t][pz] = xs[buf][t][pz][lane];
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      if (o < nto) {
        const float v[8] = {wc[o][0][0], wc[o][0][1], wc[o][0][2], wc[o][0][3], wc[o][1][0], wc[o][1][1], wc[o][1][2], wc[o][1][3]};
        bf8 wf[3];
        split_pieces<3>(v, wf);
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[t][o] = chain_bf<3>(wf, xq[t], acc[t][o]);
      }
    }
    if (more) {
      if (xload) store_x(buf ^ 1, xr);
#pragma unroll
      for (int o = 0; o < NO; ++o) { wc[o][0] = wn[o][0]; wc[o][1] = wn[o][1]; }
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const long long row = row0 + 16 * t + j;
    const bool rok = row < M;
    const long long r = rok ? row : M - 1;
    const long long b = r / a.L, l = r - b * a.L;
    const float* __restrict__ ap = a.add ? a.add + b * a.add_bs + l * a.D : nullptr;
    embed_wide_row_finish<NO>(acc[t], ap, a.ln_g, a.ln_b, a.ln_eps, a.D, wave, j, q, red, a.norm, t & 1);
    if (!rok) continue;
    float* __restrict__ op = a.out + b * a.out_bs + l * a.D;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const int cb = cw + 16 * o + 4 * q;
      if (cb < a.D) *(f4*)(op + cb) = acc[t][o];
    }
  }
}

// The form the wide embedding entry points take (include/flowtimes.h): the one place the choice is made - the launch
// dispatches on this value and ftn_embed_wide_form exports it.  misalign: the OR of the byte offsets of x and W.
int embed_wide_form(int N, int D, long long x_bs, unsigned misalign) {
  const bool vec = N % 4 == 0 && x_bs % 4 == 0 && (misalign & 15) == 0;
  return FTN_SHELL_BF | (vec ? FTN_SHELL_VEC : 0) | (D <= 256 ? 4 : 8) << 4 | EW_RT << 8;
}

int embed_wide_launch(const EmbedArgs& a, hipStream_t st) {
  const int form = embed_wide_form(a.N, a.D, a.x_bs, (unsigned)(((uintptr_t)a.x | (uintptr_t)a.W) & 15));
  const long long M = (long long)a.B * a.L;
  const dim3 grid((unsigned)((M + 16 * EW_RT - 1) / (16 * EW_RT))), block(256);
  const bool vec = form & FTN_SHELL_VEC;
  if (((form >> 4) & 15) == 4) {
    if (vec) hipLaunchKernelGGL((k_embed_wide_bf<4, EW_RT, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_embed_wide_bf<4, EW_RT, false>), grid, block, 0, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_embed_wide_bf<8, EW_RT, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_embed_wide_bf<8, EW_RT, false>), grid, block, 0, st, a);
  }
  FTN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Ring epilogue: out[b][t][:] = finish(V[b][(head + t) mod L][:] + add[b?][t][:])   (+ LayerNorm)
// ---------------------------------------------------------------------------------------------
// One memory-bound pass: a workgroup owns 16 rows, wave w the column slab w, with the lane layout and the epilogue
// function of k_embed_wide_bf<NO, ...>.
template <int NO>
__global__ __launch_bounds__(256, 2) void k_embed_wide_ring(RingArgs a) {
  __shared__ float red[2 * 4 * 16];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
  const long long M = (long long)a.B * a.L;
  const long long row = (long long)blockIdx.x * 16 + j;
  const bool ok = row < M;
  const long long r = ok ? row : M - 1;            // rows past the end still take part in the row reductions
  const long long b = r / a.L;
  const int t = (int)(r - b * a.L);
  int slot = a.head + t;
  if (slot >= a.L) slot -= a.L;
  const float* __restrict__ vp = a.V + (b * a.L + slot) * a.D;
  const int c0 = 16 * NO * wave + 4 * q;
  f4 v[NO];
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    const int cb = c0 + 16 * o;
    v[o] = *(const f4*)(vp + (cb < a.D ? cb : a.D - 4));      // (columns past d_model are never used)
  }
  const float* __restrict__ ap = a.add ? a.add + b * a.add_bs + (long long)t * a.D : nullptr;
  embed_wide_row_finish<NO>(v, ap, a.ln_g, a.ln_b, a.ln_eps, a.D, wave, j, q, red, a.norm, 0);
  if (!ok) return;
  float* __restrict__ op = a.out + r * a.D;
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    const int cb = c0 + 16 * o;
    if (cb < a.D) *(f4*)(op + cb) = v[o];
  }
}

int ring_wide_launch(const RingArgs& a, hipStream_t st) {
  const long long M = (long long)a.B * a.L;
  const dim3 grid((unsigned)((M + 15) / 16));
  if (a.D <= 256) hipLaunchKernelGGL(k_embed_wide_ring<4>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_embed_wide_ring<8>, grid, dim3(256), 0, st, a);
  FTN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Rate / dispersion heads
// ---------------------------------------------------------------------------------------------
// The epilogue of four series n .. n + 3 of one row, shared by both wide kernels: + bias + history tail (+ late bias),
// softplus20, floor, the finite-positive flags and the stores - the arithmetic of k_head / k_head_bf (shell.hip).
// tp / lp point at series n of the row's tail / late-bias row (lp null: none).  Returns the bad bits.
template <bool VEC>
__device__ __forceinline__ int head_wide_finish(const HeadArgs& a, f4 mu, f4 sg, f4 bm, f4 bs, f4 fl,
                                                const float* __restrict__ tp, const float* __restrict__ lp,
                                                long long row, int n, bool rok) {
  f4 tv = {0.f, 0.f, 0.f, 0.f}, lv = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    if (n < a.N) {
      tv = *(const f4*)tp;
      if (lp) lv = *(const f4*)lp;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n + r < a.N) {
        tv[r] = tp[r];
        if (lp) lv[r] = lp[r];
      }
  }
  f4 pre = mu + bm + tv;                                  // mu_head(hidden) + history tail (:2079)
  if (lp) pre = pre + lv;                                 // + gate * late_bias (:2080-2090)
  int badbits = 0;
  f4 rt, dp;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    rt[r] = softplus20(pre[r]) + 1e-6f;                   // :2091
    dp[r] = softplus20(sg[r] + bs[r]) + fl[r] + 1e-6f;    // :2092-2094
    if (rok && n + r < a.N) {
      if (!(rt[r] > 0.f && rt[r] <= 3.4028234664e38f)) badbits |= 1;
      if (!(dp[r] > 0.f && dp[r] <= 3.4028234664e38f)) badbits |= 2;
    }
  }
  if (!rok) return badbits;
  float* __restrict__ rp = a.rate + row * a.N + n;
  float* __restrict__ dq = a.disp + row * a.N + n;
  if (VEC) {
    if (n < a.N) {
      __builtin_nontemporal_store(rt, (f4*)rp);
      __builtin_nontemporal_store(dp, (f4*)dq);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n + r < a.N) { rp[r] = rt[r]; dq[r] = dp[r]; }
  }
  if (a.sig_mu) {                                           // the refit's forward keeps softplus' derivatives
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (n + r < a.N) {
        a.sig_mu[row * a.N + n + r] = sigmoid20(pre[r]);
        a.sig_sg[row * a.N + n + r] = sigmoid20(sg[r] + bs[r]);
      }
  }
  return badbits;
}

// A workgroup owns NT tiles of 16 series.  Both weight slices are split into three bf16 pieces once and sit in LDS as
// K-32 A fragments ([head][tile][slab][piece][lane] x 16 B: 6 KB per tile and slab, ceil(D / 32) slabs - 96 KB at
// d_model 512 with NT = 1 and at d_model 256 with NT = 2).  A wave walks 16-row tiles of `hidden` and splits its
// rows slab by slab inside the K loop (B operand: lane (j, q) holds k = 32 S + 8 q .. + 7 of row j), the next slab's
// 32 bytes requested one slab ahead.  An element's K order is slab order: it depends on D alone.
template <int NT>
__global__ __launch_bounds__(256) void k_head_wide_bf(HeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) char hl[];     // [2][NT][ns32][3][64] bf8 | 3 x [16 NT] fp32
  bf8* __restrict__ wl = (bf8*)hl;
  constexpr int NW = 16 * NT;                                   // series per workgroup
  const int ns32 = (a.D + 31) >> 5;
  const int n0 = blockIdx.x * NW;
  const f4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int f = threadIdx.x; f < 2 * NT * ns32 * 64; f += 256) {
    const int ln = f & 63;
    int t = f >> 6;
    const int S = t % ns32;
    t /= ns32;
    const int o = t % NT, h = t / NT, i = ln & 15, qa = ln >> 4;
    const int n = n0 + 16 * o + i, k = 32 * S + 8 * qa;
    f4 v0 = zero, v1 = zero;
    if (n < a.N) {                                              // D % 4 == 0: a quad is all inside a row or all outside
      const float* __restrict__ wp = (h ? a.wsg : a.wmu) + (size_t)n * a.D + k;
      if (k < a.D) v0 = *(const f4*)wp;
      if (k + 4 < a.D) v1 = *(const f4*)(wp + 4);
    }
    const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
    bf8 pc[3];
    split_pieces<3>(v, pc);
#pragma unroll
    for (int pz = 0; pz < 3; ++pz) wl[(((h * NT + o) * ns32 + S) * 3 + pz) * 64 + ln] = pc[pz];
  }
  // per-series constants of the slice: [0] b_mu, [1] b_sigma, [2] dispersion floor
  float* cst = (float*)(hl + (size_t)2 * NT * ns32 * 3 * 1024);
  if (threadIdx.x < 3 * NW) {
    const int which = threadIdx.x / NW, n = n0 + (threadIdx.x % NW);
    float v = which == 2 ? a.floor_s : 0.f;
    if (n < a.N) v = which == 0 ? a.bmu[n] : which == 1 ? a.bsg[n] : (a.floorv ? a.floorv[n] : a.floor_s);
    cst[threadIdx.x] = v;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
  const int nl0 = n0 + 4 * q;           // lane (j, q) of tile o holds series nl0 + 16*o .. +3 of row j
  int badbits = 0;
  for (long long t = (long long)blockIdx.y * 4 + wave; t * 16 < a.rows; t += (long long)gridDim.y * 4) {
    const long long row = t * 16 + j;
    const bool rok = row < a.rows;
    const long long rr = rok ? row : a.rows - 1;
    const long long b = rr / a.S;
    const int s = (int)(rr - b * a.S);
    const float* __restrict__ hp = a.hidden + rr * a.D + 8 * q;
    auto load_h = [&](int S, f4 (&v)[2]) {
      const int k = 32 * S + 8 * q;
      v[0] = k < a.D ? *(const f4*)(hp + 32 * S) : zero;
      v[1] = k + 4 < a.D ? *(const f4*)(hp + 32 * S + 4) : zero;
    };
    f4 am[NT], as[NT];
#pragma unroll
    for (int o = 0; o < NT; ++o) am[o] = as[o] = zero;
    f4 hc[2], hn[2];
    load_h(0, hc);
    for (int S = 0; S < ns32; ++S) {
      load_h(S + 1, hn);                                        // (zeros past D)
      const float v[8] = {hc[0][0], hc[0][1], hc[0][2], hc[0][3], hc[1][0], hc[1][1], hc[1][2], hc[1][3]};
      bf8 hq[3];
      split_pieces<3>(v, hq);
#pragma unroll
      for (int o = 0; o < NT; ++o) {
        bf8 wm[3], ws[3];
#pragma unroll
        for (int pz = 0; pz < 3; ++pz) {
          wm[pz] = wl[(((0 * NT + o) * ns32 + S) * 3 + pz) * 64 + lane];
          ws[pz] = wl[(((1 * NT + o) * ns32 + S) * 3 + pz) * 64 + lane];
        }
        am[o] = chain_bf<3>(wm, hq, am[o]);
        as[o] = chain_bf<3>(ws, hq, as[o]);
      }
      hc[0] = hn[0]; hc[1] = hn[1];
    }
    const float* __restrict__ tp = a.tail + b * a.tail_bs + (size_t)(s < a.hist ? s : a.hist - 1) * a.N + nl0;
    const float* __restrict__ lp = a.late ? a.late + b * a.late_bs + (size_t)s * a.N + nl0 : nullptr;
#pragma unroll
    for (int o = 0; o < NT; ++o) {
      const f4 bm = *(const f4*)(cst + 16 * o + 4 * q), bs = *(const f4*)(cst + NW + 16 * o + 4 * q);
      const f4 fl = *(const f4*)(cst + 2 * NW + 16 * o + 4 * q);
      badbits |= head_wide_finish<true>(a, am[o], as[o], bm, bs, fl, tp + 16 * o, lp ? lp + 16 * o : nullptr, rr,
                                        nl0 + 16 * o, rok);
    }
  }
  if (badbits) atomicOr(a.bad, badbits);
}

// The heads for operands that are not vectorisable (N % 4 != 0, a batch stride that is no multiple of 4, tail / late
// / rate / disp off a 16-byte boundary): a thread owns four series of one row and walks d_model with fp32 FMAs in k
// order (hidden and the weights are 16-byte aligned with D % 4 == 0, so those are vector loads).  Correct, not fast.
__global__ __launch_bounds__(256) void k_head_wide_f32(HeadArgs a) {
  const long long nq = (a.N + 3) >> 2, total = a.rows * nq;
  int badbits = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long row = i / nq;
    const int n = (int)(i - row * nq) * 4;
    const long long b = row / a.S;
    const int s = (int)(row - b * a.S);
    const float* __restrict__ hp = a.hidden + row * a.D;
    f4 mu = {0.f, 0.f, 0.f, 0.f}, sg = {0.f, 0.f, 0.f, 0.f}, bm = mu, bs = mu, fl = mu;
    const float* wm[4];
    const float* ws[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int nn = n + r < a.N ? n + r : a.N - 1;
      wm[r] = a.wmu + (size_t)nn * a.D;
      ws[r] = a.wsg + (size_t)nn * a.D;
      bm[r] = a.bmu[nn];
      bs[r] = a.bsg[nn];
      fl[r] = a.floorv ? a.floorv[nn] : a.floor_s;
    }
    for (int k = 0; k < a.D; k += 4) {
      const f4 h = *(const f4*)(hp + k);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const f4 m = *(const f4*)(wm[r] + k), g = *(const f4*)(ws[r] + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          mu[r] = fmaf(h[e], m[e], mu[r]);
          sg[r] = fmaf(h[e], g[e], sg[r]);
        }
      }
    }
    const float* __restrict__ tp = a.tail + b * a.tail_bs + (size_t)(s < a.hist ? s : a.hist - 1) * a.N + n;
    const float* __restrict__ lp = a.late ? a.late + b * a.late_bs + (size_t)s * a.N + n : nullptr;
    badbits |= head_wide_finish<false>(a, mu, sg, bm, bs, fl, tp, lp, row, n, true);
  }
  if (badbits) atomicOr(a.bad, badbits);
}

static size_t head_wide_lds(int nt, int D) { return (size_t)2 * nt * ((D + 31) / 32) * 3 * 1024 + 3 * 16 * nt * sizeof(float); }

// The form ftn_head_wide_forward takes (include/flowtimes.h): the one place the choice is made.  misalign: the OR of
// the byte offsets of tail, late, rate and disp from a 16-byte boundary.  The cap on gridDim.y keeps as many
// workgroups per CU in flight as their LDS allows (160 KB a CU); beyond 64 * cap rows a workgroup walks several row
// tiles.  0: k_head_wide_f32.
int head_wide_form(int N, int D, long long tail_bs, long long late_bs, unsigned misalign) {
  const bool vec = N % 4 == 0 && tail_bs % 4 == 0 && late_bs % 4 == 0 && (misalign & 15) == 0;
  if (!vec) return 0;
  const int nt = D <= 256 ? 2 : 1;
  const int ntile = (N + 16 * nt - 1) / (16 * nt);
  const int per_cu = (int)((size_t)160 * 1024 / head_wide_lds(nt, D));
  const int cap = (per_cu * 256 + ntile - 1) / ntile;
  return FTN_SHELL_BF | FTN_SHELL_VEC | nt << 4 | cap << 16;
}

template <int NT>
static int launch_head_wide_bf(const HeadArgs& a, int form, hipStream_t st) {
  const int ntile = (a.N + 16 * NT - 1) / (16 * NT);
  const unsigned gy = head_grid_y(a.rows, form);
  const size_t lds = head_wide_lds(NT, a.D);
  hipError_t e = hipFuncSetAttribute((const void*)k_head_wide_bf<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { ftn_set_error("hipFuncSetAttribute(k_head_wide_bf): %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL((k_head_wide_bf<NT>), dim3(ntile, gy), dim3(256), lds, st, a);
  FTN_CHECK_LAUNCH();
  return 0;
}

int head_wide_launch(const HeadArgs& a, hipStream_t st) {
  const int form = head_wide_form(a.N, a.D, a.tail_bs, a.late_bs,
                                  (unsigned)(((uintptr_t)a.tail | (uintptr_t)a.late | (uintptr_t)a.rate | (uintptr_t)a.disp) & 15));
  if (form & FTN_SHELL_BF) return ((form >> 4) & 15) == 2 ? launch_head_wide_bf<2>(a, form, st) : launch_head_wide_bf<1>(a, form, st);
  const long long total = a.rows * ((a.N + 3) / 4);
  long long nblk = (total + 255) / 256;
  if (nblk > 4096) nblk = 4096;                                 // grid-stride beyond
  hipLaunchKernelGGL(k_head_wide_f32, dim3((unsigned)nblk), dim3(256), 0, st, a);
  FTN_CHECK_LAUNCH();
  return 0;
}
