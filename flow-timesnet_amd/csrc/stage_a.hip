// Stage A of the TimesBlock conv path (block.hip) and the small row-wise helpers: the generic pointwise kernel k_pw
// (stage A, and the generic stage-C chain for widths beyond the fused kernels), its fusion with the selector's
// finalize (k_finalize_pw), the single-conv embed and the standalone residual + LayerNorm.
#include "ftn_pw.h"
#include "ftn_mlp.h"

#define NPXU 4  // 16-pixel units per wave in the pointwise kernels

// Copies the caller's descriptor to the head of the workspace; a descriptor that exceeds the bounds the
// workspace and the grids were sized for (more groups than max_groups, more pixels than px_bound) is
// replaced by an empty one, which makes the call the identity y = x instead of a write past a buffer.
__device__ __forceinline__ void guard_desc(const FtnDesc* __restrict__ src, FtnDesc* __restrict__ dst, int max_groups,
                                           int px_bound) {
  const int* s = (const int*)src;
  int* d = (int*)dst;
  const bool bad = src->n_groups < 0 || src->n_groups > max_groups || src->total_px < 0 || src->total_px > px_bound;
  for (int e = threadIdx.x; e < (int)(sizeof(FtnDesc) / 4); e += blockDim.x) d[e] = bad ? 0 : s[e];
  if (threadIdx.x == 0) d[sizeof(FtnDesc) / 4] = bad ? 1 : 0;
}

// ---------------------------------------------------------------- stage A and the generic pointwise layers
// out[n][:] = epilogue( W in[n][:] + b )  on exact fp32 MFMA, any number of output tiles and any K.
//   XIN 0: in = buffer [N][KIN] per grid pixel      XIN 1: in = x by window row (stage A, see below)
//   XIN 2: in = x by grid pixel (zero rows for the live pad pixels t >= L)
//   EPI 0: store fp32      EPI 2 / 3: store three bf16 / two fp16 pieces (input of the split conv engines)
//   EPI 4: store v - x[n]  (r = res2(g) - x)      EPI 5: store act(v)      EPI 6: out = act(v + out)  (in place)
// Stage A always runs here; EPI 4-6 with XIN 0 / 2 form the generic stage C for widths beyond the fused
// kernels' limits (more than 16 output tiles, or a hidden chunk's fragments not fitting LDS twice).
template <int ACT, int XIN, bool XVEC, int EPI>
__device__ __forceinline__ void pw_body(const PwArgs& a, const int bid) {
  // XIN 1 (stage A): a = W_in1 x + b depends on (b, t) only, not on the period group, so it is computed once per
  // window position - rows n = b*L + t of `out` - plus ONE pad row n = B*L for the live zero pixels t >= L of
  // every grid (x = 0 there, :1017, so a = bias).  The conv stage folds these rows into its period grids while
  // staging (ConvArgs.bt_L), which is the reference's reshape (:1041-1046) done by index arithmetic.
  const FtnDesc* __restrict__ d = a.desc;
  if (XIN == 1 && bid == 0 && a.guard_dst != nullptr) guard_desc(a.guard_src, a.guard_dst, a.guard_groups, a.guard_px);
  const int N = XIN == 1 ? a.B * a.L + 1 : a.B * d->total_px;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
  const int n0 = (bid * 4 + wave) * (16 * NPXU);
  if (n0 >= N) return;
  Px px[NPXU];
#pragma unroll
  for (int u = 0; u < NPXU; ++u) {
    if (XIN == 1) {
      const int n = n0 + 16 * u + j;
      px[u].ok = n < N;
      px[u].n = px[u].ok ? n : N - 1;
      px[u].xrow = px[u].n < N - 1 ? a.x + (size_t)px[u].n * a.C : nullptr;
    } else {
      px[u] = decode_px16(d, a.x, a.B, a.L, a.C, n0 + 16 * u, j, N);
    }
  }
  const int KIN = a.KIN;
  bool range_bad = false;
  for (int og = 0; og < a.n_ot; og += 4) {
    f4 acc[4][NPXU];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      f4 bv = {0.f, 0.f, 0.f, 0.f};
      if (og + o < a.n_ot) bv = *(const f4*)(a.bias + 16 * (og + o) + 4 * q);
#pragma unroll
      for (int u = 0; u < NPXU; ++u) acc[o][u] = bv;
    }
    // operands of K step s + 16 are requested before the products of step s (every load used to sit right in front of
    // its MFMAs: at d_model 128 stage A ran at a fifth of the fp32 pipe's rate)
    auto load_step = [&](int s, f4 (&bf)[NPXU], f4 (&af)[4]) {
#pragma unroll
      for (int u = 0; u < NPXU; ++u) {
        if (XIN != 0) bf[u] = load_x4<XVEC>(px[u].xrow, s + 4 * q, a.C);
        else bf[u] = *(const f4*)(a.in + (size_t)px[u].n * KIN + s + 4 * q);
      }
#pragma unroll
      for (int o = 0; o < 4; ++o)
        af[o] = og + o < a.n_ot ? *(const f4*)(a.W + (size_t)(16 * (og + o) + j) * KIN + s + 4 * q) : f4{0.f, 0.f, 0.f, 0.f};
    };
    f4 bfc[NPXU], afc[4];
    load_step(0, bfc, afc);
    for (int s = 0; s < KIN; s += 16) {
      f4 bfn[NPXU], afn[4];
      const bool more = s + 16 < KIN;
      if (more) load_step(s + 16, bfn, afn);
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        if (og + o < a.n_ot) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int u = 0; u < NPXU; ++u) acc[o][u] = mfma16(afc[o][e], bfc[u][e], acc[o][u]);
        }
      }
      if (more) {
#pragma unroll
        for (int u = 0; u < NPXU; ++u) bfc[u] = bfn[u];
#pragma unroll
        for (int o = 0; o < 4; ++o) afc[o] = afn[o];
      }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      if (og + o < a.n_ot) {
#pragma unroll
        for (int u = 0; u < NPXU; ++u) {
          if (!px[u].ok) continue;
          const int ch = 16 * (og + o) + 4 * q;
          float* op = a.out + (size_t)px[u].n * a.OUTC + ch;
          if (EPI == 0) {
            *(f4*)op = acc[o][u];
          } else if (EPI == 2 || EPI == 3) {   // bf16x3 (P3) / f16x2 (H2) pieces: input of the split conv engines
            constexpr int NSP = EPI == 3 ? 2 : 3;
            if (EPI == 3) range_bad |= h2_bad4(acc[o][u]);
            store_px<NSP>((__bf16*)a.out + ((size_t)px[u].n * (a.OUTC >> 4) + (og + o)) * PxFmt<NSP>::ELEMS, q, acc[o][u]);
          } else if (EPI == 4) {
            *(f4*)op = acc[o][u] - load_x4<XVEC>(px[u].xrow, ch, a.C);
          } else if (EPI == 5) {
            *(f4*)op = act4<ACT>(acc[o][u]);
          } else {
            *(f4*)op = act4<ACT>(acc[o][u] + *(const f4*)op);
          }
        }
      }
    }
  }
  if (EPI == 3) raise_range_flag(a.range_flag, range_bad);
}

template <int ACT, int XIN, bool XVEC, int EPI>
__global__ __launch_bounds__(256) void k_pw(PwArgs a) { pw_body<ACT, XIN, XVEC, EPI>(a, (int)blockIdx.x); }

// Stage A has no use for the selector's result, and the selector ends in a one-workgroup kernel (k_finalize, ~17 us
// of serial latency with 255 CUs idle): this launch runs both - workgroup 0 is k_finalize (and then publishes the
// sanitised descriptor copy at the head of the workspace), workgroups 1.. are stage A - so stage A's ~22 us
// disappear behind the selector's tail (ftn_period_finalize_stage_a).
#include "ftn_finalize.h"
// part: 0 = both (workgroup 0 finalizes, the others run stage A), 1 = stage A only (a sharded batch runs it while
// the partial sums are exchanged), 2 = finalize + descriptor copy only (one workgroup, after that exchange)
template <int ACT, bool XVEC, int EPI>
__global__ __launch_bounds__(256) void k_finalize_pw(FinalizeArgs fa, PwArgs pa, int part) {
  if (part != 1 && blockIdx.x == 0) {
    finalize_body(fa);
    __syncthreads();
    guard_desc(fa.desc, pa.guard_dst, pa.guard_groups, pa.guard_px);
  } else if (part != 2) {
    PwArgs q = pa;
    q.guard_dst = nullptr;
    pw_body<ACT, 1, XVEC, EPI>(q, (int)blockIdx.x - (part == 0 ? 1 : 0));
  }
}

// Elementwise pieces of the generic stage C when a res_proj is the identity (d_ff == d_model):
//   mode 0: g = act(g + x)      mode 1: r = g - x      (rows = grid pixels, CH = FP = CP channels)
template <int ACT, bool XVEC>
__global__ void k_ew_ident(const float* __restrict__ x, float* __restrict__ g, float* __restrict__ r,
                           const FtnDesc* __restrict__ d, int B, int L, int C, int CH, int mode) {
  const int N = B * d->total_px;
  const int cq = CH >> 2;
  const long long total = (long long)N * cq;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(e / cq), c = (int)(e - (long long)n * cq) * 4;
    const Px px = decode_px(d, x, B, L, C, n, N);
    const f4 xv = load_x4<XVEC>(px.xrow, c, C);
    f4* gp = (f4*)(g + (size_t)n * CH + c);
    if (mode == 0) *gp = act4<ACT>(*gp + xv);
    else *(f4*)(r + (size_t)n * CH + c) = *gp - xv;
  }
}

// ---------------------------------------------------------------- small elementwise stages
// single-conv mode, stage A: a[n][CP] = zero-extended x
__global__ void k_embed(const float* __restrict__ x, float* __restrict__ out, int B, int L, int C, int CP,
                        const FtnDesc* guard_src, FtnDesc* guard_dst, int guard_groups, int guard_px) {
  if (blockIdx.x == 0) guard_desc(guard_src, guard_dst, guard_groups, guard_px);
  // rows n = b*L + t of the window, channels zero-padded to CP, plus one all-zero pad row n = B*L
  // (the live zero pixels t >= L of every period grid, :1017); the conv folds them (ConvArgs.bt_L)
  const int cq = CP >> 2;
  const long long rows = (long long)B * L + 1;
  const long long total = rows * cq;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long n = e / cq;
    const int c = (int)(e - n * cq) * 4;
    *(f4*)(out + (size_t)n * CP + c) = load_x4<false>(n < rows - 1 ? x + (size_t)n * C : nullptr, c, C);
  }
}

// Standalone form of the same epilogue for the shapes k_out does not fuse (d_model > 64) and for
// blocks that return x unchanged: out = LayerNorm_C(x + (nw - x)); one wave per row, in place allowed.
__global__ __launch_bounds__(256) void k_resid_ln(const float* __restrict__ x, const float* nw, float* out,
                                                  const float* __restrict__ g, const float* __restrict__ b,
                                                  float eps, long long rows, int C) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * C;
  const float* nr = nw + row * C;
  float* orow = out + row * C;
  constexpr int MAXV = 8;                      // channels cached in registers: C <= 512; beyond that re-read
  float v[MAXV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + 64 * i;
    v[i] = 0.f;
    if (c < C) { const float xv = xr[c]; v[i] = xv + (nr[c] - xv); s += v[i]; }
  }
  for (int c = lane + 64 * MAXV; c < C; c += 64) { const float xv = xr[c]; s += xv + (nr[c] - xv); }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) s += __shfl_xor(s, m);
  const float mean = s / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (lane + 64 * i < C) { const float dv = v[i] - mean; ss += dv * dv; }
  for (int c = lane + 64 * MAXV; c < C; c += 64) { const float xv = xr[c]; const float dv = xv + (nr[c] - xv) - mean; ss += dv * dv; }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) ss += __shfl_xor(ss, m);
  const float rstd = 1.0f / sqrtf(ss / (float)C + eps);
  // the tail (C > 512) must be produced before the cached part overwrites an in-place row
  for (int c = lane + 64 * MAXV; c < C; c += 64) { const float xv = xr[c]; orow[c] = (xv + (nr[c] - xv) - mean) * rstd * g[c] + b[c]; }
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = lane + 64 * i;
    if (c < C) orow[c] = (v[i] - mean) * rstd * g[c] + b[c];
  }
}

template <int ACT, int XIN, int EPI>
static int launch_pw(const PwArgs& pa, bool xvec, int nblk, hipStream_t st) {
  if (xvec) hipLaunchKernelGGL((k_pw<ACT, XIN, true, EPI>), dim3(nblk), dim3(256), 0, st, pa);
  else hipLaunchKernelGGL((k_pw<ACT, XIN, false, EPI>), dim3(nblk), dim3(256), 0, st, pa);
  FTN_CHECK_LAUNCH();
  return 0;
}

// the (XIN, EPI) pairs that exist: stage A (1: 0 / 2 / 3) and the generic stage-C chain (0: 0 / 2 / 3 / 4 / 5, 2: 6)
static int launch_pw_any(const PwArgs& pa, int act, int xin, int epi, bool xvec, int nblk, hipStream_t st) {
#define FTN_PW_CASE(XIN, EPI) \
  if (xin == XIN && epi == EPI) return act == 1 ? launch_pw<1, XIN, EPI>(pa, xvec, nblk, st) : launch_pw<0, XIN, EPI>(pa, xvec, nblk, st);
  FTN_PW_CASE(1, 0) FTN_PW_CASE(1, 2) FTN_PW_CASE(1, 3)
  FTN_PW_CASE(0, 0) FTN_PW_CASE(0, 2) FTN_PW_CASE(0, 3) FTN_PW_CASE(0, 4) FTN_PW_CASE(0, 5) FTN_PW_CASE(2, 6)
#undef FTN_PW_CASE
  ftn_set_error("k_pw: no form for xin=%d epi=%d", xin, epi);
  return -1;
}

// S3-S5 of the selector and stage A of the block in ONE launch (k_finalize_pw): see flowtimes.h
template <int ACT, bool XVEC>
static int launch_finalize_pw(const FinalizeArgs& fa, const PwArgs& pa, int epi, int nblk_pw, int part, hipStream_t st) {
  const dim3 grid(part == 0 ? 1 + nblk_pw : (part == 1 ? nblk_pw : 1)), blk(256);
  const size_t lds = ftn_finalize_lds_bytes(fa.F);
  if (epi == 3) hipLaunchKernelGGL((k_finalize_pw<ACT, XVEC, 3>), grid, blk, lds, st, fa, pa, part);
  else if (epi == 2) hipLaunchKernelGGL((k_finalize_pw<ACT, XVEC, 2>), grid, blk, lds, st, fa, pa, part);
  else hipLaunchKernelGGL((k_finalize_pw<ACT, XVEC, 0>), grid, blk, lds, st, fa, pa, part);
  FTN_CHECK_LAUNCH();
  return 0;
}

int ftn_launch_stage_a(const PwArgs& pa, const FinalizeArgs* fa, int part, int act, int epi, bool xvec, hipStream_t st) {
  const int nblk_pw = (int)(((long long)pa.B * pa.L + 1 + 16 * NPXU * 4 - 1) / (16 * NPXU * 4));   // window rows + pad row
  if (fa == nullptr) return launch_pw_any(pa, act, 1, epi, xvec, nblk_pw, st);
  // a launch that finalizes (part 0 / 2) leaves the per-row section of a large batch to k_row_weights behind it
  FinalizeArgs f = *fa;
  f.rows_outside = part != 1 && ftn_fin_rows_outside(f.B) ? 1 : 0;
  int rc;
  if (act == 1) rc = xvec ? launch_finalize_pw<1, true>(f, pa, epi, nblk_pw, part, st) : launch_finalize_pw<1, false>(f, pa, epi, nblk_pw, part, st);
  else rc = xvec ? launch_finalize_pw<0, true>(f, pa, epi, nblk_pw, part, st) : launch_finalize_pw<0, false>(f, pa, epi, nblk_pw, part, st);
  if (rc == 0 && f.rows_outside) rc = ftn_launch_row_weights(f, st);
  return rc;
}

static int launch_ew_ident(const PwArgs& pg, float* G, float* R, int CH, int mode, int act, bool xvec, hipStream_t st) {
  const dim3 grid(2048), blk(256);
  if (act == 1 && xvec) hipLaunchKernelGGL((k_ew_ident<1, true>), grid, blk, 0, st, pg.x, G, R, pg.desc, pg.B, pg.L, pg.C, CH, mode);
  else if (act == 1) hipLaunchKernelGGL((k_ew_ident<1, false>), grid, blk, 0, st, pg.x, G, R, pg.desc, pg.B, pg.L, pg.C, CH, mode);
  else if (xvec) hipLaunchKernelGGL((k_ew_ident<0, true>), grid, blk, 0, st, pg.x, G, R, pg.desc, pg.B, pg.L, pg.C, CH, mode);
  else hipLaunchKernelGGL((k_ew_ident<0, false>), grid, blk, 0, st, pg.x, G, R, pg.desc, pg.B, pg.L, pg.C, CH, mode);
  FTN_CHECK_LAUNCH();
  return 0;
}

// wide blocks: the chain as pointwise launches with the hidden tensor g in the workspace
//   g1 = act(W_out1 m + b);  g = act(g1 + res1(x));  a' = W_in2 g + b;  r = res2(g) - x
int ftn_launch_stagec_generic(PwArgs pg, const FtnPlan* pl, const float* wb, float* G, long long Nmax, int act, int epi, bool xvec,
                              hipStream_t st) {
  const int CA = pl->nbr * pl->MP, CP = pl->CP, FP = pl->FP;
  const int nblk_px = (int)((Nmax + 16 * NPXU * 4 - 1) / (16 * NPXU * 4));
  float* const outA = pg.out;
  float* const R = pg.R;
  int rc;
  pg.R = nullptr;
  pg.W = wb + pl->w_out1; pg.bias = wb + pl->b_out1; pg.out = G; pg.KIN = CA; pg.n_ot = FP / 16; pg.OUTC = FP;
  if ((rc = launch_pw_any(pg, act, 0, 5, xvec, nblk_px, st))) return rc;
  if (pl->res1) {
    pg.in = nullptr; pg.W = wb + pl->w_res1; pg.bias = wb + pl->b_res1; pg.KIN = CP;
    if ((rc = launch_pw_any(pg, act, 2, 6, xvec, nblk_px, st))) return rc;
  } else if ((rc = launch_ew_ident(pg, G, R, FP, 0, act, xvec, st))) return rc;
  pg.in = G; pg.W = wb + pl->w_in2; pg.bias = wb + pl->b_in2; pg.out = outA; pg.KIN = FP; pg.n_ot = CA / 16; pg.OUTC = CA;
  if ((rc = launch_pw_any(pg, act, 0, epi, xvec, nblk_px, st))) return rc;
  if (pl->res2) {
    pg.W = wb + pl->w_res2; pg.bias = wb + pl->b_res2; pg.out = R; pg.n_ot = CP / 16; pg.OUTC = CP;
    return launch_pw_any(pg, act, 0, 4, xvec, nblk_px, st);
  }
  return launch_ew_ident(pg, G, R, FP, 1, act, xvec, st);
}

int ftn_launch_embed(const PwArgs& pa, int CP, hipStream_t st) {
  hipLaunchKernelGGL(k_embed, dim3(2048), dim3(256), 0, st, pa.x, pa.out, pa.B, pa.L, pa.C, CP, pa.guard_src, pa.guard_dst,
                     pa.guard_groups, pa.guard_px);
  FTN_CHECK_LAUNCH();
  return 0;
}

int ftn_launch_resid_ln(const float* x, const float* nw, float* out, const float* g, const float* b, float eps, long long rows,
                        int C, hipStream_t st) {
  hipLaunchKernelGGL(k_resid_ln, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, nw, out, g, b, eps, rows, C);
  FTN_CHECK_LAUNCH();
  return 0;
}
