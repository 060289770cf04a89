// Scoring a forecast where it lies (reference losses.py:27-58 negative_binomial_nll, train.py:675-765 _eval_metrics):
//   k_score_cols<CPL>  one pass over y, rate, dispersion (and a mask): a record {nll_sum, smape_sum, nll_cnt,
//                      smape_cnt} per column (b, n), optionally the per-element log-likelihood
//   k_score_fold       adds the column records into the caller's per-slot accumulators, in place
// Every sum is fp64 and taken in an order that the shape fixes: over h ascending inside a segment of H, the
// segments in ascending order, the columns of a slot in ascending (b, n) order.  No float atomics; a column's record
// is the same bits in a batch of 1 or of B.
//
// The log-likelihood is evaluated in fp64 and rounded once: lgamma(yc + r) - lgamma(r) with r = 1 / alpha up to
// 1e8 cancels ~1e9 against ~1e9, and fp64 FMAs issue at the rate of unpacked fp32 ones on this part.  Nothing here
// calls a library lgamma or log: the three lgammas share one shift product and cost four logs between them, and
// the kernel's two other logs are log1p(alpha mu) and log1p(1 / (alpha mu)).
#include "ftn_common.h"
#include "ftn_nbmath.h"
#include <math.h>

#define SC_MAXSEG 8          // waves of a workgroup = segments of H
#define SC_MINROWS 4         // rows of a segment at least

struct ScoreArgs {
  const float* y;  const float* rate;  const float* disp;
  const void* mask;            // [B][H][N] contiguous: uint8 (mask_kind 1) or fp32 (2); null (0)
  float* ll;                   // [B][H][N] contiguous or null
  FtnScorePart* part;          // [B N]
  long long ybs, rbs, dbs;     // batch strides in elements
  float eps;
  int B, H, N, mask_kind, seg, ncols;
};

// One element.  ll: the fp32 log-likelihood (0 where invalid); term: the sMAPE term where `counts`.
__device__ inline void sc_element(float y, float rate, float disp, bool m, float eps, float& ll, bool& valid,
                                  float& term, bool& counts) {
  const float yc = y < 0.f ? 0.f : y;                           // comparisons, not fmaxf: a NaN stays a NaN
  const float al = disp < eps ? eps : disp;
  const float mu = rate < eps ? eps : rate;
  valid = m && __builtin_isfinite(yc) && __builtin_isfinite(al) && __builtin_isfinite(mu);
  counts = valid && __builtin_isfinite(y) && fabsf(y) > 1e-8f;
  ll = 0.f;
  term = 0.f;
  if (valid) {
    double l1p;                                                 // the product of two floats is exact
    const double v = sc_nb_ll((double)yc, sc_rcp((double)al), (double)al * (double)mu, l1p);
    ll = (float)v;
  }
  if (counts) {
    const float d = fabsf(rate - y), s = fabsf(y) + fabsf(rate);
    term = (2.0f * d) / s;
  }
}

template <int CPL>
__global__ __launch_bounds__(64 * SC_MAXSEG) void k_score_cols(ScoreArgs a) {
  __shared__ double s_nll[(SC_MAXSEG - 1) * 64 * CPL], s_sm[(SC_MAXSEG - 1) * 64 * CPL];
  __shared__ int s_nc[(SC_MAXSEG - 1) * 64 * CPL], s_sc[(SC_MAXSEG - 1) * 64 * CPL];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nseg = blockDim.x >> 6;
  const long long c0 = ((long long)blockIdx.x * 64 + lane) * CPL;  // first of this lane's CPL columns
  const bool active = c0 < a.ncols;                             // CPL == 4: N % 4 == 0, a quad has one b
  const int b = active ? (int)(c0 / a.N) : 0, n = active ? (int)(c0 - (long long)b * a.N) : 0;
  double nll[CPL], sm[CPL];
  int nc[CPL], sc[CPL];
#pragma unroll
  for (int k = 0; k < CPL; ++k) { nll[k] = 0.0; sm[k] = 0.0; nc[k] = 0; sc[k] = 0; }
  const int h0 = wave * a.seg, h1 = h0 + a.seg < a.H ? h0 + a.seg : a.H;
  if (active) {
    const float* __restrict__ yp = a.y + (size_t)b * a.ybs + n;
    const float* __restrict__ rp = a.rate + (size_t)b * a.rbs + n;
    const float* __restrict__ dp = a.disp + (size_t)b * a.dbs + n;
    const size_t base = (size_t)b * a.H * a.N + n;              // into mask and ll_out
    for (int h = h0; h < h1; ++h) {
      const size_t ro = (size_t)h * a.N;
      float y[CPL], rt[CPL], ds[CPL], ll[CPL];
      bool m[CPL];
      if (CPL == 4) {
        const f4 yv = *(const f4*)(yp + ro), rv = *(const f4*)(rp + ro), dv = *(const f4*)(dp + ro);
        uint32_t mb = 0x01010101u;
        f4 mf = {1.f, 1.f, 1.f, 1.f};
        if (a.mask_kind == 1) mb = *(const uint32_t*)((const uint8_t*)a.mask + base + ro);
        if (a.mask_kind == 2) mf = *(const f4*)((const float*)a.mask + base + ro);
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          y[k] = yv[k]; rt[k] = rv[k]; ds[k] = dv[k];
          m[k] = ((mb >> (8 * k)) & 0xffu) != 0 && mf[k] != 0.f;
        }
      } else {
        y[0] = yp[ro]; rt[0] = rp[ro]; ds[0] = dp[ro];
        m[0] = a.mask_kind == 1 ? ((const uint8_t*)a.mask)[base + ro] != 0
             : a.mask_kind == 2 ? ((const float*)a.mask)[base + ro] != 0.f : true;
      }
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        bool valid, counts;
        float term;
        sc_element(y[k], rt[k], ds[k], m[k], a.eps, ll[k], valid, term, counts);
        if (valid) { nll[k] -= (double)ll[k]; ++nc[k]; }
        if (counts) { sm[k] += (double)term; ++sc[k]; }
      }
      if (a.ll) {
        if (CPL == 4) __builtin_nontemporal_store(f4{ll[0], ll[1], ll[2], ll[3]}, (f4*)(a.ll + base + ro));
        else a.ll[base + ro] = ll[0];
      }
    }
  }
  // the segments' sums, added in ascending order by wave 0
  if (nseg > 1) {
    if (wave > 0) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int i = ((wave - 1) * CPL + k) * 64 + lane;
        s_nll[i] = nll[k]; s_sm[i] = sm[k]; s_nc[i] = nc[k]; s_sc[i] = sc[k];
      }
    }
    __syncthreads();
  }
  if (wave == 0 && active) {
    for (int w = 1; w < nseg; ++w) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const int i = ((w - 1) * CPL + k) * 64 + lane;
        nll[k] += s_nll[i]; sm[k] += s_sm[i]; nc[k] += s_nc[i]; sc[k] += s_sc[i];
      }
    }
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      FtnScorePart* o = a.part + c0 + k;
      o->nll_sum = nll[k]; o->smape_sum = sm[k]; o->nll_cnt = nc[k]; o->smape_cnt = sc[k];
    }
  }
}

// acc[slot] += part[col], a record at a time.  kinds 0 / 1: thread n owns slot n / ids[n] and walks b ascending.
// kind 2: thread s owns slot s and walks order[seg_start[s] .. seg_start[s + 1]), columns in ascending (b, n) order
// because the argsort was stable.
__global__ __launch_bounds__(64) void k_score_fold(const FtnScorePart* __restrict__ part, int B, int N, int kind,
                                                   const long long* __restrict__ ids,
                                                   const long long* __restrict__ order,
                                                   const long long* __restrict__ seg_start, FtnScorePart* acc,
                                                   int n_slots, int* err) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const long long ncols = (long long)B * N;
  if (kind == 2) {
    if (i == 0 && (seg_start[0] != 0 || seg_start[n_slots] != ncols)) atomicOr(err, 1);   // ids beside the slots
    if (i >= n_slots) return;
    long long lo = seg_start[i], hi = seg_start[i + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > ncols ? ncols : hi;
    if (lo >= hi) return;
    FtnScorePart s = acc[i];
#pragma unroll 8
    for (long long j = lo; j < hi; ++j) {
      const long long c = order[j];
      if (c < 0 || c >= ncols) { atomicOr(err, 1); continue; }
      const FtnScorePart p = part[c];
      s.nll_sum += p.nll_sum; s.smape_sum += p.smape_sum; s.nll_cnt += p.nll_cnt; s.smape_cnt += p.smape_cnt;
    }
    acc[i] = s;
    return;
  }
  if (i >= N) return;
  const long long slot = kind == 1 ? ids[i] : i;
  if (slot < 0 || slot >= n_slots) { atomicOr(err, 1); return; }
  FtnScorePart s = acc[slot];
#pragma unroll 16
  for (int b = 0; b < B; ++b) {
    const FtnScorePart p = part[(size_t)b * N + i];
    s.nll_sum += p.nll_sum; s.smape_sum += p.smape_sum; s.nll_cnt += p.nll_cnt; s.smape_cnt += p.smape_cnt;
  }
  acc[slot] = s;
}

// The form ftn_score_columns takes (include/flowtimes.h): the one place the choice is made.
static int score_form(int H, int N, long long ybs, long long rbs, long long dbs, unsigned misalign_or) {
  int seg = (H + SC_MAXSEG - 1) / SC_MAXSEG;
  if (seg < SC_MINROWS) seg = SC_MINROWS;
  const int nseg = (H + seg - 1) / seg;
  return (ftn_vec4_ok(N, ybs, rbs, dbs, misalign_or) ? FTN_SHELL_VEC : 0) | nseg << 4 | seg << 8;
}

extern "C" int ftn_score_form(int H, int N, long long y_bstride, long long rate_bstride, long long disp_bstride,
                              int misalign_or) {
  FTN_CHECK_ARG(H >= 1 && N >= 1 && (long long)H * N <= 0x7fffffffLL && H < (1 << 20),
                "ftn_score_form: H=%d N=%d", H, N);
  FTN_CHECK_ARG(y_bstride >= 0 && rate_bstride >= 0 && disp_bstride >= 0 && misalign_ok(misalign_or),
                "ftn_score_form: strides %lld %lld %lld misalign=%d", y_bstride, rate_bstride, disp_bstride, misalign_or);
  return score_form(H, N, y_bstride, rate_bstride, disp_bstride, (unsigned)misalign_or);
}

extern "C" int ftn_score_columns(const float* y_dev, long long y_bstride, const float* rate_dev,
                                 long long rate_bstride, const float* disp_dev, long long disp_bstride,
                                 const void* mask_dev, int mask_kind, float eps, int B, int H, int N,
                                 FtnScorePart* part_out_dev, float* ll_out_dev, void* stream) {
  FTN_CHECK_ARG(y_dev && rate_dev && disp_dev && part_out_dev, "ftn_score_columns: null pointer");
  FTN_CHECK_ARG(B >= 1 && H >= 1 && N >= 1, "ftn_score_columns: bad shape B=%d H=%d N=%d", B, H, N);
  FTN_CHECK_ARG((long long)H * N <= 0x7fffffffLL && (long long)B * N <= 0x7fffffffLL && H < (1 << 20),
                "ftn_score_columns: H N = %lld or B N = %lld beyond int32", (long long)H * N, (long long)B * N);
  const long long row = (long long)H * N;
  FTN_CHECK_ARG(B == 1 || (y_bstride >= row && rate_bstride >= row && disp_bstride >= row),
                "ftn_score_columns: batch strides %lld %lld %lld are below H N = %lld", y_bstride, rate_bstride,
                disp_bstride, row);
  FTN_CHECK_ARG(y_bstride >= 0 && rate_bstride >= 0 && disp_bstride >= 0, "ftn_score_columns: negative batch stride");
  FTN_CHECK_ARG(mask_kind >= 0 && mask_kind <= 2 && (mask_kind == 0) == (mask_dev == nullptr),
                "ftn_score_columns: mask_kind=%d does not fit the mask pointer", mask_kind);
  FTN_CHECK_ARG(eps > 0.f && eps < 1.f, "ftn_score_columns: eps=%g", (double)eps);
  FTN_CHECK_ARG((((uintptr_t)y_dev | (uintptr_t)rate_dev | (uintptr_t)disp_dev | (uintptr_t)ll_out_dev) & 3) == 0 &&
                    (mask_kind != 2 || ((uintptr_t)mask_dev & 3) == 0) && ((uintptr_t)part_out_dev & 7) == 0,
                "ftn_score_columns: operands must be 4-byte aligned, part_out 8-byte aligned");
  unsigned mis = (unsigned)(((uintptr_t)y_dev | (uintptr_t)rate_dev | (uintptr_t)disp_dev | (uintptr_t)ll_out_dev) & 15);
  if (mask_kind == 2) mis |= (unsigned)((uintptr_t)mask_dev & 15);
  if (mask_kind == 1) mis |= (unsigned)((uintptr_t)mask_dev & 3) << 2;
  const int form = score_form(H, N, B > 1 ? y_bstride : 0, B > 1 ? rate_bstride : 0, B > 1 ? disp_bstride : 0, mis);
  ScoreArgs a;
  a.y = y_dev; a.rate = rate_dev; a.disp = disp_dev; a.mask = mask_dev; a.ll = ll_out_dev; a.part = part_out_dev;
  a.ybs = B > 1 ? y_bstride : 0; a.rbs = B > 1 ? rate_bstride : 0; a.dbs = B > 1 ? disp_bstride : 0;
  a.eps = eps; a.B = B; a.H = H; a.N = N; a.mask_kind = mask_kind;
  a.seg = form >> 8; a.ncols = B * N;
  const int nseg = (form >> 4) & 15, cpl = form & FTN_SHELL_VEC ? 4 : 1;
  const dim3 grid((unsigned)(((long long)a.ncols + 64 * cpl - 1) / (64 * cpl))), block(64 * nseg);
  hipStream_t st = (hipStream_t)stream;
  if (cpl == 4) hipLaunchKernelGGL(k_score_cols<4>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(k_score_cols<1>, grid, block, 0, st, a);
  FTN_CHECK_LAUNCH();
  return 0;
}

extern "C" int ftn_score_fold(const FtnScorePart* part_dev, int B, int N, int ids_kind, const long long* ids_dev,
                              const long long* order_dev, const long long* seg_start_dev, FtnScorePart* acc_dev,
                              int n_slots, int* err_dev, void* stream) {
  FTN_CHECK_ARG(part_dev && acc_dev && err_dev, "ftn_score_fold: null pointer");
  FTN_CHECK_ARG(B >= 1 && N >= 1 && (long long)B * N <= 0x7fffffffLL, "ftn_score_fold: bad shape B=%d N=%d", B, N);
  FTN_CHECK_ARG(n_slots >= 1, "ftn_score_fold: n_slots=%d", n_slots);
  FTN_CHECK_ARG(ids_kind >= 0 && ids_kind <= 2, "ftn_score_fold: ids_kind=%d", ids_kind);
  FTN_CHECK_ARG(ids_kind != 0 || (N <= n_slots && !ids_dev && !order_dev && !seg_start_dev),
                "ftn_score_fold: without ids the %d series need %d slots or more (and no id operands)", N, N);
  FTN_CHECK_ARG(ids_kind != 1 || (ids_dev && !order_dev && !seg_start_dev),
                "ftn_score_fold: ids_kind 1 takes ids alone");
  FTN_CHECK_ARG(ids_kind != 2 || (order_dev && seg_start_dev), "ftn_score_fold: ids_kind 2 takes order and seg_start");
  FTN_CHECK_ARG((((uintptr_t)part_dev | (uintptr_t)acc_dev | (uintptr_t)ids_dev | (uintptr_t)order_dev |
                  (uintptr_t)seg_start_dev) & 7) == 0 && ((uintptr_t)err_dev & 3) == 0,
                "ftn_score_fold: misaligned operand");
  const int threads = ids_kind == 2 ? n_slots : N;
  hipLaunchKernelGGL(k_score_fold, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, (hipStream_t)stream, part_dev, B,
                     N, ids_kind, ids_dev, order_dev, seg_start_dev, acc_dev, n_slots, err_dev);
  FTN_CHECK_LAUNCH();
  return 0;
}
