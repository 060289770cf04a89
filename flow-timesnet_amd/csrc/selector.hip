// Period selector on gfx950, S3 - S5: FFTPeriodSelector.forward from the batch-mean spectrum on + PeriodGrouper.group
// + the softmax/scatter weights of the reference (models/timesnet.py:124-159, 513-557, 992-1009), one launch and no
// host synchronisation, and the host-only descriptor math.  S1 + S2 (med[B][F], psum[F]) come from spectrum.hip.
//
//   k_finalize   S3-S5  mean, DC kill, log penalty, top-k (wave arg-max),
//                       periods, grouping, tiling, softmax weights -> FtnDesc, amps, w   (body: ftn_finalize.h)
#include <math.h>
#include <stdlib.h>
#include "ftn_common.h"
#include "ftn_exchange.h"

// ---------------------------------------------------------------- S3 - S5
__global__ __launch_bounds__(256) void k_finalize(FinalizeArgs fa) { finalize_body(fa); }

// The per-row section of the finalize (amps[B][16], w[B][16]) over a grid, one thread per batch row: the finalize
// workgroup walks the rows 256 at a time, which at B = 65 536 is 256 serial iterations on the critical path of the
// block call.  Launched behind a finalize that ran with FinalizeArgs.rows_outside; reads the finished descriptor from
// device memory and runs finalize_row, the very function the workgroup's loop runs, so the results agree bit for bit.
__global__ __launch_bounds__(256) void k_row_weights(const FtnDesc* __restrict__ desc, const float* __restrict__ med, int B,
                                                     int F, float* __restrict__ amps, float* __restrict__ wts, int act_dtype) {
  __shared__ FtnDesc sd;
  __shared__ float red[256][FTN_KMAX + 1];
  __shared__ float wred[256][FTN_KMAX + 1];
  const int tid = threadIdx.x;
  {
    const int* src = (const int*)desc;
    int* dst = (int*)&sd;
    for (int e = tid; e < (int)(sizeof(FtnDesc) / 4); e += 256) dst[e] = src[e];
  }
  __syncthreads();
  const long long b = (long long)blockIdx.x * 256 + tid;
  if (b >= B) return;
  finalize_row(sd, med + (size_t)b * F, red[tid], wred[tid], amps + (size_t)b * FTN_KMAX, wts + (size_t)b * FTN_KMAX, sd.n_sel,
               sd.n_groups, act_dtype);
}

// Rows from which the grid form takes the per-row section.  Measured (profiles/finalize_rows_time.json, DESIGN §4
// "Row passes"); never below 1024, so every benchmarked configuration keeps the single launch.  FTN_FIN_ROWS=<n>
// forces it for tests and A/B runs (read once per process): n >= 1 = rows from which the grid form runs, 0 = never.
#define FTN_FIN_ROWS_DEFAULT 1024
bool ftn_fin_rows_outside(int B) {
  static const long long thr = [] {
    const char* e = getenv("FTN_FIN_ROWS");
    return e == nullptr || e[0] == '\0' ? (long long)FTN_FIN_ROWS_DEFAULT : atoll(e);
  }();
  return thr > 0 && B >= thr;
}

int ftn_launch_row_weights(const FinalizeArgs& fa, hipStream_t st) {
  hipLaunchKernelGGL(k_row_weights, dim3((unsigned)((fa.B + 255) / 256)), dim3(256), 0, st, (const FtnDesc*)fa.desc, fa.med, fa.B,
                     fa.F, fa.amps, fa.wts, fa.act_dtype);
  FTN_CHECK_LAUNCH();
  return 0;
}

int ftn_finalize_check(const char* who, const double* psum, int nparts, int Btotal, const float* med, int B, int L,
                       const FtnDesc* desc, const float* amps, const float* wts, const FtnExchange* xch) {
  FTN_CHECK_ARG((psum || xch) && med && desc && amps && wts, "%s: null pointer", who);
  FTN_CHECK_ARG(xch == nullptr || ftn_xch_ok(xch, L / 2 + 1), "%s: bad exchange (world / rank / seq / mode / F_cap)", who);
  if (xch != nullptr) nparts = xch->world;
  FTN_CHECK_ARG((((uintptr_t)amps | (uintptr_t)wts) & 15) == 0, "%s: amps / weights must be 16-byte aligned", who);
  FTN_CHECK_ARG(B >= 1 && L >= 2 && nparts >= 1 && Btotal >= B, "%s: bad shape", who);
  return 0;
}

int ftn_finalize_args(const char* who, const double* psum, int nparts, int Btotal, const float* med, int B, int L, int k, int pmax,
                      int min_thr, int act_dtype, int max_unique, double log_base, FtnDesc* desc, float* amps, float* wts,
                      const FtnExchange* xch, FinalizeArgs* fa) {
  ftn_selector_clamp(&k, &pmax, &min_thr);
  const int F = L / 2 + 1;
  FTN_CHECK_ARG(ftn_finalize_lds_bytes(F) <= 48 * 1024, "%s: L=%d too long", who, L);
  *fa = FinalizeArgs{psum, xch != nullptr ? xch->world : nparts, Btotal, med, B, L, F, k, pmax, min_thr, desc, amps, wts, act_dtype,
                     max_unique > 0 ? max_unique : 0, log_base > 1.0 ? (float)log(log_base) : 0.f};
  if (xch != nullptr) ftn_xch_fill(xch, F, fa);
  return 0;
}

extern "C" int ftn_period_finalize(const double* psum_dev, int nparts, int Btotal, const float* med_dev, int B,
                                   int L, int k_periods, int pmax, int min_period_threshold, int act_dtype,
                                   int max_unique, double log_base, FtnDesc* desc_dev, float* amps_dev,
                                   float* weights_dev, void* stream, const FtnExchange* xch) {
  const char* who = "ftn_period_finalize";
  int rc = ftn_finalize_check(who, psum_dev, nparts, Btotal, med_dev, B, L, desc_dev, amps_dev, weights_dev, xch);
  if (rc) return rc;
  FTN_CHECK_ARG(k_periods <= FTN_KMAX, "ftn_period_finalize: k_periods=%d > FTN_KMAX=%d", k_periods, FTN_KMAX);
  FTN_CHECK_ARG(act_dtype >= 0 && act_dtype <= 2, "ftn_period_finalize: act_dtype=%d", act_dtype);
  FinalizeArgs fa;
  if ((rc = ftn_finalize_args(who, psum_dev, nparts, Btotal, med_dev, B, L, k_periods, pmax, min_period_threshold, act_dtype,
                              max_unique, log_base, desc_dev, amps_dev, weights_dev, xch, &fa)))
    return rc;
  fa.rows_outside = ftn_fin_rows_outside(B) ? 1 : 0;
  hipLaunchKernelGGL(k_finalize, dim3(1), dim3(256), ftn_finalize_lds_bytes(fa.F), (hipStream_t)stream, fa);
  FTN_CHECK_LAUNCH();
  return fa.rows_outside ? ftn_launch_row_weights(fa, (hipStream_t)stream) : 0;
}

// Bound on FtnDesc.total_px / n_groups for descriptors written by ftn_period_finalize: the selector can only
// produce periods clamp(ceil(L/i), lo, hi) for rFFT bins i = 1..F-1 (:144-145), at most k of them, so the
// sum of the k largest L + pad over those distinct periods bounds the grid pixels per batch row.  For
// i >= 2 the pad is < i, i.e. (almost) every group is L pixels plus a few; only bin 1 (period L-1) doubles.
extern "C" int ftn_selector_px_bound(int L, int k_periods, int pmax, int min_period_threshold, int* max_groups_out) {
  FTN_CHECK_ARG(L >= 2 && k_periods <= FTN_KMAX, "ftn_selector_px_bound: L=%d k=%d", L, k_periods);
  ftn_selector_clamp(&k_periods, &pmax, &min_period_threshold);
  const int F = L / 2 + 1;
  const int k = k_periods < F - 1 ? k_periods : F - 1;
  const int hi = pmax < (L - 1 > 1 ? L - 1 : 1) ? pmax : (L - 1 > 1 ? L - 1 : 1), lo = min_period_threshold;
  int best[FTN_KMAX] = {0};
  int ndist = 0, last = -1;
  if (hi >= lo) {
    for (int i = 1; i < F; ++i) {                 // periods are non-increasing in i: distinct values are runs
      int p = (L + i - 1) / i;
      p = p < lo ? lo : (p > hi ? hi : p);
      if ((L + p - 1) / p < 2 || p == last) continue;
      last = p;
      ++ndist;
      int v = L + (p - (L % p)) % p;
      for (int s = 0; s < k; ++s)
        if (v > best[s]) { int tmp = best[s]; best[s] = v; v = tmp; }
    }
  }
  long long sum = 0;
  for (int s = 0; s < k; ++s) sum += best[s];
  if (max_groups_out) *max_groups_out = ndist < k ? (ndist > 0 ? ndist : 1) : (k > 0 ? k : 1);
  return sum > 0 ? (int)sum : L;
}

extern "C" int ftn_desc_from_periods(const int64_t* periods, int K, int L, int min_period, int max_period,
                                     FtnDesc* d) {
  FTN_CHECK_ARG(periods && d && K >= 0 && K <= FTN_KMAX && L >= 1, "ftn_desc_from_periods: bad argument (K=%d)", K);
  int p32[FTN_KMAX];
  for (int j = 0; j < FTN_KMAX; ++j) { d->sel_freq[j] = 0; d->sel_period[j] = 0; p32[j] = 0; }
  for (int j = 0; j < K; ++j) {
    long long p = periods[j];
    if (p > 0x3fffffff) p = 0x3fffffff;
    if (p < -1) p = -1;
    p32[j] = (int)p;
    d->sel_period[j] = (int)p;
  }
  d->n_sel = K;
  ftn_build_groups(p32, K, L, min_period, max_period, d);
  return 0;
}
