// Using the forecast's distribution where it lies: the CDF and the quantiles of the negative binomial that every
// forward returns as (rate, dispersion), in the scorer's parameterisation (sc_element, score.hip):
//   al = disp < eps ? eps : disp,  mu = rate < eps ? eps : rate,  r = 1 / al,  t = al mu,  p = 1 / (1 + t)
//   F(k) = I_p(r, k + 1)  (regularised incomplete beta),  Q(q) = the smallest integer k >= 0 with F(k) >= q
//   k_nb_cdf<CPL>       one pass over y, rate, disp: F(floor(max(y, 0))) as fp32 (and, optionally, the fp64 value)
//   k_nb_quantile<CPL>  up to FTN_QMAX levels per launch, ascending, each element's search continuing from its
//                       answer to the level before
//
// F(k) = front cf(a, b, x) / a with a = r, b = k + 1, x = p, or 1 - front cf(b, a, 1 - x) / b when
// x >= (a + 1) / (a + b + 2); cf is the continued fraction of I_x(a, b) by the modified Lentz method, and
// front = exp(lgamma(a + b) - lgamma(a) - lgamma(b) + a log x + b log(1 - x)) = pmf(k) (k + r) (1 - p), so one
// evaluation yields F(k) and pmf(k).  Everything is fp64 and rounded once.  What keeps the exponent accurate for
// k up to 2^24 and r up to 1e8, where each lgamma is ~1e9:
//   - log x = -log1p(t) and log(1 - x) = -log1p(1 / t): no cancellation in either tail
//   - lgamma(L + S) - lgamma(L), L = max(a, b), as Stirling's difference
//     S log(L + S) + (L - 1/2) log1p(S / L) - S + corr(L + S) - corr(L): the two ~L log L terms never exist
//   - nq_log carries the atanh series to s^21 (~3e-16 relative; sc_log's 1e-12 would be 1e-5 absolute at L = 1e7)
// Error of the pieces: nq_log / nq_log1p ~3e-16 relative; nq_exp 3e-16 relative beyond its argument's error
// (Taylor to x^13 on |x| <= log(2) / 2, remainder 4e-18; results below 2^-1022 flush to 0); Stirling's corr is
// truncated after z^7, 6e-12 absolute at x = 8, the bound of the whole exponent for a, b in the fixtures' ranges.
//
// Every loop has a compile-time trip count; an element that exhausts one is written as NaN and raises bit 1 of the
// flag, as does an answer >= 2^24.  No wave spins on data:
//   NBQ_CF_MAX  4096  continued-fraction iterations, ended when a step's factor is within NBQ_CF_EPS = 1e-13 of 1
//                     (where a = 1e8 drives the odd coefficients to -1 the factor's own rounding noise is a few
//                     1e-15, and 1e-13 in F is far below what the quantile needs).  The count grows like
//                     c sqrt(max(a, b)) at its worst point, x at the mean: 573 is the most seen over alpha in
//                     [1e-8, 1e-5] x mu in [0.5, 1e6] x k within -4 .. +6 sd, fewer than 500 for alpha >= 1e-3 and
//                     mu up to 1.2e7 (and 1471 at a = 1e8, b = 1.2e7 with a 2e-15 test): 4096 leaves a factor of 2.8.
//   NBQ_EVALS   32    CDF evaluations of one level: NBQ_NEWTON = 6 safeguarded Newton steps k += (q - F) / pmf, then
//                     bisection of a bracket that is at most [0, 2^24]: 24 halvings to width 1, one evaluation each,
//                     and two to spare.
//   NBQ_WALK    64    steps of the pmf recurrence pmf(k + 1) = pmf(k) (k + r) / (k + 1) (1 - p) after an evaluation
// The evaluation is the convergent part (every lane of a wave that still searches runs it together); the walk is
// the divergent part and costs one reciprocal a step.
#include "ftn_nbq.h"

struct NbqArgs {
  const float* y;  const float* rate;  const float* disp;
  float* out;                  // cdf: [B][H][N]; quantile: [nq][B][H][N], contiguous
  double* out64;               // cdf only, or null
  int* flag;                   // or null (cdf)
  long long ybs, rbs, dbs;     // batch strides in elements
  long long HN, total;         // H N, B H N
  float eps;
  int nq;
  double lev[FTN_QMAX];        // ascending
  double z[FTN_QMAX];          // the standard normal quantile of lev[i]
  int row[FTN_QMAX];           // the output row of lev[i]
};

template <int CPL>
__global__ __launch_bounds__(NBQ_THREADS) void k_nb_cdf(NbqArgs a) {
  const long long e0 = nq_first<CPL>();
  int bad = 0;
  if (e0 < a.total) {
    const NbAt at = nq_at(e0, a.HN);
    const f4 yv = nq_load<CPL>(a.y, a.ybs, at), rv = nq_load<CPL>(a.rate, a.rbs, at),
             dv = nq_load<CPL>(a.disp, a.dbs, at);
    f4 fv = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int j = 0; j < CPL; ++j) {
      const float y = NQ_LANE(yv, j);
      const float yc = y < 0.f ? 0.f : y;
      NbDist D;
      const bool valid = nq_dist(NQ_LANE(rv, j), NQ_LANE(dv, j), a.eps, D) && __builtin_isfinite(yc);
      const double k = floor(valid ? (double)yc : 0.0);
      const bool inside = k < NBQ_KLIM;
      double F, pm;
      const bool ok = nq_cdf_pmf(D, inside ? k : 0.0, F, pm) && inside;
      if (valid && !ok) bad = 1;
      if (!(valid && ok)) F = __builtin_nan("");
      const float f = (float)F;
      fv.x = j == 0 ? f : fv.x; fv.y = j == 1 ? f : fv.y; fv.z = j == 2 ? f : fv.z; fv.w = j == 3 ? f : fv.w;
      if (a.out64) a.out64[e0 + j] = F;
    }
    if (CPL == 4) *(f4*)(a.out + e0) = fv;
    else a.out[e0] = fv.x;
  }
  if (a.flag) NQ_RAISE(a.flag, bad);
}

template <int CPL>
__global__ __launch_bounds__(NBQ_THREADS) void k_nb_quantile(NbqArgs a) {
  const long long e0 = nq_first<CPL>();
  int bad = 0;
  if (e0 < a.total) {
    const NbAt at = nq_at(e0, a.HN);
    const f4 rv = nq_load<CPL>(a.rate, a.rbs, at), dv = nq_load<CPL>(a.disp, a.dbs, at);
#pragma unroll 1
    for (int j = 0; j < CPL; ++j) {
      NbDist D;
      const bool valid = nq_dist(NQ_LANE(rv, j), NQ_LANE(dv, j), a.eps, D);
      NbWalk w = {0.0, 0.0, 0.0, 0.0, false};
#pragma unroll 1
      for (int i = 0; i < a.nq; ++i)
        a.out[(long long)a.row[i] * a.total + e0 + j] = nq_level(D, valid, a.lev[i], a.z[i], w, bad);
    }
  }
  NQ_RAISE(a.flag, bad);
}

extern "C" int ftn_nbq_form(int N, long long y_bstride, long long rate_bstride, long long disp_bstride,
                            int misalign_or) {
  FTN_CHECK_ARG(N >= 1, "ftn_nbq_form: N=%d", N);
  FTN_CHECK_ARG(y_bstride >= 0 && rate_bstride >= 0 && disp_bstride >= 0 && misalign_ok(misalign_or),
                "ftn_nbq_form: strides %lld %lld %lld misalign=%d", y_bstride, rate_bstride, disp_bstride, misalign_or);
  return nbq_form(N, y_bstride, rate_bstride, disp_bstride, (unsigned)misalign_or);
}

extern "C" int ftn_nb_cdf(const float* y_dev, long long y_bstride, const float* rate_dev, long long rate_bstride,
                          const float* disp_dev, long long disp_bstride, int B, int H, int N, float eps,
                          float* out_dev, double* out64_dev, int* flag_dev, void* stream) {
  FTN_CHECK_ARG(y_dev && rate_dev && disp_dev && out_dev, "ftn_nb_cdf: null pointer");
  if (nbq_check("ftn_nb_cdf", B, H, N, {y_bstride, rate_bstride, disp_bstride}, eps) < 0) return -1;
  FTN_CHECK_ARG((((uintptr_t)y_dev | (uintptr_t)rate_dev | (uintptr_t)disp_dev | (uintptr_t)out_dev |
                  (uintptr_t)flag_dev) & 3) == 0 && ((uintptr_t)out64_dev & 7) == 0,
                "ftn_nb_cdf: operands must be 4-byte aligned, out64 8-byte aligned");
  const unsigned mis = (unsigned)(((uintptr_t)y_dev | (uintptr_t)rate_dev | (uintptr_t)disp_dev | (uintptr_t)out_dev) & 15);
  NbqArgs a = {};
  a.y = y_dev; a.rate = rate_dev; a.disp = disp_dev; a.out = out_dev; a.out64 = out64_dev; a.flag = flag_dev;
  a.ybs = B > 1 ? y_bstride : 0; a.rbs = B > 1 ? rate_bstride : 0; a.dbs = B > 1 ? disp_bstride : 0;
  a.HN = (long long)H * N; a.total = (long long)B * a.HN; a.eps = eps;
  NBQ_LAUNCH(k_nb_cdf, nbq_form(N, a.ybs, a.rbs, a.dbs, mis), a, stream);
  return 0;
}

extern "C" int ftn_nb_quantiles(const float* rate_dev, long long rate_bstride, const float* disp_dev,
                                long long disp_bstride, int B, int H, int N, const double* levels_host, int Q,
                                float eps, float* out_dev, int* flag_dev, void* stream) {
  FTN_CHECK_ARG(rate_dev && disp_dev && levels_host && out_dev && flag_dev, "ftn_nb_quantiles: null pointer");
  FTN_CHECK_ARG(Q >= 1 && Q <= FTN_QMAX, "ftn_nb_quantiles: Q=%d is outside 1..%d", Q, FTN_QMAX);
  for (int i = 0; i < Q; ++i)
    FTN_CHECK_ARG(levels_host[i] > 0.0 && levels_host[i] < 1.0, "ftn_nb_quantiles: level %d = %g is not inside (0, 1)",
                  i, levels_host[i]);
  if (nbq_check("ftn_nb_quantiles", B, H, N, {rate_bstride, disp_bstride}, eps) < 0) return -1;
  FTN_CHECK_ARG((((uintptr_t)rate_dev | (uintptr_t)disp_dev | (uintptr_t)out_dev | (uintptr_t)flag_dev) & 3) == 0,
                "ftn_nb_quantiles: operands must be 4-byte aligned");
  const unsigned mis = (unsigned)(((uintptr_t)rate_dev | (uintptr_t)disp_dev) & 15);
  NbqArgs a = {};
  a.rate = rate_dev; a.disp = disp_dev; a.out = out_dev; a.flag = flag_dev;
  a.rbs = B > 1 ? rate_bstride : 0; a.dbs = B > 1 ? disp_bstride : 0;
  a.HN = (long long)H * N; a.total = (long long)B * a.HN; a.eps = eps; a.nq = Q;
  for (int i = 0; i < Q; ++i) {                                 // ascending, by insertion; equal levels keep their order
    int j = i;
    for (; j > 0 && a.lev[j - 1] > levels_host[i]; --j) { a.lev[j] = a.lev[j - 1]; a.row[j] = a.row[j - 1]; }
    a.lev[j] = levels_host[i];
    a.row[j] = i;
  }
  for (int i = 0; i < Q; ++i) a.z[i] = nbq_normal_quantile(a.lev[i]);
  NBQ_LAUNCH(k_nb_quantile, nbq_form(N, 0, a.rbs, a.dbs, mis), a, stream);
  return 0;
}
