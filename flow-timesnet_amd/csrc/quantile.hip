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
#include "ftn_common.h"
#include "ftn_nbmath.h"
#include <math.h>

#define NBQ_CF_MAX 4096
#define NBQ_CF_EPS 1e-13     // where a = 1e8 makes aa -> -1 the factor's own rounding noise is a few 1e-15
#define NBQ_EVALS 32
#define NBQ_NEWTON 6
#define NBQ_WALK 64
#define NBQ_KLIM 16777216.0
#define NBQ_THREADS 256

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

// log x for a normal positive x to ~3e-16 relative: sc_log's reduction, the series through s^21
__device__ inline double nq_log(double x) {
  int e = __builtin_amdgcn_frexp_exp(x);
  double m = __builtin_amdgcn_frexp_mant(x);                    // [0.5, 1)
  const bool lo = m < 0.70710678118654752;
  m = lo ? m + m : m;
  e = lo ? e - 1 : e;
  const double s = (m - 1.0) * sc_rcp(m + 1.0), z = s * s;
  double p = 1.0 / 21.0;
  p = fma(p, z, 1.0 / 19.0);
  p = fma(p, z, 1.0 / 17.0);
  p = fma(p, z, 1.0 / 15.0);
  p = fma(p, z, 1.0 / 13.0);
  p = fma(p, z, 1.0 / 11.0);
  p = fma(p, z, 1.0 / 9.0);
  p = fma(p, z, 1.0 / 7.0);
  p = fma(p, z, 1.0 / 5.0);
  p = fma(p, z, 1.0 / 3.0);
  p = fma(p, z * s, s);
  return fma((double)e, 0.69314718055994531, p + p);
}

// log(1 + x), x >= 0, relative: log(u) with the rounding of u = 1 + x given back
__device__ inline double nq_log1p(double x) {
  const double u = 1.0 + x;
  return nq_log(u) - ((u - 1.0) - x) * sc_rcp(u);
}

// exp x, x <= 700: x = n log 2 + f, |f| <= log(2) / 2, Taylor through f^13 (remainder 4e-18), scaled by 2^n.
// 0 below -708 (no subnormal results).
__device__ inline double nq_exp(double x) {
  if (!(x > -708.0)) return x != x ? x : 0.0;
  const double n = __builtin_rint(x * 1.44269504088896341);
  double f = fma(-n, 6.93147180369123816490e-01, x);            // n log2_hi is exact: 21 trailing zero bits
  f = fma(-n, 1.90821492927058770002e-10, f);
  double p = 1.0 / 6227020800.0;
  p = fma(p, f, 1.0 / 479001600.0);
  p = fma(p, f, 1.0 / 39916800.0);
  p = fma(p, f, 1.0 / 3628800.0);
  p = fma(p, f, 1.0 / 362880.0);
  p = fma(p, f, 1.0 / 40320.0);
  p = fma(p, f, 1.0 / 5040.0);
  p = fma(p, f, 1.0 / 720.0);
  p = fma(p, f, 1.0 / 120.0);
  p = fma(p, f, 1.0 / 24.0);
  p = fma(p, f, 1.0 / 6.0);
  p = fma(p, f, 0.5);
  p = fma(p, f, 1.0);
  p = fma(p, f, 1.0);
  return __builtin_ldexp(p, (int)n);
}

// lgamma(x) - ((x - 1/2) log x - x + log sqrt(2 pi)) for x >= 8: sc_stirling's series
__device__ inline double nq_corr(double x) {
  const double z = sc_rcp(x), z2 = z * z;
  double w = -1.0 / 1680.0;
  w = fma(w, z2, 1.0 / 1260.0);
  w = fma(w, z2, -1.0 / 360.0);
  w = fma(w, z2, 1.0 / 12.0);
  return w * z;
}

// lgamma(x), x > 0
__device__ inline double nq_lgamma(double x) {
  double pr = 1.0;
  sc_shift(x, pr);
  return fma(x - 0.5, nq_log(x), 0.91893853320467274 - x) + nq_corr(x) - nq_log(pr);
}

// lgamma(a + b) - lgamma(a) - lgamma(b), a, b > 0.  L = max(a, b) is shifted up to >= 8 with the factors of both
// lgamma(L + S) and lgamma(L) gathered (pn / pd), then the difference of the two is taken in Stirling's form.
__device__ inline double nq_log_inv_beta(double a, double b) {
  double L = a > b ? a : b;
  const double S = a > b ? b : a;
  double pn = 1.0, pd = 1.0;
  if (L < 8.0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool s = L < 8.0;
      pn = s ? pn * (L + S) : pn;
      pd = s ? pd * L : pd;
      L = s ? L + 1.0 : L;
    }
  }
  const double g = fma(S, nq_log(L + S), fma(L - 0.5, nq_log1p(S * sc_rcp(L)), -S)) + (nq_corr(L + S) - nq_corr(L));
  return g - nq_log(pn * sc_rcp(pd)) - nq_lgamma(S);
}

// The continued fraction of I_x(a, b), modified Lentz.  With aa = num / den the two updates are
// d <- den / (den + num d) and c <- 1 + num / (den c): two reciprocals a half step.  false: NBQ_CF_MAX reached.
#define NQ_GUARD(v) ((v) < 1e-300 && (v) > -1e-300 ? 1e-300 : (v))
__device__ inline bool nq_betacf(double a, double b, double x, double& h) {
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x * sc_rcp(qap);
  d = sc_rcp(NQ_GUARD(d));
  h = d;
  for (int m = 1; m <= NBQ_CF_MAX; ++m) {
    const double fm = (double)m, m2 = fm + fm, am2 = a + m2;
    double num = fm * (b - fm) * x, den = (qam + m2) * am2;
    double v = fma(num, d, den), u = den * c;
    d = den * sc_rcp(NQ_GUARD(v));
    c = fma(num, sc_rcp(NQ_GUARD(u)), 1.0);
    c = NQ_GUARD(c);
    h *= d * c;
    num = -(a + fm) * (qab + fm) * x;
    den = am2 * (qap + m2);
    v = fma(num, d, den);
    u = den * c;
    d = den * sc_rcp(NQ_GUARD(v));
    c = fma(num, sc_rcp(NQ_GUARD(u)), 1.0);
    c = NQ_GUARD(c);
    const double de = d * c;
    h *= de;
    if (fabs(de - 1.0) < NBQ_CF_EPS) return true;
  }
  return false;
}

struct NbDist { double r, al, t, p, omp, lp, lomp; };

// false where al or mu is not finite
__device__ inline bool nq_dist(float rate, float disp, float eps, NbDist& D) {
  const float al = disp < eps ? eps : disp;                     // comparisons, not fmaxf: a NaN stays a NaN
  const float mu = rate < eps ? eps : rate;
  const bool valid = __builtin_isfinite(al) && __builtin_isfinite(mu);
  D.al = valid ? (double)al : 1.0;
  D.r = sc_rcp(D.al);
  D.t = D.al * (valid ? (double)mu : 1.0);                      // the product of two floats is exact
  D.p = sc_rcp(1.0 + D.t);
  D.omp = D.t * D.p;
  D.lp = -nq_log1p(D.t);
  D.lomp = -nq_log1p(sc_rcp(D.t));
  return valid;
}

// F(k) and pmf(k) for an integer-valued 0 <= k < 2^24.  false: the fraction did not converge.
__device__ inline bool nq_cdf_pmf(const NbDist& D, double k, double& F, double& pm) {
  const double a = D.r, b = k + 1.0;
  const double front = nq_exp(nq_log_inv_beta(a, b) + a * D.lp + b * D.lomp);
  const bool swap = D.p * (a + b + 2.0) >= a + 1.0;
  double h;
  const bool ok = nq_betacf(swap ? b : a, swap ? a : b, swap ? D.omp : D.p, h);
  double f = swap ? 1.0 - front * h * sc_rcp(b) : front * h * D.al;
  f = f < 0.0 ? 0.0 : f;
  F = f > 1.0 ? 1.0 : f;
  pm = front * sc_rcp((k + D.r) * D.omp);
  return ok;
}

// element e of [B][H][N] in an operand with batch stride bs
__device__ inline long long nq_off(long long e, long long HN, long long bs) {
  const long long b = e / HN;
  return b * bs + (e - b * HN);
}

template <int CPL>
__global__ __launch_bounds__(NBQ_THREADS) void k_nb_cdf(NbqArgs a) {
  const long long e0 = ((long long)blockIdx.x * NBQ_THREADS + threadIdx.x) * CPL;
  int bad = 0;
  if (e0 < a.total) {                                           // CPL == 4: total % 4 == 0, a quad has one row
    const long long b = e0 / a.HN, o = e0 - b * a.HN;
    f4 yv = {0.f, 0.f, 0.f, 0.f}, rv = yv, dv = yv, fv = yv;
    if (CPL == 4) {
      yv = *(const f4*)(a.y + b * a.ybs + o);
      rv = *(const f4*)(a.rate + b * a.rbs + o);
      dv = *(const f4*)(a.disp + b * a.dbs + o);
    } else {
      yv.x = a.y[b * a.ybs + o]; rv.x = a.rate[b * a.rbs + o]; dv.x = a.disp[b * a.dbs + o];
    }
#pragma unroll 1
    for (int j = 0; j < CPL; ++j) {
      const float y = j == 0 ? yv.x : j == 1 ? yv.y : j == 2 ? yv.z : yv.w;
      const float rt = j == 0 ? rv.x : j == 1 ? rv.y : j == 2 ? rv.z : rv.w;
      const float ds = j == 0 ? dv.x : j == 1 ? dv.y : j == 2 ? dv.z : dv.w;
      const float yc = y < 0.f ? 0.f : y;
      NbDist D;
      const bool valid = nq_dist(rt, ds, a.eps, D) && __builtin_isfinite(yc);
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
  if (a.flag && __syncthreads_or(bad) && threadIdx.x == 0) atomicOr(a.flag, FTN_NBQ_RANGE);
}

// Cornish-Fisher start: mean + sd (z + skew (z^2 - 1) / 6), floored into [0, 2^24); hardware sqrt / rsq estimates
__device__ inline double nq_guess(const NbDist& D, double z) {
  const double mean = D.r * D.t, sd = __builtin_amdgcn_sqrt(mean * (1.0 + D.t));
  const double skew = (2.0 - D.p) * __builtin_amdgcn_rsq(D.r * D.omp);
  const double g = floor(fma(sd, fma(skew * (1.0 / 6.0), fma(z, z, -1.0), z), mean));
  return !(g >= 0.0) ? 0.0 : g > NBQ_KLIM - 1.0 ? NBQ_KLIM - 1.0 : g;
}

// (k, F, pm): the last point whose F(k) and pmf(k) are known; prev: the answer to the level before
struct NbWalk { double k, F, pm, prev; bool have; };

// One level of one element, continuing from w.  NaN (and bad = 1 where the element is valid) when the answer is
// >= 2^24 or a cap was reached.
__device__ inline float nq_level(const NbDist& D, bool valid, double q, double z, NbWalk& w, int& bad) {
  double k = w.k, F = w.F, pm = w.pm;
  double g = nq_guess(D, z);
  g = g < w.prev ? w.prev : g;
  // the answer lies in [lo, hi]: F(lo - 1) < q, and F(hi) >= q unless hi is still 2^24
  double lo = w.prev, hi = NBQ_KLIM;
  bool need = !(w.have && g <= k + (double)NBQ_WALK);           // near the last answer: walk on from it
  k = need ? g : k;
  bool done = !valid;
#pragma unroll 1
  for (int it = 0; it < NBQ_EVALS; ++it) {
    if (done) break;
    if (need && !nq_cdf_pmf(D, k, F, pm)) break;                // the fraction's cap: lo < hi, so NaN below
    if (F >= q) {
#pragma unroll 1
      for (int s = 0; s < NBQ_WALK; ++s) {
        if (!(k > lo && F - pm >= q)) break;
        F -= pm;
        pm *= k * sc_rcp((k - 1.0 + D.r) * D.omp);
        k -= 1.0;
      }
    } else {
#pragma unroll 1
      for (int s = 0; s < NBQ_WALK; ++s) {
        if (!(F < q && k + 1.0 < NBQ_KLIM)) break;
        lo = k + 1.0;
        pm *= (k + D.r) * D.omp * sc_rcp(k + 1.0);
        k += 1.0;
        F += pm;
      }
    }
    if (F >= q) {
      hi = k < hi ? k : hi;
      if (k <= lo || F - pm < q) lo = hi = k;
    } else {
      lo = k + 1.0;
    }
    if (lo >= hi) { done = true; break; }
    const double kn = floor(k + (q - F) * sc_rcp(pm) + 0.5);
    k = (it < NBQ_NEWTON && kn >= lo && kn < hi) ? kn : floor(0.5 * (lo + hi));
    need = true;
  }
  const bool ans = valid && done && hi < NBQ_KLIM;
  if (valid && !ans) bad = 1;
  w.k = k; w.F = F; w.pm = pm;
  w.have = ans && k == hi;
  w.prev = ans ? hi : w.prev;
  return ans ? (float)hi : __builtin_nanf("");
}

template <int CPL>
__global__ __launch_bounds__(NBQ_THREADS) void k_nb_quantile(NbqArgs a) {
  const long long e0 = ((long long)blockIdx.x * NBQ_THREADS + threadIdx.x) * CPL;
  int bad = 0;
  if (e0 < a.total) {                                           // CPL == 4: total % 4 == 0, a quad has one row
    const long long b = e0 / a.HN, o = e0 - b * a.HN;
    f4 rv = {0.f, 0.f, 0.f, 0.f}, dv = rv;
    if (CPL == 4) {
      rv = *(const f4*)(a.rate + b * a.rbs + o);
      dv = *(const f4*)(a.disp + b * a.dbs + o);
    } else {
      rv.x = a.rate[b * a.rbs + o]; dv.x = a.disp[b * a.dbs + o];
    }
#pragma unroll 1
    for (int j = 0; j < CPL; ++j) {
      const float rt = j == 0 ? rv.x : j == 1 ? rv.y : j == 2 ? rv.z : rv.w;
      const float ds = j == 0 ? dv.x : j == 1 ? dv.y : j == 2 ? dv.z : dv.w;
      NbDist D;
      const bool valid = nq_dist(rt, ds, a.eps, D);
      NbWalk w = {0.0, 0.0, 0.0, 0.0, false};
#pragma unroll 1
      for (int i = 0; i < a.nq; ++i)
        a.out[(long long)a.row[i] * a.total + e0 + j] = nq_level(D, valid, a.lev[i], a.z[i], w, bad);
    }
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(a.flag, FTN_NBQ_RANGE);
}

// The form both entry points take (include/flowtimes.h): the one place the choice is made.
static int nbq_form(int N, long long ybs, long long rbs, long long dbs, unsigned misalign_or) {
  const bool vec = N % 4 == 0 && ybs % 4 == 0 && rbs % 4 == 0 && dbs % 4 == 0 && (misalign_or & 15) == 0;
  return vec ? FTN_SHELL_VEC : 0;
}

extern "C" int ftn_nbq_form(int N, long long y_bstride, long long rate_bstride, long long disp_bstride,
                            int misalign_or) {
  FTN_CHECK_ARG(N >= 1, "ftn_nbq_form: N=%d", N);
  FTN_CHECK_ARG(y_bstride >= 0 && rate_bstride >= 0 && disp_bstride >= 0 && misalign_or >= 0 && misalign_or < 16 &&
                    misalign_or % 4 == 0,
                "ftn_nbq_form: strides %lld %lld %lld misalign=%d", y_bstride, rate_bstride, disp_bstride, misalign_or);
  return nbq_form(N, y_bstride, rate_bstride, disp_bstride, (unsigned)misalign_or);
}

// the shape and layout checks both entry points share; 0 or < 0
static int nbq_check(const char* who, int B, int H, int N, long long s0, long long s1, long long s2, float eps) {
  FTN_CHECK_ARG(B >= 1 && H >= 1 && N >= 1, "%s: bad shape B=%d H=%d N=%d", who, B, H, N);
  const long long row = (long long)H * N;
  FTN_CHECK_ARG(row <= 0x7fffffffLL && (long long)B * row / 4 / NBQ_THREADS < 0x7fffffffLL,
                "%s: H N = %lld or the grid beyond int32", who, row);
  FTN_CHECK_ARG(s0 >= 0 && s1 >= 0 && s2 >= 0, "%s: negative batch stride", who);
  FTN_CHECK_ARG(B == 1 || (s0 >= row && s1 >= row && s2 >= row), "%s: batch strides %lld %lld %lld are below H N = %lld",
                who, s0, s1, s2, row);
  FTN_CHECK_ARG(eps > 0.f && eps < 1.f, "%s: eps=%g", who, (double)eps);
  return 0;
}

extern "C" int ftn_nb_cdf(const float* y_dev, long long y_bstride, const float* rate_dev, long long rate_bstride,
                          const float* disp_dev, long long disp_bstride, int B, int H, int N, float eps,
                          float* out_dev, double* out64_dev, int* flag_dev, void* stream) {
  FTN_CHECK_ARG(y_dev && rate_dev && disp_dev && out_dev, "ftn_nb_cdf: null pointer");
  const long long row = (long long)H * N;
  if (nbq_check("ftn_nb_cdf", B, H, N, y_bstride, rate_bstride, disp_bstride, eps) < 0) return -1;
  FTN_CHECK_ARG((((uintptr_t)y_dev | (uintptr_t)rate_dev | (uintptr_t)disp_dev | (uintptr_t)out_dev |
                  (uintptr_t)flag_dev) & 3) == 0 && ((uintptr_t)out64_dev & 7) == 0,
                "ftn_nb_cdf: operands must be 4-byte aligned, out64 8-byte aligned");
  const unsigned mis = (unsigned)(((uintptr_t)y_dev | (uintptr_t)rate_dev | (uintptr_t)disp_dev | (uintptr_t)out_dev) & 15);
  NbqArgs a = {};
  a.y = y_dev; a.rate = rate_dev; a.disp = disp_dev; a.out = out_dev; a.out64 = out64_dev; a.flag = flag_dev;
  a.ybs = B > 1 ? y_bstride : 0; a.rbs = B > 1 ? rate_bstride : 0; a.dbs = B > 1 ? disp_bstride : 0;
  a.HN = row; a.total = (long long)B * row; a.eps = eps;
  const int cpl = nbq_form(N, a.ybs, a.rbs, a.dbs, mis) & FTN_SHELL_VEC ? 4 : 1;
  const long long per = (long long)NBQ_THREADS * cpl;
  const dim3 grid((unsigned)((a.total + per - 1) / per)), block(NBQ_THREADS);
  if (cpl == 4) hipLaunchKernelGGL(k_nb_cdf<4>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_nb_cdf<1>, grid, block, 0, (hipStream_t)stream, a);
  FTN_CHECK_LAUNCH();
  return 0;
}

// The standard normal quantile (P. J. Acklam's rational approximation, ~1e-9 relative): it only seeds a search.
static double nbq_normal_quantile(double q) {
  static const double A[6] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
                              1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00};
  static const double Bc[5] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02,
                               6.680131188771972e+01, -1.328068155288572e+01};
  static const double Cc[6] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
                               -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00};
  static const double Dc[4] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00,
                               3.754408661907416e+00};
  if (q < 0.02425 || q > 1.0 - 0.02425) {
    const double u = sqrt(-2.0 * log(q < 0.5 ? q : 1.0 - q));
    const double x = (((((Cc[0] * u + Cc[1]) * u + Cc[2]) * u + Cc[3]) * u + Cc[4]) * u + Cc[5]) /
                     ((((Dc[0] * u + Dc[1]) * u + Dc[2]) * u + Dc[3]) * u + 1.0);
    return q < 0.5 ? x : -x;
  }
  const double u = q - 0.5, v = u * u;
  return (((((A[0] * v + A[1]) * v + A[2]) * v + A[3]) * v + A[4]) * v + A[5]) * u /
         (((((Bc[0] * v + Bc[1]) * v + Bc[2]) * v + Bc[3]) * v + Bc[4]) * v + 1.0);
}

extern "C" int ftn_nb_quantiles(const float* rate_dev, long long rate_bstride, const float* disp_dev,
                                long long disp_bstride, int B, int H, int N, const double* levels_host, int Q,
                                float eps, float* out_dev, int* flag_dev, void* stream) {
  FTN_CHECK_ARG(rate_dev && disp_dev && levels_host && out_dev && flag_dev, "ftn_nb_quantiles: null pointer");
  FTN_CHECK_ARG(Q >= 1 && Q <= FTN_QMAX, "ftn_nb_quantiles: Q=%d is outside 1..%d", Q, FTN_QMAX);
  for (int i = 0; i < Q; ++i)
    FTN_CHECK_ARG(levels_host[i] > 0.0 && levels_host[i] < 1.0, "ftn_nb_quantiles: level %d = %g is not inside (0, 1)",
                  i, levels_host[i]);
  if (nbq_check("ftn_nb_quantiles", B, H, N, rate_bstride, rate_bstride, disp_bstride, eps) < 0) return -1;
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
  const int cpl = nbq_form(N, 0, a.rbs, a.dbs, mis) & FTN_SHELL_VEC ? 4 : 1;
  const long long per = (long long)NBQ_THREADS * cpl;
  const dim3 grid((unsigned)((a.total + per - 1) / per)), block(NBQ_THREADS);
  if (cpl == 4) hipLaunchKernelGGL(k_nb_quantile<4>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_nb_quantile<1>, grid, block, 0, (hipStream_t)stream, a);
  FTN_CHECK_LAUNCH();
  return 0;
}
