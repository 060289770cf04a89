// What the negative-binomial CDF, quantile and sampling kernels share (quantile.hip, sample.hip): the fp64 pieces of
// F(k) = I_p(r, k + 1), the distribution's parameters, and the bracketed search for the smallest k with F(k) >= q.
// quantile.hip's head comment states the method and the error of every piece; the caps below bound every loop.
#pragma once
#include "ftn_common.h"
#include "ftn_nbmath.h"
#include <math.h>
#include <initializer_list>

#define NBQ_CF_MAX 4096
#define NBQ_CF_EPS 1e-13     // where a = 1e8 makes aa -> -1 the factor's own rounding noise is a few 1e-15
#define NBQ_EVALS 32
#define NBQ_NEWTON 6
#define NBQ_WALK 64
#define NBQ_KLIM 16777216.0
#define NBQ_THREADS 256

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

// The element loop the three kernels share.  A lane owns CPL consecutive elements of [B][H][N] from nq_first (4 with
// 16-byte loads, where B H N % 4 == 0 and a quad lies in one row; else 1): nq_at splits the first into its batch row
// and the offset within it, nq_load reads the lane's elements of an operand with batch stride bs, NQ_LANE picks one.
struct NbAt { long long b, o; };

template <int CPL>
__device__ inline long long nq_first() { return ((long long)blockIdx.x * NBQ_THREADS + threadIdx.x) * CPL; }

__device__ inline NbAt nq_at(long long e0, long long HN) {
  const long long b = e0 / HN;
  return {b, e0 - b * HN};
}

template <int CPL>
__device__ inline f4 nq_load(const float* p, long long bs, NbAt at) {
  if (CPL == 4) return *(const f4*)(p + at.b * bs + at.o);
  return f4{p[at.b * bs + at.o], 0.f, 0.f, 0.f};
}

// As macros: either one as a function changes the kernels' register allocation (tools/kres.sh, the disassembly).
#define NQ_LANE(v, j) ((j) == 0 ? (v).x : (j) == 1 ? (v).y : (j) == 2 ? (v).z : (v).w)

// FTN_NBQ_RANGE into *flag when any lane of the workgroup saw a bad element: every lane of the workgroup runs it
#define NQ_RAISE(flag, bad) \
  do { if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(flag, FTN_NBQ_RANGE); } while (0)

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

// The standard normal quantile (P. J. Acklam's rational approximation, ~1e-9 relative): it only seeds a search.  One
// body for the host (the levels of ftn_nb_quantiles) and the device (the uniforms of k_nb_sample).
__host__ __device__ inline double nbq_normal_quantile(double q) {
  if (q < 0.02425 || q > 1.0 - 0.02425) {
    const double u = sqrt(-2.0 * log(q < 0.5 ? q : 1.0 - q));
    const double x = (((((-7.784894002430293e-03 * u + -3.223964580411365e-01) * u + -2.400758277161838e+00) * u +
                        -2.549732539343734e+00) * u + 4.374664141464968e+00) * u + 2.938163982698783e+00) /
                     ((((7.784695709041462e-03 * u + 3.224671290700398e-01) * u + 2.445134137142996e+00) * u +
                       3.754408661907416e+00) * u + 1.0);
    return q < 0.5 ? x : -x;
  }
  const double u = q - 0.5, v = u * u;
  return (((((-3.969683028665376e+01 * v + 2.209460984245205e+02) * v + -2.759285104469687e+02) * v +
            1.383577518672690e+02) * v + -3.066479806614716e+01) * v + 2.506628277459239e+00) * u /
         (((((-5.447609879822406e+01 * v + 1.615858368580409e+02) * v + -1.556989798598866e+02) * v +
            6.680131188771972e+01) * v + -1.328068155288572e+01) * v + 1.0);
}

// The form every entry point takes (include/flowtimes.h): the one place the choice is made.
static inline int nbq_form(int N, long long ybs, long long rbs, long long dbs, unsigned misalign_or) {
  return ftn_vec4_ok(N, ybs, rbs, dbs, misalign_or) ? FTN_SHELL_VEC : 0;
}

// the shape and layout checks the entry points share, for any number of operands' batch strides; 0 or < 0
static inline int nbq_check(const char* who, int B, int H, int N, std::initializer_list<long long> bstrides, float eps) {
  FTN_CHECK_ARG(B >= 1 && H >= 1 && N >= 1, "%s: bad shape B=%d H=%d N=%d", who, B, H, N);
  const long long row = (long long)H * N;
  FTN_CHECK_ARG(row <= 0x7fffffffLL && (long long)B * row / 4 / NBQ_THREADS < 0x7fffffffLL,
                "%s: H N = %lld or the grid beyond int32", who, row);
  for (const long long s : bstrides) {
    FTN_CHECK_ARG(s >= 0, "%s: negative batch stride", who);
    FTN_CHECK_ARG(B == 1 || s >= row, "%s: batch stride %lld is below H N = %lld", who, s, row);
  }
  FTN_CHECK_ARG(eps > 0.f && eps < 1.f, "%s: eps=%g", who, (double)eps);
  return 0;
}

// The launch tail of the three entry points: form -> elements per lane -> grid -> kernel K<4> or K<1>
#define NBQ_LAUNCH(K, form, args, stream)                                                   \
  do {                                                                                      \
    const int cpl_ = (form) & FTN_SHELL_VEC ? 4 : 1;                                        \
    const long long per_ = (long long)NBQ_THREADS * cpl_;                                   \
    const dim3 grid_((unsigned)(((args).total + per_ - 1) / per_)), block_(NBQ_THREADS);    \
    if (cpl_ == 4) hipLaunchKernelGGL(K<4>, grid_, block_, 0, (hipStream_t)(stream), args); \
    else hipLaunchKernelGGL(K<1>, grid_, block_, 0, (hipStream_t)(stream), args);           \
    FTN_CHECK_LAUNCH();                                                                     \
  } while (0)
