// fp64 arithmetic of the negative-binomial kernels (score.hip, quantile.hip): reciprocal, log, log1p and lgamma's
// pieces, with no library call.  Each states its own error.
#pragma once
#include <hip/hip_runtime.h>

// 1 / x for a normal positive x: the hardware estimate and two Newton steps
__device__ inline double sc_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(r, fma(-x, r, 1.0), r);
  r = fma(r, fma(-x, r, 1.0), r);
  return r;
}

// log x for a normal positive x, to ~1e-12 relative: x = 2^e m with m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s),
// s = (m - 1) / (m + 1), |s| <= 0.1716, the series through s^13
__device__ inline double sc_log(double x) {
  int e = __builtin_amdgcn_frexp_exp(x);
  double m = __builtin_amdgcn_frexp_mant(x);                    // [0.5, 1)
  const bool lo = m < 0.70710678118654752;
  m = lo ? m + m : m;
  e = lo ? e - 1 : e;
  const double s = (m - 1.0) * sc_rcp(m + 1.0), z = s * s;
  double p = 1.0 / 13.0;
  p = fma(p, z, 1.0 / 11.0);
  p = fma(p, z, 1.0 / 9.0);
  p = fma(p, z, 1.0 / 7.0);
  p = fma(p, z, 1.0 / 5.0);
  p = fma(p, z, 1.0 / 3.0);
  p = fma(p, z * s, s);
  return fma((double)e, 0.69314718055994531, p + p);
}

// log(1 + x), x >= 0: log(u) with the rounding of u = 1 + x given back
__device__ inline double sc_log1p(double x) {
  const double u = 1.0 + x;
  return sc_log(u) - ((u - 1.0) - x) * sc_rcp(u);
}

// x > 0 up to >= 8 by x -> x + 1, the factors gathered in p:  lgamma(x_in) = lgamma(x_out) - log p
__device__ inline void sc_shift(double& x, double& p) {
  if (x < 8.0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool s = x < 8.0;
      p = s ? p * x : p;
      x = s ? x + 1.0 : x;
    }
  }
}

// lgamma(x) for x >= 8: Stirling's series through z^7 (the next term is 6e-12 at x = 8)
__device__ inline double sc_stirling(double x) {
  const double z = sc_rcp(x), z2 = z * z;
  double w = -1.0 / 1680.0;
  w = fma(w, z2, 1.0 / 1260.0);
  w = fma(w, z2, -1.0 / 360.0);
  w = fma(w, z2, 1.0 / 12.0);
  return fma(x - 0.5, sc_log(x), fma(w, z, 0.91893853320467274 - x));
}
