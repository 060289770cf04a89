// fp64 arithmetic of the negative-binomial kernels (score.hip, quantile.hip, headfit.hip): reciprocal, log, log1p,
// lgamma's pieces and the digamma difference, with no library call.  Each states its own error.
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

// The NB log-likelihood of one valid element (losses.py:47-53): yc = max(y, 0), r = 1 / alpha, t = alpha mu.  The
// three lgammas share one shift product and cost four logs between them; l1p returns log1p(t).
//   log alpha + log mu - log1p(alpha mu) = -log1p(1 / (alpha mu))
__device__ inline double sc_nb_ll(double yc, double r, double t, double& l1p) {
  double xa = yc + r, xr = r, xc = yc + 1.0, pa = 1.0, pr = 1.0, pc = 1.0;
  sc_shift(xa, pa);
  sc_shift(xr, pr);
  sc_shift(xc, pc);
  double g = sc_stirling(xa) - sc_stirling(xr) - sc_stirling(xc);
  if (pa != 1.0 || pr != 1.0 || pc != 1.0) g += sc_log(pr * pc * sc_rcp(pa));
  l1p = sc_log1p(t);
  return g - r * l1p - yc * sc_log1p(sc_rcp(t));
}

// psi(y + r) - psi(r) for y >= 0, r > 0, never as two digammas subtracted.  Both arguments go up by the same m <= 8
// steps until R = r + m >= 8, X = R + y:
//   psi(y + r) - psi(r) = sum_{j < m} y / ((r + j)(r + y + j)) + D(R, X)
//   D = log1p(y / R) + y / (2 R X) + f(1 / X^2) - f(1 / R^2),   f(z) = -z/12 + z^2/120 - z^3/252 + z^4/240 - z^5/132
// and the difference of the two series is taken term by term, z_X^k - z_R^k = (z_X - z_R) sum_i z_X^i z_R^(k-1-i)
// with z_X - z_R = -y (R + X) z_R z_X.  Every term is >= 0 or dominated by log1p(y / R), so nothing cancels, for r
// large against y as for r small.  Relative error: the first series term left out, 691/32760 z^6, is 3.7e-12 of the
// result at R = 8 (its worst, y -> 0) and sc_log1p gives ~1e-12: 5e-12 in all, the class of sc_stirling.
__device__ inline double sc_dpsi(double y, double r) {
  double R = r, s = 0.0;
  if (R < 8.0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool up = R < 8.0;
      s = up ? fma(y, sc_rcp(R * (R + y)), s) : s;
      R = up ? R + 1.0 : R;
    }
  }
  const double X = R + y, a = sc_rcp(R), b = sc_rcp(X), za = a * a, zb = b * b;
  double pb = zb, h = za + zb, g = -1.0 / 12.0;                  // h_k = sum_i zb^i za^(k-1-i), here k = 2
  g = fma(1.0 / 120.0, h, g);
  pb *= zb; h = fma(za, h, pb);
  g = fma(-1.0 / 252.0, h, g);
  pb *= zb; h = fma(za, h, pb);
  g = fma(1.0 / 240.0, h, g);
  pb *= zb; h = fma(za, h, pb);
  g = fma(-1.0 / 132.0, h, g);
  const double yab = y * a * b;
  return s + (sc_log1p(y * a) + yab * (0.5 - (R + X) * a * b * g));
}
