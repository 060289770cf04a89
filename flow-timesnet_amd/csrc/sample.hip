// Sample paths of the forecast's distribution: S draws of the negative binomial (rate, dispersion) per element, by
// inversion of the CDF that quantile.hip defines (ftn_nbq.h): draw s of element e is the smallest integer k >= 0 with
// F(k) >= u(e, s).  One uniform per draw makes a draw a pure function of (seed, offset, e, s):
//   Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (e & 0xffffffff, e >> 32, s >> 2, offset),
//   e = (b H + h) N + n the logical element index (no stride, no kernel form in it); draw s takes output word s & 3;
//   u = (word + 0.5) 2^-32 in fp64: exact, strictly inside (0, 1), tails down to 1.2e-10.
//   k_nb_sample<CPL>  a lane owns CPL elements (4 with 16-byte loads, else 1) and all S draws of each
//
// What a lane computes once per element and reuses for every draw: the distribution (nq_dist: three reciprocals and
// two log1p) and pmf(0) = p^r = exp(r log p).  A draw is then one nq_level call that starts from the known point
// (k, F, pmf) = (0, p^r, p^r): where the Cornish-Fisher start of the draw's level is within NBQ_WALK of 0 the search
// walks the pmf recurrence up from 0 and never touches the continued fraction (the whole of a low-count forecast);
// elsewhere, and where p^r underflows, it evaluates F at the start and goes on exactly as a quantile does.  The start
// needs the normal quantile of u on the device: nbq_normal_quantile, the body the host uses for ftn_nb_quantiles.
//
// Loops: the draws (S, a launch argument) and nq_level's capped loops; no wave spins on data.  An answer >= 2^24 or
// a cap reached gives NaN and raises FTN_NBQ_RANGE; alpha or mu not finite gives NaN and leaves the flag alone.
#include "ftn_nbq.h"
#include "ftn_philox.h"

struct NbsArgs {
  const float* rate;  const float* disp;
  float* out;                          // [S][B][H][N], contiguous
  double* uout;                        // the uniforms, same shape, or null
  int* flag;
  const unsigned long long* seed_dev;  // read instead of seed where not null
  unsigned long long seed;
  long long rbs, dbs;                  // batch strides in elements
  long long HN, total;                 // H N, B H N
  float eps;
  int S;
  unsigned offset;
};

template <int CPL>
__global__ __launch_bounds__(NBQ_THREADS) void k_nb_sample(NbsArgs a) {
  const long long e0 = nq_first<CPL>();
  int bad = 0;
  if (e0 < a.total) {
    const unsigned long long seed = a.seed_dev ? *a.seed_dev : a.seed;
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    const NbAt at = nq_at(e0, a.HN);
    const f4 rv = nq_load<CPL>(a.rate, a.rbs, at), dv = nq_load<CPL>(a.disp, a.dbs, at);
#pragma unroll 1
    for (int j = 0; j < CPL; ++j) {
      NbDist D;
      const bool valid = nq_dist(NQ_LANE(rv, j), NQ_LANE(dv, j), a.eps, D);
      const double pm0 = nq_exp(D.r * D.lp);                    // pmf(0) = F(0) = p^r; 0 where it underflows
      const unsigned long long e = (unsigned long long)(e0 + j);
      PhiloxWords wd = {0u, 0u, 0u, 0u};
#pragma unroll 1
      for (int s = 0; s < a.S; ++s) {
        if ((s & 3) == 0) wd = ftn_philox((unsigned)e, (unsigned)(e >> 32), (unsigned)s >> 2, a.offset, k0, k1);
        const unsigned word = (s & 3) == 0 ? wd.x : (s & 3) == 1 ? wd.y : (s & 3) == 2 ? wd.z : wd.w;
        const double u = ((double)word + 0.5) * 2.3283064365386963e-10;   // 2^-32
        NbWalk w = {0.0, pm0, pm0, 0.0, pm0 > 0.0};
        const long long at = (long long)s * a.total + (long long)e;
        a.out[at] = nq_level(D, valid, u, nbq_normal_quantile(u), w, bad);
        if (a.uout) a.uout[at] = u;
      }
    }
  }
  NQ_RAISE(a.flag, bad);
}

extern "C" int ftn_nb_sample_form(int N, long long rate_bstride, long long disp_bstride, int misalign_or) {
  FTN_CHECK_ARG(N >= 1, "ftn_nb_sample_form: N=%d", N);
  FTN_CHECK_ARG(rate_bstride >= 0 && disp_bstride >= 0 && misalign_ok(misalign_or),
                "ftn_nb_sample_form: strides %lld %lld misalign=%d", rate_bstride, disp_bstride, misalign_or);
  return nbq_form(N, 0, rate_bstride, disp_bstride, (unsigned)misalign_or);
}

extern "C" int ftn_nb_sample(const float* rate_dev, long long rate_bstride, const float* disp_dev,
                             long long disp_bstride, int B, int H, int N, int S, unsigned long long seed,
                             const unsigned long long* seed_dev, unsigned offset, float eps, float* out_dev,
                             double* u_out_dev, int* flag_dev, void* stream) {
  FTN_CHECK_ARG(rate_dev && disp_dev && out_dev && flag_dev, "ftn_nb_sample: null pointer");
  FTN_CHECK_ARG(S >= 1, "ftn_nb_sample: S=%d", S);
  if (nbq_check("ftn_nb_sample", B, H, N, {rate_bstride, disp_bstride}, eps) < 0) return -1;
  FTN_CHECK_ARG((((uintptr_t)rate_dev | (uintptr_t)disp_dev | (uintptr_t)out_dev | (uintptr_t)flag_dev) & 3) == 0 &&
                    (((uintptr_t)u_out_dev | (uintptr_t)seed_dev) & 7) == 0,
                "ftn_nb_sample: operands must be 4-byte aligned, u_out and seed_dev 8-byte aligned");
  const unsigned mis = (unsigned)(((uintptr_t)rate_dev | (uintptr_t)disp_dev) & 15);
  NbsArgs a = {};
  a.rate = rate_dev; a.disp = disp_dev; a.out = out_dev; a.uout = u_out_dev; a.flag = flag_dev;
  a.seed_dev = seed_dev; a.seed = seed; a.offset = offset;
  a.rbs = B > 1 ? rate_bstride : 0; a.dbs = B > 1 ? disp_bstride : 0;
  a.HN = (long long)H * N; a.total = (long long)B * a.HN; a.eps = eps; a.S = S;
  NBQ_LAUNCH(k_nb_sample, nbq_form(N, 0, a.rbs, a.dbs, mis), a, stream);
  return 0;
}
