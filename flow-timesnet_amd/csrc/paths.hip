// Summaries of sample paths: per output element (b, h', n) of samples [P][B][H][N] the order statistics at given
// ranks, the mean, the sample CRPS against y and, on request, the sorted column - one read of the paths, window sums
// or maxima formed on the fly, nothing intermediate in HBM (include/flowtimes.h states the definitions).
//
// Order: a value becomes an unsigned key that sorts as torch.sort sorts floats (-inf .. -0 < +0 .. +inf < NaN, every
// NaN the one key PK_NAN) and the padding up to the network's size is PK_PAD above that, so ONE integer min / max
// network is a total order: nothing is dropped the way fminf / fmaxf drop a NaN (ftn_median.h), and a key decodes to
// the bits it came from.
//   k_path_reg<PP, CPL>  P <= 64: a lane owns CPL columns (4 with 16-byte loads and PP <= 16, else 1; consecutive n on
//                        consecutive lanes) and their PP = 2 .. 64 keys in registers; the bitonic network is unrolled
//                        on the lane's own registers: no cross-lane traffic, no LDS
//   k_path_lds<CPL>      P <= 1024: a workgroup owns a tile of T consecutive columns as keys [PP][T] in LDS (columns
//                        along the banks), PP = 128 .. 1024, PP T 4 <= 64 KiB; a thread takes 2^NB rows of one column
//                        that differ in NB <= 3 consecutive index bits into registers and runs NB network steps on
//                        them, so a stage of m steps costs ceil(m / 3) passes over the tile instead of m
// Sums (mean, A, G) run over the SORTED column in ascending rank; in the LDS form a thread takes the ranks
// r, r + R, ... of its column and the R partial sums are added in ascending r: the order is a function of PP alone.
// Neither kernel has a data-dependent loop, an atomic or a store outside its own elements.
#include "ftn_common.h"

#define PK_NAN 0xFFC00000u   // above +inf (0xFF800000); decodes to the quiet NaN 0x7FC00000
#define PK_PAD 0xFFFFFFFFu
#define PL_THREADS 256
#define PL_LDS_BYTES 65536

struct PathArgs {
  const float* x;  const float* y;
  float* q;  float* mean;  float* crps;  float* sorted;
  long long ps, bs, ybs;       // path and batch strides of x, batch stride of y, in elements
  long long E;                 // B H' N
  int P, N, HpN, window, reduce, Q;
  int rank[FTN_QMAX];          // 1 .. P
};

__host__ __device__ inline unsigned pk_key(float v) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return v != v ? PK_NAN : k;
}
__host__ __device__ inline float pk_val(unsigned k) {
  const unsigned u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  return __builtin_bit_cast(float, u);
}
__host__ __device__ inline void pk_cx(unsigned& a, unsigned& b, bool asc) {
  const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
  a = asc ? lo : hi;
  b = asc ? hi : lo;
}

// the bitonic network on PP keys of one owner, ascending
template <int PP>
__host__ __device__ inline void pk_sort(unsigned (&k)[PP]) {
#pragma unroll
  for (int s = 2; s <= PP; s <<= 1)
#pragma unroll
    for (int j = s >> 1; j > 0; j >>= 1)
#pragma unroll
      for (int i = 0; i < PP; ++i)
        if ((i & j) == 0) pk_cx(k[i], k[i | j], (i & s) == 0);
}

// One pass of stage s over a [PP][T] tile: thread `tid` of PL_THREADS takes, per item, the 2^NB rows of one column that
// differ in the index bits of the distances jtop, jtop / 2, .. jlow = jtop >> (NB - 1) and runs those NB steps.
// s >= 2 jtop, so the direction (row & s) is one for the whole item.
template <int NB>
__host__ __device__ inline void pl_pass(unsigned* t, int T, int tsh, int PP, int s, int jtop, int tid) {
  constexpr int R = 1 << NB;
  const int jlow = jtop >> (NB - 1);
  const int items = (PP >> NB) << tsh;
  for (int w = tid; w < items; w += PL_THREADS) {
    const int c = w & (T - 1), g = w >> tsh;
    const int base = ((g & ~(jlow - 1)) << NB) | (g & (jlow - 1));
    const bool asc = (base & s) == 0;
    unsigned v[R];
#pragma unroll
    for (int u = 0; u < R; ++u) v[u] = t[((base + u * jlow) << tsh) + c];
#pragma unroll
    for (int bit = R >> 1; bit > 0; bit >>= 1)
#pragma unroll
      for (int u = 0; u < R; ++u)
        if ((u & bit) == 0) pk_cx(v[u], v[u | bit], asc);
#pragma unroll
    for (int u = 0; u < R; ++u) t[((base + u * jlow) << tsh) + c] = v[u];
  }
}

// the passes of the whole network, `sync` between them
template <class Sync>
__host__ __device__ inline void pl_sort(unsigned* t, int T, int tsh, int PP, int tid, Sync sync) {
  for (int s = 2; s <= PP; s <<= 1) {
    int j = s >> 1;
    while (j > 0) {
      if (j >= 4) { pl_pass<3>(t, T, tsh, PP, s, j, tid); j >>= 3; }
      else if (j == 2) { pl_pass<2>(t, T, tsh, PP, s, j, tid); j = 0; }
      else { pl_pass<1>(t, T, tsh, PP, s, j, tid); j = 0; }
      sync();
    }
  }
}

// The form every entry point takes (include/flowtimes.h): the one place the choice is made.
static inline int path_form(int P, int N, long long ps, long long bs, long long ybs, unsigned misalign_or) {
  int pp = 2;
  while (pp < P) pp <<= 1;
  const bool lds = pp > 64;
  const bool aligned = N % 4 == 0 && ps % 4 == 0 && bs % 4 == 0 && ybs % 4 == 0 && (misalign_or & 15) == 0;
  const bool vec = aligned && (lds || pp <= 16);               // 4 columns of 32 or 64 keys do not fit a lane
  int T = 0;
  if (lds) {
    T = PL_LDS_BYTES / 4 / pp;
    if (T > 64) T = 64;
  }
  return (vec ? FTN_SHELL_VEC : 0) | (lds ? FTN_PATH_LDS : 0) | pp << 8 | T << 20;
}

template <int CPL>
__device__ __forceinline__ f4 pk_load(const float* p) {
  if (CPL == 4) return *(const f4*)p;
  return f4{*p, 0.f, 0.f, 0.f};
}
template <int CPL>
__device__ __forceinline__ void pk_store(float* p, const float (&v)[CPL]) {
  if constexpr (CPL == 4) *(f4*)p = f4{v[0], v[1], v[2], v[3]};
  else *p = v[0];
}
__device__ __forceinline__ float pk_elem(f4 v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }
// torch.amax: a NaN stays
__device__ __forceinline__ float pk_max(float m, float v) { return (v > m || v != v) ? v : m; }

// offset of element e's first window row in a [B][H][N] operand of batch stride bs
__device__ __forceinline__ long long pk_offset(const PathArgs& a, long long e, long long bs) {
  const long long b = e / a.HpN;
  const int r = (int)(e - b * a.HpN), hp = r / a.N, n = r - hp * a.N;
  return b * bs + (long long)hp * a.window * a.N + n;
}

// (A P - G) / P^2 and S / P: one fp64 product, difference and division each, then one rounding to fp32
__device__ __forceinline__ float pk_crps(double A, double G, int P) {
  return (float)__ddiv_rn(__dsub_rn(__dmul_rn(A, (double)P), G), (double)P * (double)P);
}

template <int PP, int CPL>
__global__ __launch_bounds__(PL_THREADS) void k_path_reg(PathArgs a) {
  const long long e0 = ((long long)blockIdx.x * PL_THREADS + threadIdx.x) * CPL;
  if (e0 >= a.E) return;                                        // CPL == 4: E % 4 == 0, a quad has one row
  constexpr int CH = PP * CPL <= 16 ? PP : 16 / CPL;            // paths in flight per lane
  const float* base = a.x + pk_offset(a, e0, a.bs);
  const bool sum = a.reduce == FTN_PATH_SUM;
  unsigned key[CPL][PP];
#pragma unroll
  for (int c0 = 0; c0 < PP; c0 += CH) {
    double s[CH][CPL];
    float m[CH][CPL];
#pragma unroll
    for (int u = 0; u < CH; ++u)
#pragma unroll
      for (int c = 0; c < CPL; ++c) { s[u][c] = 0.0; m[u][c] = -INFINITY; }
    for (int j = 0; j < a.window; ++j) {
#pragma unroll
      for (int u = 0; u < CH; ++u) {                            // a path beyond P re-reads path P - 1: no branch
        const int p = c0 + u < a.P ? c0 + u : a.P - 1;
        const f4 v = pk_load<CPL>(base + p * a.ps + (long long)j * a.N);
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
          const float t = pk_elem(v, c);
          if (sum) s[u][c] += (double)t;
          else m[u][c] = pk_max(m[u][c], t);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < CH; ++u)
#pragma unroll
      for (int c = 0; c < CPL; ++c)
        key[c][c0 + u] = c0 + u < a.P ? pk_key(sum ? (float)s[u][c] : m[u][c]) : PK_PAD;
  }
#pragma unroll
  for (int c = 0; c < CPL; ++c) pk_sort<PP>(key[c]);

  for (int i = 0; i < a.Q; ++i) {
    const int r = a.rank[i] - 1;
    float out[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      unsigned k = key[c][0];
#pragma unroll
      for (int p = 1; p < PP; ++p) k = r == p ? key[c][p] : k;
      out[c] = pk_val(k);
    }
    pk_store<CPL>(a.q + i * a.E + e0, out);
  }
  if (a.sorted) {
#pragma unroll
    for (int p = 0; p < PP; ++p) {
      if (p < a.P) {
        float out[CPL];
#pragma unroll
        for (int c = 0; c < CPL; ++c) out[c] = pk_val(key[c][p]);
        pk_store<CPL>(a.sorted + p * a.E + e0, out);
      }
    }
  }
  if (a.mean) {
    float out[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      double S = 0.0;
#pragma unroll
      for (int p = 0; p < PP; ++p)
        if (p < a.P) S += (double)pk_val(key[c][p]);
      out[c] = (float)__ddiv_rn(S, (double)a.P);
    }
    pk_store<CPL>(a.mean + e0, out);
  }
  if (a.crps) {
    const float* yb = a.y + pk_offset(a, e0, a.ybs);
    double ys[CPL];
    float ym[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) { ys[c] = 0.0; ym[c] = -INFINITY; }
    for (int j = 0; j < a.window; ++j) {
      const f4 v = pk_load<CPL>(yb + (long long)j * a.N);
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        ys[c] += (double)pk_elem(v, c);
        ym[c] = pk_max(ym[c], pk_elem(v, c));
      }
    }
    float out[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const double yw = (double)(sum ? (float)ys[c] : ym[c]);
      double A = 0.0, G = 0.0;
#pragma unroll
      for (int p = 0; p < PP; ++p) {
        if (p < a.P) {
          const double xv = (double)pk_val(key[c][p]);
          A += fabs(xv - yw);
          G += __dmul_rn((double)(2 * p + 1 - a.P), xv);        // (2 i - P - 1) x(i), i = p + 1: the product is exact
        }
      }
      out[c] = pk_crps(A, G, a.P);
    }
    pk_store<CPL>(a.crps + e0, out);
  }
}

template <int CPL>
__global__ __launch_bounds__(PL_THREADS) void k_path_lds(PathArgs a, int PP, int tsh) {
  extern __shared__ __attribute__((aligned(16))) unsigned tile[];          // [PP][T]; later the partial sums
  const int tid = threadIdx.x, T = 1 << tsh;
  const long long tile0 = (long long)blockIdx.x * T;
  const bool sum = a.reduce == FTN_PATH_SUM;
  {                                                             // stage: thread -> CPL columns, rows r0, r0 + RS, ..
    const int TC = T / CPL, cs = (tid % TC) * CPL, r0 = tid / TC, RS = PL_THREADS / TC;
    const bool live = tile0 + cs < a.E;                         // CPL == 4: E % 4 == 0, so a quad is whole
    const float* base = a.x + (live ? pk_offset(a, tile0 + cs, a.bs) : 0);   // idle columns read element 0's window
    for (int p0 = r0; p0 < PP; p0 += 4 * RS) {                  // PP % (4 RS) == 0 (host)
      double s[4][CPL];
      float m[4][CPL];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < CPL; ++c) { s[u][c] = 0.0; m[u][c] = -INFINITY; }
      for (int j = 0; j < a.window; ++j) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int p = p0 + u * RS < a.P ? p0 + u * RS : a.P - 1;
          const f4 v = pk_load<CPL>(base + p * a.ps + (long long)j * a.N);
#pragma unroll
          for (int c = 0; c < CPL; ++c) {
            const float t = pk_elem(v, c);
            if (sum) s[u][c] += (double)t;
            else m[u][c] = pk_max(m[u][c], t);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = p0 + u * RS;
#pragma unroll
        for (int c = 0; c < CPL; ++c)
          tile[(p << tsh) + cs + c] = live && p < a.P ? pk_key(sum ? (float)s[u][c] : m[u][c]) : PK_PAD;
      }
    }
  }
  __syncthreads();
  pl_sort(tile, T, tsh, PP, tid, [] { __syncthreads(); });

  // thread -> column c, ranks r, r + R, ..
  const int c = tid & (T - 1), r = tid >> tsh, R = PL_THREADS >> tsh;
  const long long e = tile0 + c;
  const bool live = e < a.E;
  if (live) {
    for (int i = r; i < a.Q; i += R) a.q[i * a.E + e] = pk_val(tile[((a.rank[i] - 1) << tsh) + c]);
    if (a.sorted)
      for (int p = r; p < a.P; p += R) a.sorted[p * a.E + e] = pk_val(tile[(p << tsh) + c]);
  }
  double S = 0.0, A = 0.0, G = 0.0;
  if (a.mean || a.crps) {
    double yw = 0.0;
    if (a.crps && live) {
      const float* yb = a.y + pk_offset(a, e, a.ybs);
      double ys = 0.0;
      float ym = -INFINITY;
      for (int j = 0; j < a.window; ++j) {
        const float v = yb[(long long)j * a.N];
        ys += (double)v;
        ym = pk_max(ym, v);
      }
      yw = (double)(sum ? (float)ys : ym);
    }
    for (int p = r; p < a.P; p += R) {
      const double xv = (double)pk_val(tile[(p << tsh) + c]);
      S += xv;
      A += fabs(xv - yw);
      G += __dmul_rn((double)(2 * p + 1 - a.P), xv);
    }
    __syncthreads();                                            // every key has been read: the tile becomes [3][R][T] fp64
    double* part = (double*)tile;
    part[(0 * R + r) * T + c] = S;
    part[(1 * R + r) * T + c] = A;
    part[(2 * R + r) * T + c] = G;
    __syncthreads();
    if (r == 0 && live) {
      for (int k = 1; k < R; ++k) {
        S += part[(0 * R + k) * T + c];
        A += part[(1 * R + k) * T + c];
        G += part[(2 * R + k) * T + c];
      }
      if (a.mean) a.mean[e] = (float)__ddiv_rn(S, (double)a.P);
      if (a.crps) a.crps[e] = pk_crps(A, G, a.P);
    }
  }
}

template <int PP>
static void path_launch_reg(bool vec, dim3 grid, hipStream_t st, const PathArgs& a) {
  if constexpr (PP <= 16) {
    if (vec) { hipLaunchKernelGGL((k_path_reg<PP, 4>), grid, dim3(PL_THREADS), 0, st, a); return; }
  }
  hipLaunchKernelGGL((k_path_reg<PP, 1>), grid, dim3(PL_THREADS), 0, st, a);
}

static int path_form_check(const char* who, int P, int N, int window, long long ps, long long bs, long long ybs) {
  FTN_CHECK_ARG(P >= 1 && P <= FTN_PATHS_MAX, "%s: P=%d is outside 1..%d", who, P, FTN_PATHS_MAX);
  FTN_CHECK_ARG(N >= 1 && window >= 1, "%s: N=%d window=%d", who, N, window);
  FTN_CHECK_ARG(ps >= 0 && bs >= 0 && ybs >= 0, "%s: negative stride %lld %lld %lld", who, ps, bs, ybs);
  return 0;
}

extern "C" int ftn_path_summary_form(int P, int N, int window, long long p_stride, long long b_stride,
                                     long long y_bstride, int misalign_or) {
  if (path_form_check("ftn_path_summary_form", P, N, window, p_stride, b_stride, y_bstride) < 0) return -1;
  FTN_CHECK_ARG(misalign_ok(misalign_or), "ftn_path_summary_form: misalign=%d", misalign_or);
  return path_form(P, N, p_stride, b_stride, y_bstride, (unsigned)misalign_or);
}

extern "C" int ftn_path_summary(const float* samples_dev, long long p_stride, long long b_stride, int P, int B, int H,
                                int N, int window, int reduce, const float* y_dev, long long y_bstride,
                                const int* ranks_host, int Q, float* q_out_dev, float* mean_out_dev,
                                float* crps_out_dev, float* sorted_out_dev, void* stream) {
  const char* who = "ftn_path_summary";
  FTN_CHECK_ARG(samples_dev, "%s: null samples", who);
  if (path_form_check(who, P, N, window, p_stride, b_stride, y_bstride) < 0) return -1;
  FTN_CHECK_ARG(B >= 1 && H >= 1 && H % window == 0, "%s: bad shape B=%d H=%d window=%d", who, B, H, window);
  FTN_CHECK_ARG(reduce == FTN_PATH_SUM || reduce == FTN_PATH_MAX, "%s: reduce=%d", who, reduce);
  const long long row = (long long)H * N, E = (long long)B * (H / window) * N;
  FTN_CHECK_ARG(row <= 0x7fffffffLL && E <= 0x7fffffffLL, "%s: H N = %lld or B H' N = %lld beyond int32", who, row, E);
  FTN_CHECK_ARG(B == 1 || (b_stride >= row && (!y_dev || y_bstride >= row)),
                "%s: batch strides %lld %lld are below H N = %lld", who, b_stride, y_bstride, row);
  const long long span = (B - 1) * (B > 1 ? b_stride : 0) + row;
  FTN_CHECK_ARG(P == 1 || p_stride >= span, "%s: path stride %lld is below a path's span %lld", who, p_stride, span);
  FTN_CHECK_ARG(Q >= 0 && Q <= FTN_QMAX, "%s: Q=%d is outside 0..%d", who, Q, FTN_QMAX);
  FTN_CHECK_ARG(Q == 0 || (ranks_host && q_out_dev), "%s: Q=%d needs ranks and q_out", who, Q);
  for (int i = 0; i < Q; ++i)
    FTN_CHECK_ARG(ranks_host[i] >= 1 && ranks_host[i] <= P, "%s: rank %d is outside 1..%d", who, ranks_host[i], P);
  FTN_CHECK_ARG(!crps_out_dev || y_dev, "%s: crps_out needs y", who);
  FTN_CHECK_ARG(Q > 0 || mean_out_dev || crps_out_dev || sorted_out_dev, "%s: no output requested", who);
  const uintptr_t all = (uintptr_t)samples_dev | (uintptr_t)y_dev | (uintptr_t)q_out_dev | (uintptr_t)mean_out_dev |
                        (uintptr_t)crps_out_dev | (uintptr_t)sorted_out_dev;
  FTN_CHECK_ARG((all & 3) == 0, "%s: operands must be 4-byte aligned", who);
  PathArgs a = {};
  a.x = samples_dev; a.y = crps_out_dev ? y_dev : nullptr;
  a.q = Q ? q_out_dev : nullptr; a.mean = mean_out_dev; a.crps = crps_out_dev; a.sorted = sorted_out_dev;
  a.ps = P > 1 ? p_stride : 0; a.bs = B > 1 ? b_stride : 0; a.ybs = B > 1 && a.y ? y_bstride : 0;
  a.E = E; a.P = P; a.N = N; a.HpN = (H / window) * N; a.window = window; a.reduce = reduce; a.Q = Q;
  for (int i = 0; i < Q; ++i) a.rank[i] = ranks_host[i];
  const uintptr_t used = (uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.q | (uintptr_t)a.mean | (uintptr_t)a.crps |
                         (uintptr_t)a.sorted;
  const int form = path_form(P, N, a.ps, a.bs, a.ybs, (unsigned)(used & 15));
  const bool vec = form & FTN_SHELL_VEC;
  const int PP = (form >> 8) & 0xfff;
  hipStream_t st = (hipStream_t)stream;
  if (form & FTN_PATH_LDS) {
    const int T = form >> 20;
    int tsh = 0;
    while ((1 << tsh) < T) ++tsh;
    const int rs = PL_THREADS / (T / (vec ? 4 : 1));
    FTN_CHECK_ARG((1 << tsh) == T && PP % (4 * rs) == 0 && PP * T * 4 <= PL_LDS_BYTES &&
                      3 * PL_THREADS * 8 <= PP * T * 4,
                  "%s: tile PP=%d T=%d", who, PP, T);
    const dim3 grid((unsigned)((E + T - 1) / T));
    const size_t lds = (size_t)PP * T * 4;
    if (vec) hipLaunchKernelGGL(k_path_lds<4>, grid, dim3(PL_THREADS), lds, st, a, PP, tsh);
    else hipLaunchKernelGGL(k_path_lds<1>, grid, dim3(PL_THREADS), lds, st, a, PP, tsh);
  } else {
    const long long per = (long long)PL_THREADS * (vec ? 4 : 1);
    const dim3 grid((unsigned)((E + per - 1) / per));
    switch (PP) {
      case 2: path_launch_reg<2>(vec, grid, st, a); break;
      case 4: path_launch_reg<4>(vec, grid, st, a); break;
      case 8: path_launch_reg<8>(vec, grid, st, a); break;
      case 16: path_launch_reg<16>(vec, grid, st, a); break;
      case 32: path_launch_reg<32>(vec, grid, st, a); break;
      default: path_launch_reg<64>(vec, grid, st, a); break;
    }
  }
  FTN_CHECK_LAUNCH();
  return 0;
}
