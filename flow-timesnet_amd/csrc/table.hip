// Table preparation on the device (include/flowtimes.h, "table preparation"): what the reference does to the wide
// table [T][N] between the CSV and the loader, and to the forecast after the model.
//
//   k_tab_moments / k_tab_mean / k_tab_fin   ftn_table_moments: column count, sum, mean, centred sum of squares, min,
//                                        max (and the same of first differences): two passes over the table, the
//                                        means finished between them
//   k_tab_twiddle                        the T twiddles of the full-history DFT, fp64 evaluated, fp32 rounded
//   k_tab_spectrum / k_tab_spec_fin      ftn_table_spectrum: the DFT of every demeaned column as a GEMM on
//                                        v_mfma_f32_32x32x2_f32, peak bin, peak power and total power per column
//   k_tab_features / k_tab_scaler        the reference's finishing arithmetic of the five features and of the scaler
//   k_tab_affine                         ftn_table_affine: (x - loc) / scale or x * scale + loc over [outer][S][inner]
//
// Orders of summation (all fixed by the shape, none by the grid; no floating-point atomics):
//   moments   a thread owns a column and a block of `rb` consecutive rows (rb = 32 doubled until at most 32 blocks
//             cover T) and adds its rows ascending in fp64; the blocks' partials are added ascending in fp64.
//   spectrum  one MFMA accumulator per (bin, column) over t ascending in k-steps of two; a lane adds the powers of its
//             16 bins ascending in fp64, then half-wave 0 + half-wave 1, then the four waves of a 128-bin block
//             ascending, then the bin blocks ascending.  The peak takes the lowest bin among equals at every step.
// Nothing in this file is contracted into an FMA: ftn_table_affine promises one rounding per operation.
#include <math.h>
#include "ftn_common.h"

#pragma clang fp contract(off)

#define TAB_THREADS 256
#define TAB_GRID_MAX 4096
#define TAB_AFF_CHUNK 1024
#define TAB_T_MAX 65536

static bool tab_mul(long long a, long long b, long long* out) {
  return !__builtin_mul_overflow(a, b, out) && *out <= (1LL << 61);
}
static inline bool tab_aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// ---------------------------------------------------------------- moments
// rows a block: 32, doubled until at most FTN_TAB_PARTIALS_MAX blocks cover T
static long long tab_row_block(long long T) {
  long long rb = 32;
  while ((T + rb - 1) / rb > FTN_TAB_PARTIALS_MAX) rb *= 2;
  return rb;
}

struct TabMom {
  const float* X; const float* M;
  long long xs, ms, T, rb, units;
  int N, nrb, clip, diff, tile;                                 // tile: columns a workgroup (256 V)
  double* pa;                                                   // [nrb][8][N] cnt, sum, min, max and the differences'
  double* pb;                                                   // [nrb][2][N] centred sums of squares
  double* stats;                                                // [6 | 12][N]
};

// min and max as numpy's: a NaN is kept once met
__device__ __forceinline__ float tab_min(float m, float v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ float tab_max(float m, float v) { return (v > m || v != v) ? v : m; }

template <int V>
__device__ __forceinline__ void tab_load(const float* p, float (&v)[V]) {
  if (V == 4) { const f4 q = *(const f4*)p; v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
  else v[0] = *p;
}

// Row r of the thread's V columns: the values (clipped when asked) and whether each counts.
template <int V>
__device__ __forceinline__ void tab_row(const TabMom& a, long long r, long long c, float (&x)[V], bool (&ok)[V]) {
  tab_load<V>(a.X + r * a.xs + c, x);
  if (a.M != nullptr) {
    float m[V];
    tab_load<V>(a.M + r * a.ms + c, m);
#pragma unroll
    for (int v = 0; v < V; ++v) ok[v] = m[v] > 0.0f;
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) ok[v] = true;
  }
  if (a.clip) {
#pragma unroll
    for (int v = 0; v < V; ++v) x[v] = x[v] < 0.0f ? 0.0f : x[v];
  }
}

// The mean of a column from the row blocks' partials, rounded to fp32 once; NaN when the sum is not finite.
__device__ __forceinline__ float tab_mean(const double* pa, int nrb, int N, long long c, int k, double* cnt_out,
                                          double* sum_out) {
  double cnt = 0.0, sum = 0.0;
  for (int b = 0; b < nrb; ++b) {
    cnt += pa[((long long)b * 8 + k) * N + c];
    sum += pa[((long long)b * 8 + k + 1) * N + c];
  }
  *cnt_out = cnt; *sum_out = sum;
  if (!(fabs(sum) <= 1.7976931348623157e308)) return NAN;
  return (float)(sum / (cnt > 1.0 ? cnt : 1.0));
}

template <int V, bool CSS>
__global__ __launch_bounds__(TAB_THREADS) void k_tab_moments(TabMom a) {
  const int nct = (a.N + a.tile - 1) / a.tile;
  for (long long unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
    const int rbi = (int)(unit / nct);
    const long long c = (unit - (long long)rbi * nct) * a.tile + (long long)threadIdx.x * V;
    if (c >= a.N) continue;                                     // N % 4 == 0 when V == 4: a quad is inside or outside
    const long long r0 = rbi * a.rb, r1 = r0 + a.rb < a.T ? r0 + a.rb : a.T;
    float mean[V], dmean[V];
    if (CSS) {                                                  // the means k_tab_mean left in the statistics
#pragma unroll
      for (int v = 0; v < V; ++v) {
        mean[v] = (float)a.stats[2LL * a.N + c + v];
        dmean[v] = a.diff ? (float)a.stats[8LL * a.N + c + v] : 0.0f;
      }
    }
    double acc0[V], acc1[V], dacc0[V], dacc1[V];                // pass 1: count and sum; pass 2: css (acc0)
    float mn[V], mx[V], dmn[V], dmx[V], xp[V];
    bool okp[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      acc0[v] = acc1[v] = dacc0[v] = dacc1[v] = 0.0;
      mn[v] = dmn[v] = INFINITY; mx[v] = dmx[v] = -INFINITY; xp[v] = 0.0f; okp[v] = false;
    }
    if (a.diff && r0 > 0) tab_row<V>(a, r0 - 1, c, xp, okp);
    for (long long r = r0; r < r1; ++r) {
      float x[V];
      bool ok[V];
      tab_row<V>(a, r, c, x, ok);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (ok[v]) {
          if (CSS) {
            const float d = x[v] - mean[v];                     // formed in fp32, as the reference forms it
            acc0[v] += (double)d * (double)d;
          } else {
            acc0[v] += 1.0; acc1[v] += (double)x[v];
            mn[v] = tab_min(mn[v], x[v]); mx[v] = tab_max(mx[v], x[v]);
          }
        }
        if (a.diff && ok[v] && okp[v]) {                        // okp is false in front of the table's first row
          const float dx = x[v] - xp[v];
          if (CSS) {
            const float d = dx - dmean[v];
            dacc0[v] += (double)d * (double)d;
          } else {
            dacc0[v] += 1.0; dacc1[v] += (double)dx;
            dmn[v] = tab_min(dmn[v], dx); dmx[v] = tab_max(dmx[v], dx);
          }
        }
        xp[v] = x[v]; okp[v] = ok[v];
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (CSS) {
        double* p = a.pb + (long long)rbi * 2 * a.N + c + v;
        p[0] = acc0[v]; p[1LL * a.N] = dacc0[v];
      } else {
        double* p = a.pa + (long long)rbi * 8 * a.N + c + v;
        p[0] = acc0[v]; p[1LL * a.N] = acc1[v]; p[2LL * a.N] = (double)mn[v]; p[3LL * a.N] = (double)mx[v];
        p[4LL * a.N] = dacc0[v]; p[5LL * a.N] = dacc1[v]; p[6LL * a.N] = (double)dmn[v]; p[7LL * a.N] = (double)dmx[v];
      }
    }
  }
}

// Between the passes: a thread a column adds the row blocks' partials ascending and writes count, sum, mean, min and max
// (and the differences') once, so the second pass reads one mean a column, not every partial.
__global__ __launch_bounds__(TAB_THREADS) void k_tab_mean(TabMom a) {
  for (long long c = (long long)blockIdx.x * TAB_THREADS + threadIdx.x; c < a.N; c += (long long)gridDim.x * TAB_THREADS) {
    double cnt, sum, dcnt = 0.0, dsum = 0.0;
    const float mean = tab_mean(a.pa, a.nrb, a.N, c, 0, &cnt, &sum);
    const float dmean = a.diff ? tab_mean(a.pa, a.nrb, a.N, c, 4, &dcnt, &dsum) : 0.0f;
    float mn = INFINITY, mx = -INFINITY, dmn = INFINITY, dmx = -INFINITY;
    for (int b = 0; b < a.nrb; ++b) {
      const double* p = a.pa + (long long)b * 8 * a.N + c;
      mn = tab_min(mn, (float)p[2LL * a.N]); mx = tab_max(mx, (float)p[3LL * a.N]);
      if (a.diff) { dmn = tab_min(dmn, (float)p[6LL * a.N]); dmx = tab_max(dmx, (float)p[7LL * a.N]); }
    }
    double* s = a.stats + c;
    s[0] = cnt; s[1LL * a.N] = sum; s[2LL * a.N] = (double)mean; s[4LL * a.N] = (double)mn; s[5LL * a.N] = (double)mx;
    if (a.diff) {
      s[6LL * a.N] = dcnt; s[7LL * a.N] = dsum; s[8LL * a.N] = (double)dmean; s[10LL * a.N] = (double)dmn;
      s[11LL * a.N] = (double)dmx;
    }
  }
}

__global__ __launch_bounds__(TAB_THREADS) void k_tab_fin(TabMom a) {
  for (long long c = (long long)blockIdx.x * TAB_THREADS + threadIdx.x; c < a.N; c += (long long)gridDim.x * TAB_THREADS) {
    double css = 0.0, dcss = 0.0;
    for (int b = 0; b < a.nrb; ++b) {
      css += a.pb[(long long)b * 2 * a.N + c];
      dcss += a.pb[((long long)b * 2 + 1) * a.N + c];
    }
    a.stats[3LL * a.N + c] = css;
    if (a.diff) a.stats[9LL * a.N + c] = dcss;
  }
}

static int mom_plan(const char* who, const FtnTableMomentsArgs* a, TabMom* k, FtnTableForm* form) {
  FTN_CHECK_ARG(a != nullptr, "%s: null arguments", who);
  FTN_CHECK_ARG(a->T >= 1 && a->N >= 1, "%s: T=%lld, N=%d must be positive", who, a->T, a->N);
  FTN_CHECK_ARG((a->flags & ~(FTN_TAB_CLIP | FTN_TAB_MASK | FTN_TAB_DIFF)) == 0, "%s: flags=%d has bits outside "
                "FTN_TAB_CLIP | FTN_TAB_MASK | FTN_TAB_DIFF", who, a->flags);
  FTN_CHECK_ARG(a->X != nullptr, "%s: null X", who);
  FTN_CHECK_ARG(a->x_stride >= a->N, "%s: X row stride %lld is below N=%d", who, a->x_stride, a->N);
  const bool masked = (a->flags & FTN_TAB_MASK) != 0;
  FTN_CHECK_ARG(!masked || a->M != nullptr, "%s: FTN_TAB_MASK without M", who);
  FTN_CHECK_ARG(!masked || a->m_stride >= a->N, "%s: M row stride %lld is below N=%d", who, a->m_stride, a->N);
  FTN_CHECK_ARG(((((uintptr_t)a->X | (uintptr_t)a->M)) & 3) == 0, "%s: tables must be 4-byte aligned", who);
  long long reach = 0;
  FTN_CHECK_ARG(tab_mul(a->T, a->x_stride, &reach) && (!masked || tab_mul(a->T, a->m_stride, &reach)),
                "%s: T=%lld rows at the given strides pass 64 bits", who, a->T);
  const bool vec = a->N % 4 == 0 && a->x_stride % 4 == 0 && tab_aligned16(a->X) &&
                   (!masked || (a->m_stride % 4 == 0 && tab_aligned16(a->M)));
  k->X = a->X; k->M = masked ? a->M : nullptr; k->xs = a->x_stride; k->ms = a->m_stride; k->T = a->T; k->N = a->N;
  k->rb = tab_row_block(a->T); k->nrb = (int)((a->T + k->rb - 1) / k->rb);
  k->clip = (a->flags & FTN_TAB_CLIP) != 0; k->diff = (a->flags & FTN_TAB_DIFF) != 0;
  k->tile = TAB_THREADS * (vec ? 4 : 1);
  k->units = (long long)k->nrb * ((a->N + k->tile - 1) / k->tile);
  if (form != nullptr) {
    *form = FtnTableForm{};
    form->load_bytes = vec ? 16 : 4; form->col_tile = k->tile;
    form->block = (int)(k->rb < 0x7fffffffLL ? k->rb : 0x7fffffffLL); form->partials = k->nrb;
  }
  return vec ? 1 : 0;
}

extern "C" size_t ftn_table_moments_bytes(long long T, int N) {
  if (T < 1 || N < 1) return 0;
  const long long nrb = (T + tab_row_block(T) - 1) / tab_row_block(T);
  return (size_t)nrb * 10 * (size_t)N * sizeof(double);
}

extern "C" int ftn_table_moments_form(const FtnTableMomentsArgs* a, FtnTableForm* form) {
  FTN_CHECK_ARG(form != nullptr, "ftn_table_moments_form: null form");
  TabMom k = {};
  return mom_plan("ftn_table_moments_form", a, &k, form) < 0 ? -1 : 0;
}

extern "C" int ftn_table_moments(const FtnTableMomentsArgs* a, void* stream) {
  const char* who = "ftn_table_moments";
  TabMom k = {};
  const int vec = mom_plan(who, a, &k, nullptr);
  if (vec < 0) return -1;
  FTN_CHECK_ARG(a->stats != nullptr && (((uintptr_t)a->stats) & 7) == 0, "%s: stats must be an 8-byte aligned buffer", who);
  FTN_CHECK_ARG(a->workspace != nullptr && (((uintptr_t)a->workspace) & 7) == 0 &&
                    a->workspace_bytes >= ftn_table_moments_bytes(a->T, a->N),
                "%s: the workspace holds %zu bytes, ftn_table_moments_bytes asks for %zu (8-byte aligned)", who,
                a->workspace_bytes, ftn_table_moments_bytes(a->T, a->N));
  k.pa = (double*)a->workspace; k.pb = k.pa + (size_t)k.nrb * 8 * a->N; k.stats = a->stats;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(k.units < TAB_GRID_MAX ? k.units : TAB_GRID_MAX));
  if (vec) hipLaunchKernelGGL((k_tab_moments<4, false>), grid, dim3(TAB_THREADS), 0, st, k);
  else hipLaunchKernelGGL((k_tab_moments<1, false>), grid, dim3(TAB_THREADS), 0, st, k);
  FTN_CHECK_LAUNCH();
  const int fb = ftn_cdiv(a->N, TAB_THREADS);
  const dim3 cgrid((unsigned)(fb < TAB_GRID_MAX ? fb : TAB_GRID_MAX));
  hipLaunchKernelGGL(k_tab_mean, cgrid, dim3(TAB_THREADS), 0, st, k);
  FTN_CHECK_LAUNCH();
  if (vec) hipLaunchKernelGGL((k_tab_moments<4, true>), grid, dim3(TAB_THREADS), 0, st, k);
  else hipLaunchKernelGGL((k_tab_moments<1, true>), grid, dim3(TAB_THREADS), 0, st, k);
  FTN_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_tab_fin, cgrid, dim3(TAB_THREADS), 0, st, k);
  FTN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------- twiddles
extern "C" size_t ftn_table_twiddle_bytes(long long T) {
  return T >= 1 && T <= TAB_T_MAX ? (size_t)T * 2 * sizeof(float) : 0;
}

// tw[m] = (cos, sin)(2 pi m / T), m = 0 .. T - 1: evaluated in fp64 on the reduced argument, rounded to fp32 once
__global__ void k_tab_twiddle(float* __restrict__ tw, int T) {
  for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < T; m += gridDim.x * blockDim.x) {
    const double ang = 2.0 * (double)m / (double)T;             // in units of pi
    tw[2 * m] = (float)cospi(ang);
    tw[2 * m + 1] = (float)sinpi(ang);
  }
}

extern "C" int ftn_table_twiddle_init(void* table_dev, long long T, void* stream) {
  FTN_CHECK_ARG(T >= 1 && T <= TAB_T_MAX, "ftn_table_twiddle_init: T=%lld is outside 1..%d", T, TAB_T_MAX);
  FTN_CHECK_ARG(table_dev != nullptr && (((uintptr_t)table_dev) & 7) == 0, "ftn_table_twiddle_init: the table must be "
                "an 8-byte aligned buffer");
  const int nb = ftn_cdiv((int)T, 256);
  hipLaunchKernelGGL(k_tab_twiddle, dim3(nb < 1024 ? nb : 1024), dim3(256), 0, (hipStream_t)stream, (float*)table_dev,
                     (int)T);
  FTN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------- spectrum
// A workgroup of four waves owns a unit: FTN_TAB_SPEC_COLS = 64 columns (two MFMA column tiles) and FTN_TAB_SPEC_BINS
// = 128 bins f (a wave 32 of them).  The demeaned, masked columns pass through LDS in chunks of FTN_TAB_SPEC_CHUNK =
// 128 rows, staged along the series (the contiguous direction of the table); rows of the last chunk past T are zeros
// up to the next multiple of 16, so the k-loop runs whole blocks of eight k-steps without a guard.  Lane (i, h)
// supplies the twiddle of bin f_i at t = t0 + 2 k + h: one 8-byte gather tw[(f t) mod T], the index carried as
// m += 2 f mod T with a conditional subtract (exact: every value is below 2 T <= 2^17), feeding the cos and the sin
// MFMA of both column tiles.  Units are ordered bin block fastest, so the workgroups in flight share a column tile in L2.
struct SpecPart { float peak; int f; double total; };

struct TabSpec {
  const float* X; const float* M; const float* mean; const float2* tw;
  long long xs, ms, units;
  int T, N, F, nbb, vec;
  SpecPart* part;                                               // [nbb][N]
  float* power; int* f_peak; float* peak; float* total;
};

typedef float f16acc __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(TAB_THREADS) void k_tab_spectrum(TabSpec a) {
  __shared__ __attribute__((aligned(16))) float dl[FTN_TAB_SPEC_CHUNK * FTN_TAB_SPEC_COLS];
  __shared__ SpecPart wpart[4][FTN_TAB_SPEC_COLS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const unsigned T = (unsigned)a.T;
  for (long long unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
    const long long ct = unit / a.nbb;
    const int bb = (int)(unit - ct * a.nbb);
    const long long n0 = ct * FTN_TAB_SPEC_COLS;
    const unsigned fbase = 1u + (unsigned)bb * FTN_TAB_SPEC_BINS + (unsigned)wave * 32u;
    const unsigned f = fbase + (unsigned)i;                     // <= T / 2 + 128: f t and 2 f stay far below 2^32
    const unsigned step = (2u * f) % T;
    unsigned m = h ? f % T : 0u;
    const bool two = n0 + 32 < a.N;                             // workgroup-uniform: the second column tile holds columns
    f16acc re0 = {0}, im0 = {0}, re1 = {0}, im1 = {0};
    // staging roles: VEC a quad of columns and 16 rows a pass, else a column and 4 rows a pass
    const int scol = a.vec ? (tid & 15) * 4 : (tid & 63), srow = a.vec ? tid >> 4 : tid >> 6, sstep = a.vec ? 16 : 4;
    const bool cok = n0 + scol < a.N;
    float mu[4] = {0.f, 0.f, 0.f, 0.f};
    if (cok) {
      mu[0] = a.mean[n0 + scol];
      if (a.vec) { mu[1] = a.mean[n0 + scol + 1]; mu[2] = a.mean[n0 + scol + 2]; mu[3] = a.mean[n0 + scol + 3]; }
    }
    for (int t0 = 0; t0 < a.T; t0 += FTN_TAB_SPEC_CHUNK) {
      const int rows = a.T - t0 < FTN_TAB_SPEC_CHUNK ? a.T - t0 : FTN_TAB_SPEC_CHUNK;
      const int rows16 = (rows + 15) & ~15;                     // <= FTN_TAB_SPEC_CHUNK
      // the twiddles of the chunk's first block travel while the chunk is staged
      float2 tw[8];
      const auto load_tw = [&](float2 (&dst)[8]) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          dst[k] = a.tw[m];
          m += step;
          m = m >= T ? m - T : m;
        }
      };
      load_tw(tw);
      __syncthreads();                                          // the previous chunk (and unit) is consumed
      // staging, eight passes in flight: the loads of a batch are issued before its first LDS store
      for (int r0 = srow; r0 < rows16; r0 += 8 * sstep) {
        if (a.vec) {
          f4 xv[8], mv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int rr = r0 + u * sstep;
            const long long t = (long long)t0 + rr;
            const bool ok = cok && rr < rows;
            xv[u] = ok ? *(const f4*)(a.X + t * a.xs + n0 + scol) : f4{0.f, 0.f, 0.f, 0.f};
            mv[u] = ok && a.M != nullptr ? *(const f4*)(a.M + t * a.ms + n0 + scol) : f4{1.f, 1.f, 1.f, 1.f};
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int rr = r0 + u * sstep;
            if (rr >= rows16) break;
            f4 d = {0.f, 0.f, 0.f, 0.f};
            if (cok && rr < rows) {
              d = f4{xv[u].x - mu[0], xv[u].y - mu[1], xv[u].z - mu[2], xv[u].w - mu[3]};
              d.x = mv[u].x > 0.f ? d.x : 0.f; d.y = mv[u].y > 0.f ? d.y : 0.f;
              d.z = mv[u].z > 0.f ? d.z : 0.f; d.w = mv[u].w > 0.f ? d.w : 0.f;
            }
            *(f4*)(dl + rr * FTN_TAB_SPEC_COLS + scol) = d;
          }
        } else {
          float xv[8], mv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int rr = r0 + u * sstep;
            const long long t = (long long)t0 + rr;
            const bool ok = cok && rr < rows;
            xv[u] = ok ? a.X[t * a.xs + n0 + scol] : 0.f;
            mv[u] = ok && a.M != nullptr ? a.M[t * a.ms + n0 + scol] : 1.f;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int rr = r0 + u * sstep;
            if (rr >= rows16) break;
            float d = 0.f;
            if (cok && rr < rows) {
              d = xv[u] - mu[0];
              d = mv[u] > 0.f ? d : 0.f;
            }
            dl[rr * FTN_TAB_SPEC_COLS + scol] = d;
          }
        }
      }
      __syncthreads();
      const float* b0 = dl + h * FTN_TAB_SPEC_COLS + i;
      for (int kb = 0; kb < rows16; kb += 16) {                 // eight k-steps of two rows
        float2 twn[8];
        const bool more = kb + 16 < rows16;                     // workgroup-uniform
        if (more) load_tw(twn);                                 // the next block's twiddles behind this block's MFMAs
        float x0[8], x1[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          x0[k] = b0[(kb + 2 * k) * FTN_TAB_SPEC_COLS];
          x1[k] = b0[(kb + 2 * k) * FTN_TAB_SPEC_COLS + 32];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          re0 = __builtin_amdgcn_mfma_f32_32x32x2f32(tw[k].x, x0[k], re0, 0, 0, 0);
          im0 = __builtin_amdgcn_mfma_f32_32x32x2f32(tw[k].y, x0[k], im0, 0, 0, 0);
          if (two) {
            re1 = __builtin_amdgcn_mfma_f32_32x32x2f32(tw[k].x, x1[k], re1, 0, 0, 0);
            im1 = __builtin_amdgcn_mfma_f32_32x32x2f32(tw[k].y, x1[k], im1, 0, 0, 0);
          }
        }
        if (more) {
#pragma unroll
          for (int k = 0; k < 8; ++k) tw[k] = twn[k];
        }
      }
    }
    // ---- powers of the lane's 16 bins of both column tiles: peak (lowest bin among equals) and fp64 total
#pragma unroll
    for (int tile = 0; tile < 2; ++tile) {
      const f16acc& re = tile ? re1 : re0;
      const f16acc& im = tile ? im1 : im0;
      const long long col = n0 + tile * 32 + i;
      float best = -1.0f;
      int bf = (int)fbase + 4 * h;
      double tot = 0.0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int fr = (int)fbase + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float p = re[r] * re[r] + im[r] * im[r];
        if (fr <= a.F) {
          if (a.power != nullptr && col < a.N) a.power[(long long)(fr - 1) * a.N + col] = p;
          if (p > best) { best = p; bf = fr; }
          tot += (double)p;
        }
      }
      const float obest = __shfl_xor(best, 32);
      const int obf = __shfl_xor(bf, 32);
      const double otot = __shfl_xor(tot, 32);
      if (h == 0) {
        if (obest > best || (obest == best && obf < bf)) { best = obest; bf = obf; }
        wpart[wave][tile * 32 + i] = SpecPart{best, bf, tot + otot};
      }
    }
    __syncthreads();
    if (tid < FTN_TAB_SPEC_COLS && n0 + tid < a.N) {
      SpecPart s = wpart[0][tid];
      for (int w = 1; w < 4; ++w) {                             // waves ascend in f: strictly greater keeps the lowest bin
        const SpecPart o = wpart[w][tid];
        if (o.peak > s.peak) { s.peak = o.peak; s.f = o.f; }
        s.total += o.total;
      }
      a.part[(long long)bb * a.N + n0 + tid] = s;
    }
  }
}

__global__ __launch_bounds__(TAB_THREADS) void k_tab_spec_fin(TabSpec a) {
  for (long long c = (long long)blockIdx.x * TAB_THREADS + threadIdx.x; c < a.N; c += (long long)gridDim.x * TAB_THREADS) {
    float peak = 0.0f;
    int f = 0;
    double total = 0.0;
    if (a.nbb > 0) {
      const SpecPart s = a.part[c];
      peak = s.peak; f = s.f; total = s.total;
      for (int b = 1; b < a.nbb; ++b) {
        const SpecPart o = a.part[(long long)b * a.N + c];
        if (o.peak > peak) { peak = o.peak; f = o.f; }
        total += o.total;
      }
      if (total != total) peak = NAN;                           // a NaN never compares greater: say so
    }
    a.f_peak[c] = f; a.peak[c] = peak; a.total[c] = (float)total;
  }
}

static int spec_plan(const char* who, const FtnTableSpectrumArgs* a, TabSpec* k, FtnTableForm* form) {
  FTN_CHECK_ARG(a != nullptr, "%s: null arguments", who);
  FTN_CHECK_ARG(a->T >= 1 && a->T <= TAB_T_MAX, "%s: T=%lld is outside the supported 1..%d", who, a->T, TAB_T_MAX);
  FTN_CHECK_ARG(a->N >= 1, "%s: N=%d is not positive", who, a->N);
  FTN_CHECK_ARG(a->X != nullptr, "%s: null X", who);
  FTN_CHECK_ARG(a->x_stride >= a->N, "%s: X row stride %lld is below N=%d", who, a->x_stride, a->N);
  FTN_CHECK_ARG(a->M == nullptr || a->m_stride >= a->N, "%s: M row stride %lld is below N=%d", who, a->m_stride, a->N);
  FTN_CHECK_ARG(((((uintptr_t)a->X | (uintptr_t)a->M)) & 3) == 0, "%s: tables must be 4-byte aligned", who);
  long long reach = 0;
  FTN_CHECK_ARG(tab_mul(a->T, a->x_stride, &reach) && (a->M == nullptr || tab_mul(a->T, a->m_stride, &reach)),
                "%s: T=%lld rows at the given strides pass 64 bits", who, a->T);
  const bool vec = a->N % 4 == 0 && a->x_stride % 4 == 0 && tab_aligned16(a->X) &&
                   (a->M == nullptr || (a->m_stride % 4 == 0 && tab_aligned16(a->M)));
  k->X = a->X; k->M = a->M; k->xs = a->x_stride; k->ms = a->m_stride; k->T = (int)a->T; k->N = a->N;
  k->F = (int)(a->T / 2); k->nbb = (k->F + FTN_TAB_SPEC_BINS - 1) / FTN_TAB_SPEC_BINS; k->vec = vec;
  k->units = (long long)k->nbb * ((a->N + FTN_TAB_SPEC_COLS - 1) / FTN_TAB_SPEC_COLS);
  if (form != nullptr) {
    *form = FtnTableForm{};
    form->load_bytes = vec ? 16 : 4; form->col_tile = FTN_TAB_SPEC_COLS; form->block = FTN_TAB_SPEC_BINS;
    form->chunk = FTN_TAB_SPEC_CHUNK; form->resident = a->T <= FTN_TAB_SPEC_CHUNK; form->partials = k->nbb;
  }
  return 0;
}

extern "C" size_t ftn_table_spectrum_bytes(long long T, int N) {
  if (T < 1 || T > TAB_T_MAX || N < 1) return 0;
  const size_t nbb = (size_t)((T / 2 + FTN_TAB_SPEC_BINS - 1) / FTN_TAB_SPEC_BINS);
  return (nbb > 0 ? nbb : 1) * (size_t)N * sizeof(SpecPart);
}

extern "C" int ftn_table_spectrum_form(const FtnTableSpectrumArgs* a, FtnTableForm* form) {
  FTN_CHECK_ARG(form != nullptr, "ftn_table_spectrum_form: null form");
  TabSpec k = {};
  return spec_plan("ftn_table_spectrum_form", a, &k, form);
}

extern "C" int ftn_table_spectrum(const FtnTableSpectrumArgs* a, void* stream) {
  const char* who = "ftn_table_spectrum";
  TabSpec k = {};
  if (spec_plan(who, a, &k, nullptr) < 0) return -1;
  FTN_CHECK_ARG(a->mean != nullptr && a->twiddle != nullptr, "%s: null mean or twiddle table", who);
  FTN_CHECK_ARG((((uintptr_t)a->mean) & 3) == 0 && (((uintptr_t)a->twiddle) & 7) == 0, "%s: mean must be 4-byte and the "
                "twiddle table 8-byte aligned", who);
  FTN_CHECK_ARG(a->f_peak != nullptr && a->peak != nullptr && a->total != nullptr, "%s: null output", who);
  FTN_CHECK_ARG(((((uintptr_t)a->f_peak | (uintptr_t)a->peak | (uintptr_t)a->total | (uintptr_t)a->power_out)) & 3) == 0,
                "%s: outputs must be 4-byte aligned", who);
  FTN_CHECK_ARG(a->workspace != nullptr && (((uintptr_t)a->workspace) & 7) == 0 &&
                    a->workspace_bytes >= ftn_table_spectrum_bytes(a->T, a->N),
                "%s: the workspace holds %zu bytes, ftn_table_spectrum_bytes asks for %zu (8-byte aligned)", who,
                a->workspace_bytes, ftn_table_spectrum_bytes(a->T, a->N));
  k.mean = a->mean; k.tw = (const float2*)a->twiddle; k.part = (SpecPart*)a->workspace;
  k.power = a->power_out; k.f_peak = a->f_peak; k.peak = a->peak; k.total = a->total;
  const hipStream_t st = (hipStream_t)stream;
  if (k.units > 0) {
    hipLaunchKernelGGL(k_tab_spectrum, dim3((unsigned)(k.units < TAB_GRID_MAX ? k.units : TAB_GRID_MAX)),
                       dim3(TAB_THREADS), 0, st, k);
    FTN_CHECK_LAUNCH();
  }
  const int fb = ftn_cdiv(a->N, TAB_THREADS);
  hipLaunchKernelGGL(k_tab_spec_fin, dim3((unsigned)(fb < TAB_GRID_MAX ? fb : TAB_GRID_MAX)), dim3(TAB_THREADS), 0, st, k);
  FTN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------- features and scaler: the reference's finishing
__device__ __forceinline__ float tab_std(double css, double cnt) {
  return sqrtf((float)(css / (cnt > 1.0 ? cnt : 1.0)));         // the variance rounded once, the root once
}

__global__ __launch_bounds__(TAB_THREADS) void k_tab_features(const double* __restrict__ stats, const int* f_peak,
                                                              const float* peak, const float* total, long long T, int N,
                                                              float* __restrict__ out) {
  for (long long c = (long long)blockIdx.x * TAB_THREADS + threadIdx.x; c < N; c += (long long)gridDim.x * TAB_THREADS) {
    const float mean = (float)stats[2LL * N + c];
    float sd = tab_std(stats[3LL * N + c], stats[c]);
    float dsd = 0.0f, strength = 0.0f, period = 0.0f;
    if (T > 1) {
      dsd = tab_std(stats[9LL * N + c], stats[6LL * N + c]);
      const float tot = total[c];
      const float den = (tot >= 1e-6f || tot != tot) ? tot : 1e-6f;     // numpy's maximum keeps a NaN
      strength = peak[c] / den;
      period = tot > 1e-6f ? (float)((double)T / (double)f_peak[c]) : 0.0f;
      if (mean != mean) { dsd = NAN; strength = NAN; period = 0.0f; }
    }
    if (mean != mean) sd = NAN;
    float* o = out + c * 5;
    o[0] = mean; o[1] = sd; o[2] = dsd; o[3] = strength; o[4] = period;
  }
}

extern "C" int ftn_table_features(const double* stats_dev, const int* f_peak_dev, const float* peak_dev,
                                  const float* total_dev, long long T, int N, float* out_dev, void* stream) {
  const char* who = "ftn_table_features";
  FTN_CHECK_ARG(T >= 1 && N >= 1, "%s: T=%lld, N=%d must be positive", who, T, N);
  FTN_CHECK_ARG(stats_dev && f_peak_dev && peak_dev && total_dev && out_dev, "%s: null pointer", who);
  FTN_CHECK_ARG((((uintptr_t)stats_dev) & 7) == 0 &&
                    ((((uintptr_t)f_peak_dev | (uintptr_t)peak_dev | (uintptr_t)total_dev | (uintptr_t)out_dev)) & 3) == 0,
                "%s: stats must be 8-byte, the others 4-byte aligned", who);
  const int fb = ftn_cdiv(N, TAB_THREADS);
  hipLaunchKernelGGL(k_tab_features, dim3((unsigned)(fb < TAB_GRID_MAX ? fb : TAB_GRID_MAX)), dim3(TAB_THREADS), 0,
                     (hipStream_t)stream, stats_dev, f_peak_dev, peak_dev, total_dev, T, N, out_dev);
  FTN_CHECK_LAUNCH();
  return 0;
}

// Per series: one thread a column.  Global (one workgroup): thread i adds columns i, i + 256, .. ascending in fp64, the
// 256 partials are added ascending by thread 0; the centred sum around the global mean g follows from the column
// moments, sum_n [css_n + 2 (m_n - g)(sum_n - cnt_n m_n) + cnt_n (m_n - g)^2], the same way.
__global__ __launch_bounds__(TAB_THREADS) void k_tab_scaler(const double* __restrict__ stats, int N, int method,
                                                            int per_series, double eps, float* __restrict__ loc,
                                                            float* __restrict__ scale, float* __restrict__ pairs) {
  const float epsf = (float)eps;
  if (per_series) {
    for (long long c = (long long)blockIdx.x * TAB_THREADS + threadIdx.x; c < N; c += (long long)gridDim.x * TAB_THREADS) {
      if (method == FTN_TAB_ZSCORE) {
        const float mu = (float)stats[2LL * N + c];
        float sd = tab_std(stats[3LL * N + c], stats[c]);
        sd = sd < epsf ? 1.0f : sd;
        loc[c] = mu; scale[c] = sd; pairs[c] = mu; pairs[(long long)N + c] = sd;
      } else {
        const float mn = (float)stats[4LL * N + c], mx = (float)stats[5LL * N + c];
        const float rng = mx - mn;
        loc[c] = mn; scale[c] = rng < epsf ? 1.0f : rng; pairs[c] = mn; pairs[(long long)N + c] = mx;
      }
    }
    return;
  }
  __shared__ double red[4][TAB_THREADS];
  __shared__ double glob[4];
  const int tid = threadIdx.x;
  double cnt = 0.0, sum = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int c = tid; c < N; c += TAB_THREADS) {
    cnt += stats[c]; sum += stats[1LL * N + c];
    mn = tab_min(mn, (float)stats[4LL * N + c]); mx = tab_max(mx, (float)stats[5LL * N + c]);
  }
  red[0][tid] = cnt; red[1][tid] = sum; red[2][tid] = (double)mn; red[3][tid] = (double)mx;
  __syncthreads();
  if (tid == 0) {
    double C0 = 0.0, S0 = 0.0;
    float a = INFINITY, b = -INFINITY;
    for (int k = 0; k < TAB_THREADS; ++k) {
      C0 += red[0][k]; S0 += red[1][k]; a = tab_min(a, (float)red[2][k]); b = tab_max(b, (float)red[3][k]);
    }
    glob[0] = C0; glob[1] = (double)(float)(S0 / (C0 > 1.0 ? C0 : 1.0)); glob[2] = (double)a; glob[3] = (double)b;
  }
  __syncthreads();
  const double g = glob[1];
  double css = 0.0;
  for (int c = tid; c < N; c += TAB_THREADS) {
    const double m = stats[2LL * N + c], n = stats[c], dm = m - g;
    css += stats[3LL * N + c] + 2.0 * dm * (stats[1LL * N + c] - n * m) + n * dm * dm;
  }
  __syncthreads();
  red[0][tid] = css;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int k = 0; k < TAB_THREADS; ++k) t += red[0][k];
    red[1][0] = t;
  }
  __syncthreads();
  float l, s, p0, p1;
  if (method == FTN_TAB_ZSCORE) {
    float sd = tab_std(red[1][0], glob[0]);
    sd = (double)sd >= eps || sd != sd ? sd : 1.0f;             // the reference compares the global pair in fp64
    l = (float)g; s = sd; p0 = l; p1 = sd;
  } else {
    const float a = (float)glob[2], b = (float)glob[3];
    const float rng = (float)((double)b - (double)a);
    l = a; s = ((double)b - (double)a) >= eps || rng != rng ? rng : 1.0f; p0 = a; p1 = b;
  }
  for (int c = tid; c < N; c += TAB_THREADS) { loc[c] = l; scale[c] = s; pairs[c] = p0; pairs[(long long)N + c] = p1; }
}

extern "C" int ftn_table_scaler(const double* stats_dev, int N, int method, int per_series, double eps, float* loc_dev,
                                float* scale_dev, float* pairs_dev, void* stream) {
  const char* who = "ftn_table_scaler";
  FTN_CHECK_ARG(N >= 1, "%s: N=%d is not positive", who, N);
  FTN_CHECK_ARG(method == FTN_TAB_ZSCORE || method == FTN_TAB_MINMAX, "%s: method=%d is not FTN_TAB_ZSCORE or "
                "FTN_TAB_MINMAX", who, method);
  FTN_CHECK_ARG(eps == eps, "%s: eps is NaN", who);
  FTN_CHECK_ARG(stats_dev && loc_dev && scale_dev && pairs_dev, "%s: null pointer", who);
  FTN_CHECK_ARG((((uintptr_t)stats_dev) & 7) == 0 &&
                    ((((uintptr_t)loc_dev | (uintptr_t)scale_dev | (uintptr_t)pairs_dev)) & 3) == 0,
                "%s: stats must be 8-byte, the others 4-byte aligned", who);
  const int fb = per_series ? ftn_cdiv(N, TAB_THREADS) : 1;
  hipLaunchKernelGGL(k_tab_scaler, dim3((unsigned)(fb < TAB_GRID_MAX ? fb : TAB_GRID_MAX)), dim3(TAB_THREADS), 0,
                     (hipStream_t)stream, stats_dev, N, method, per_series != 0, eps, loc_dev, scale_dev, pairs_dev);
  FTN_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------- affine
// out[o][s][i] = ((clip ? max(x, 0) : x) - loc[c]) / scale[c], or with FTN_TAB_INVERSE x * scale[c] + loc[c] (then
// max(., 0) with FTN_TAB_CLIP), c = series ? series[s] clamped to 0 .. n_cols - 1 : s.  A unit is TAB_AFF_CHUNK
// consecutive elements e = s inner + i of one outer row; VEC: a lane takes the four elements e .. e + 3, which are one
// series (inner % 4 == 0) or four (inner == 1).
struct TabAff {
  const float* x; float* out; const float* loc; const float* scale; const long long* series;
  long long xo, xs, oo, os, units, chunks;
  int S, inner, ncols, R, inverse, clip, vec;
};

__device__ __forceinline__ float tab_affine1(const TabAff& a, float x, int s) {
  long long c = s;
  if (a.series != nullptr) {
    c = a.series[s];
    c = c < 0 ? 0 : c >= a.ncols ? a.ncols - 1 : c;
  }
  const float l = a.loc[c], sc = a.scale[c];
  if (a.inverse) {
    const float p = x * sc;                                     // two roundings: never an FMA (contract off above)
    const float r = p + l;
    return a.clip && r < 0.0f ? 0.0f : r;
  }
  const float v = a.clip && x < 0.0f ? 0.0f : x;
  return (v - l) / sc;
}

__global__ __launch_bounds__(TAB_THREADS) void k_tab_affine(TabAff a) {
  const int step = a.vec ? 4 : 1;
  for (long long unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
    const long long o = unit / a.chunks;
    const int e0 = (int)(unit - o * a.chunks) * TAB_AFF_CHUNK;
    for (int u = threadIdx.x * step; u < TAB_AFF_CHUNK; u += TAB_THREADS * step) {
      const int e = e0 + u;
      if (e >= a.R) break;                                      // R % 4 == 0 when VEC
      const int s = a.inner == 1 ? e : e / a.inner, i = e - s * a.inner;
      const float* src = a.x + o * a.xo + (long long)s * a.xs + i;
      float* dst = a.out + o * a.oo + (long long)s * a.os + i;
      if (a.vec) {
        const f4 x = *(const f4*)src;
        const int ds = a.inner == 1 ? 1 : 0;
        f4 r;
        r.x = tab_affine1(a, x.x, s); r.y = tab_affine1(a, x.y, s + ds);
        r.z = tab_affine1(a, x.z, s + 2 * ds); r.w = tab_affine1(a, x.w, s + 3 * ds);
        *(f4*)dst = r;
      } else {
        *dst = tab_affine1(a, *src, s);
      }
    }
  }
}

static int aff_plan(const char* who, const FtnTableAffineArgs* a, TabAff* k, FtnTableForm* form) {
  FTN_CHECK_ARG(a != nullptr, "%s: null arguments", who);
  FTN_CHECK_ARG(a->outer >= 1 && a->S >= 1 && a->inner >= 1, "%s: outer=%lld, S=%d, inner=%d must be positive", who,
                a->outer, a->S, a->inner);
  const long long R = (long long)a->S * a->inner;
  FTN_CHECK_ARG(R < (1LL << 31) - TAB_AFF_CHUNK, "%s: S inner = %lld is not below 2^31 - %d", who, R, TAB_AFF_CHUNK);
  FTN_CHECK_ARG((a->flags & ~(FTN_TAB_CLIP | FTN_TAB_INVERSE)) == 0, "%s: flags=%d has bits outside FTN_TAB_CLIP | "
                "FTN_TAB_INVERSE", who, a->flags);
  FTN_CHECK_ARG(a->n_cols >= 1 && (a->series != nullptr || a->S <= a->n_cols), "%s: S=%d series do not fit the %d "
                "columns of loc and scale without a series map", who, a->S, a->n_cols);
  FTN_CHECK_ARG(a->x_sstride >= a->inner && a->o_sstride >= a->inner, "%s: series strides %lld / %lld are below inner=%d",
                who, a->x_sstride, a->o_sstride, a->inner);
  FTN_CHECK_ARG(a->outer == 1 || (a->x_ostride >= 0 && a->o_ostride >= (a->S - 1) * a->o_sstride + a->inner),
                "%s: outer strides %lld / %lld: the output rows would overlap", who, a->x_ostride, a->o_ostride);
  FTN_CHECK_ARG(a->x != nullptr && a->out != nullptr && a->loc != nullptr && a->scale != nullptr, "%s: null pointer", who);
  FTN_CHECK_ARG(((((uintptr_t)a->x | (uintptr_t)a->out | (uintptr_t)a->loc | (uintptr_t)a->scale)) & 3) == 0 &&
                    (((uintptr_t)a->series) & 7) == 0, "%s: operands must be 4-byte, the series map 8-byte aligned", who);
  long long reach = 0;
  FTN_CHECK_ARG(tab_mul(a->outer, a->x_ostride > a->o_ostride ? a->x_ostride : a->o_ostride, &reach) &&
                    tab_mul(a->S, a->x_sstride > a->o_sstride ? a->x_sstride : a->o_sstride, &reach),
                "%s: the strides pass 64 bits", who);
  const bool base = tab_aligned16(a->x) && tab_aligned16(a->out) && (a->outer == 1 || (a->x_ostride % 4 == 0 &&
                                                                                        a->o_ostride % 4 == 0));
  int axis = 0;                                                 // 1: four elements of one series, 2: of four series
  if (base && a->inner % 4 == 0 && (a->S == 1 || (a->x_sstride % 4 == 0 && a->o_sstride % 4 == 0))) axis = 1;
  else if (base && a->inner == 1 && a->S % 4 == 0 && a->x_sstride == 1 && a->o_sstride == 1) axis = 2;
  k->x = a->x; k->out = a->out; k->loc = a->loc; k->scale = a->scale; k->series = a->series;
  k->xo = a->x_ostride; k->xs = a->x_sstride; k->oo = a->o_ostride; k->os = a->o_sstride;
  k->S = a->S; k->inner = a->inner; k->ncols = a->n_cols; k->R = (int)R;
  k->inverse = (a->flags & FTN_TAB_INVERSE) != 0; k->clip = (a->flags & FTN_TAB_CLIP) != 0; k->vec = axis != 0;
  k->chunks = (R + TAB_AFF_CHUNK - 1) / TAB_AFF_CHUNK;
  FTN_CHECK_ARG(tab_mul(a->outer, k->chunks, &k->units), "%s: outer=%lld rows pass 64 bits", who, a->outer);
  if (form != nullptr) {
    *form = FtnTableForm{};
    form->load_bytes = axis ? 16 : 4; form->block = TAB_AFF_CHUNK; form->lane_axis = axis;
  }
  return 0;
}

extern "C" int ftn_table_affine_form(const FtnTableAffineArgs* a, FtnTableForm* form) {
  FTN_CHECK_ARG(form != nullptr, "ftn_table_affine_form: null form");
  TabAff k = {};
  return aff_plan("ftn_table_affine_form", a, &k, form);
}

extern "C" int ftn_table_affine(const FtnTableAffineArgs* a, void* stream) {
  TabAff k = {};
  if (aff_plan("ftn_table_affine", a, &k, nullptr) < 0) return -1;
  hipLaunchKernelGGL(k_tab_affine, dim3((unsigned)(k.units < TAB_GRID_MAX ? k.units : TAB_GRID_MAX)), dim3(TAB_THREADS),
                     0, (hipStream_t)stream, k);
  FTN_CHECK_LAUNCH();
  return 0;
}
