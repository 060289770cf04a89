// Training windows (include/flowtimes.h, "training windows"): the batches of a shuffled, time-shifted and noised
// epoch.  One launch writes the pieces of the items items[0 .. count - 1] - an arbitrary list of global item indices -
// into rows 0 .. count - 1 of the caller's outputs; a row whose item belongs to another part is left alone.
//
// k_epoch_keys: key64(k) = (x << 32) | y of Philox4x32-10 at counter (k, k >> 32, 0, epoch << 2 | 0); the epoch's
// order is the stable ascending argsort of the keys (the caller's, once per epoch).
//
// k_window_gather: row copies only, one indirection per row.  The launch's work is a list of up to GAT_PIECES pieces
// (one per requested output), each a run of units of WIN_CHUNK consecutive output words; a workgroup of 256 threads
// walks the units blockIdx.x, + gridDim.x, ..  Per unit:
//   1. the rows the unit touches (at most WIN_CHUNK of them) get a record in LDS: the item's series i and its start
//      row s = clamp(starts[w] + delta, 0, T - L - H), delta the item's time shift (one Philox call per row, purpose
//      1) - or s = -1 for an item outside item_lo .. item_lo + part items, of which nothing is read;
//   2. consecutive lanes move consecutive words of an output row:
//        GAT_SERIES  out[r][e] = tab[i][off + e]      x, y, mask of FTN_WIN_SERIES from the series-major tables
//                                                     (off = s + row_off: one contiguous run of XT[i]); statics and
//                                                     ids (off = 0)
//        GAT_WINDOW  out[r][j][c] = tab[s + row_off + j][c]   the marks (c < F); x, y, mask of FTN_WIN_WIDE (c < N)
//      so a shuffled batch reads as coalesced as an in-order one.  The shifted start is arbitrary: 4 bytes a lane.
// Noise (x only, noise_std > 0): element j of the item's x takes lane j & 3 of the Philox call at counter
// (k, k >> 32, j >> 2, epoch << 2 | 2): words (x, y) make the Box-Muller pair of lanes 0, 1 and (z, w) that of lanes
// 2, 3, in fp64; x_out = fp32(double(x) + noise_std z), the product and the sum each rounded once (not contracted).
// Every other value is moved as a 32-bit word.  No device value can address outside a table: i < N and w < W follow
// from the item range, and s is clamped.
#include "ftn_win.h"
#include "ftn_philox.h"

#define GAT_PIECES 7
#define GAT_ROWS WIN_CHUNK                                      // rows a unit can touch (JC = 1: a word a row)

enum { GAT_WINDOW = 0, GAT_SERIES = 1 };
enum { GAT_ORDER = 0, GAT_SHIFT = 1, GAT_NOISE = 2 };           // the purpose bits of the counter's last word

struct GatPiece {
  const unsigned* tab;  unsigned* out;                          // tab null: a piece of ones
  long long stride, end;                                        // words between table rows; one past its last unit
  int row_off, JC, Cw, kind, timed, noise;                      // JC words an item, Cw words a table row of it
};
struct GatLaunch {
  GatPiece p[GAT_PIECES];
  const int* starts;  const long long* items;
  long long item_lo, part_items, count, total;
  unsigned long long seed;
  double sd;
  unsigned epoch;
  int ts, np, N, smax, series;
};

__device__ __forceinline__ float gat_noise(const GatLaunch& a, unsigned long long k, unsigned j, unsigned word) {
  const PhiloxWords wd = ftn_philox((unsigned)k, (unsigned)(k >> 32), j >> 2, a.epoch << 2 | GAT_NOISE,
                                    (unsigned)a.seed, (unsigned)(a.seed >> 32));
  const unsigned wa = (j & 2) ? wd.z : wd.x, wb = (j & 2) ? wd.w : wd.y;
  const double u1 = ((double)wa + 0.5) * 2.3283064365386963e-10;  // 2^-32
  const double u2 = ((double)wb + 0.5) * 2.3283064365386963e-10;
  const double r = sqrt(-2.0 * log(u1)), t = 6.283185307179586 * u2;
  const double z = r * ((j & 1) ? sin(t) : cos(t));
  return (float)__dadd_rn((double)__uint_as_float(word), __dmul_rn(a.sd, z));
}

__global__ __launch_bounds__(WIN_THREADS) void k_window_gather(GatLaunch a) {
  __shared__ int rec_s[GAT_ROWS];
  __shared__ int rec_i[GAT_ROWS];
  for (long long unit = blockIdx.x; unit < a.total; unit += gridDim.x) {
    int pi = 0;
    while (pi < a.np - 1 && unit >= a.p[pi].end) ++pi;
    const GatPiece& p = a.p[pi];
    const long long local = unit - (pi > 0 ? a.p[pi - 1].end : 0);
    const unsigned JC = (unsigned)p.JC;                         // words of an item: < 2^31 (host check)
    const long long g0 = local * WIN_CHUNK, r0 = g0 / JC;       // the unit's first word: row r0, word e0 of it
    const unsigned e0 = (unsigned)(g0 - r0 * JC);
    long long rl = (g0 + WIN_CHUNK - 1) / JC;                   // its last row
    if (rl >= a.count) rl = a.count - 1;
    const unsigned nrows = (unsigned)(rl - r0) + 1;             // <= GAT_ROWS
    for (unsigned rr = threadIdx.x; rr < nrows; rr += WIN_THREADS) {
      const long long k = a.items[r0 + rr];
      int s = -1, i = 0;
      if (k >= a.item_lo && k - a.item_lo < a.part_items) {
        const long long kl = k - a.item_lo;
        long long w = kl;                                       // wide: item = window
        if (a.series) {
          w = kl / a.N;
          i = (int)(kl - w * a.N);
        }
        long long sv = a.starts[w];
        if (a.ts > 0) {
          const PhiloxWords wd = ftn_philox((unsigned)k, (unsigned)((unsigned long long)k >> 32), 0u,
                                            a.epoch << 2 | GAT_SHIFT, (unsigned)a.seed, (unsigned)(a.seed >> 32));
          sv += (long long)(((unsigned long long)wd.x * (2ull * (unsigned)a.ts + 1ull)) >> 32) - a.ts;
        }
        s = sv < 0 ? 0 : sv > a.smax ? a.smax : (int)sv;
      }
      rec_s[rr] = s;
      rec_i[rr] = i;
    }
    __syncthreads();
    for (unsigned u = threadIdx.x; u < WIN_CHUNK; u += WIN_THREADS) {
      const unsigned v = e0 + u, dr = v / JC, e = v - dr * JC;  // e0 + u < 2^31 + WIN_CHUNK
      if (dr >= nrows) break;
      const int s = rec_s[dr];
      if (s < 0) continue;                                      // another part's row
      unsigned* dst = p.out + (r0 + dr) * JC + e;
      if (p.tab == nullptr) {
        *dst = WIN_ONE;
        continue;
      }
      long long src;
      if (p.kind == GAT_SERIES) {
        src = (long long)rec_i[dr] * p.stride + (p.timed ? s + p.row_off : 0) + e;
      } else {
        const unsigned j = e / (unsigned)p.Cw, c = e - j * (unsigned)p.Cw;
        src = ((long long)s + p.row_off + j) * p.stride + c;
      }
      const unsigned word = p.tab[src];
      *dst = p.noise ? __float_as_uint(gat_noise(a, (unsigned long long)a.items[r0 + dr], e, word)) : word;
    }
    __syncthreads();                                            // the next unit rewrites the records
  }
}

__global__ __launch_bounds__(WIN_THREADS) void k_epoch_keys(long long n, unsigned long long seed, unsigned epoch,
                                                            long long* keys) {
  for (long long k = (long long)blockIdx.x * WIN_THREADS + threadIdx.x; k < n; k += (long long)gridDim.x * WIN_THREADS) {
    const PhiloxWords wd = ftn_philox((unsigned)k, (unsigned)((unsigned long long)k >> 32), 0u, epoch << 2 | GAT_ORDER,
                                      (unsigned)seed, (unsigned)(seed >> 32));
    keys[k] = (long long)((unsigned long long)wd.x << 32 | wd.y);
  }
}

extern "C" int ftn_epoch_keys(long long n, unsigned long long seed, unsigned epoch, long long* keys_dev, void* stream) {
  const char* who = "ftn_epoch_keys";
  FTN_CHECK_ARG(n >= 1 && n <= (1LL << 61), "%s: n=%lld", who, n);
  FTN_CHECK_ARG(epoch < (1u << 30), "%s: epoch=%u is not below 2^30", who, epoch);
  FTN_CHECK_ARG(keys_dev != nullptr && ((uintptr_t)keys_dev & 7) == 0, "%s: keys must be given and 8-byte aligned", who);
  const long long groups = (n + WIN_THREADS - 1) / WIN_THREADS;
  const dim3 grid((unsigned)(groups < WIN_GRID_MAX ? groups : WIN_GRID_MAX));
  hipLaunchKernelGGL(k_epoch_keys, grid, dim3(WIN_THREADS), 0, (hipStream_t)stream, n, seed, epoch, keys_dev);
  FTN_CHECK_LAUNCH();
  return 0;
}

extern "C" int ftn_window_gather(const FtnWindowGatherArgs* g, void* stream) {
  const char* who = "ftn_window_gather";
  FTN_CHECK_ARG(g != nullptr, "%s: null arguments", who);
  const FtnWindowArgs* a = &g->w;
  if (win_check_dims(who, a) < 0 || win_check_starts(who, a) < 0) return -1;
  const bool series = a->layout == FTN_WIN_SERIES;
  FTN_CHECK_ARG(g->items != nullptr && ((uintptr_t)g->items & 7) == 0, "%s: items must be given and 8-byte aligned", who);
  FTN_CHECK_ARG(a->count >= 1, "%s: count=%lld is not positive", who, a->count);
  FTN_CHECK_ARG(a->item0 >= 0 && a->item0 <= (1LL << 61), "%s: item_lo=%lld", who, a->item0);
  FTN_CHECK_ARG(g->ts >= 0, "%s: ts=%d is negative", who, g->ts);
  FTN_CHECK_ARG(g->noise_std >= 0.0 && g->noise_std <= 1.79769313486231570e308, "%s: noise_std=%g is not a finite "
                "non-negative number", who, g->noise_std);
  FTN_CHECK_ARG(g->epoch < (1u << 30), "%s: epoch=%u is not below 2^30", who, g->epoch);
  if (series) {
    long long reach = 0;
    FTN_CHECK_ARG(g->XT != nullptr && ((uintptr_t)g->XT & 3) == 0 && g->xt_stride >= a->T, "%s: FTN_WIN_SERIES takes XT "
                  "[N][xt_stride], 4-byte aligned, xt_stride=%lld >= T=%lld", who, g->xt_stride, a->T);
    FTN_CHECK_ARG(g->MT == nullptr || (((uintptr_t)g->MT & 3) == 0 && g->mt_stride >= a->T), "%s: MT needs 4-byte "
                  "alignment and mt_stride=%lld >= T=%lld", who, g->mt_stride, a->T);
    FTN_CHECK_ARG(win_mul(a->N, g->xt_stride, &reach) && (g->MT == nullptr || win_mul(a->N, g->mt_stride, &reach)),
                  "%s: N=%d rows at the given strides pass 64 bits", who, a->N);
  }
  const long long span = (long long)a->L + a->H;
  GatLaunch k = {};
  k.starts = a->starts; k.items = g->items; k.item_lo = a->item0; k.count = a->count;
  k.part_items = series ? (long long)a->W * a->N : a->W;        // W, N < 2^31
  k.seed = g->seed; k.sd = g->noise_std; k.epoch = g->epoch; k.ts = g->ts; k.N = a->N; k.series = series;
  k.smax = (int)(a->T - span < 0x7fffffffLL ? a->T - span : 0x7fffffffLL);
  long long total = 0;
  int np = 0;
  const bool noise = g->noise_std > 0.0;
  const auto add = [&](const void* tab, long long stride, void* out, int row_off, int J, int Cw, int kind, int timed,
                       bool noisy) -> bool {
    if (out == nullptr) return true;
    long long words = 0;
    if (!win_mul(a->count, (long long)J * Cw, &words)) return false;
    total += (words + WIN_CHUNK - 1) / WIN_CHUNK;               // <= 2^61 / 1024 a piece
    GatPiece& p = k.p[np++];
    p.tab = (const unsigned*)tab; p.out = (unsigned*)out; p.stride = stride; p.end = total;
    p.row_off = row_off; p.JC = J * Cw; p.Cw = Cw; p.kind = kind; p.timed = timed; p.noise = noisy && tab != nullptr;
    return true;
  };
  bool ok = true;
  if (series) {
    ok = ok && add(g->XT, g->xt_stride, a->x, 0, a->L, 1, GAT_SERIES, 1, noise);
    ok = ok && add(g->XT, g->xt_stride, a->y, a->L, a->H, 1, GAT_SERIES, 1, false);
    ok = ok && add(g->MT, g->mt_stride, a->mask, a->L, a->H, 1, GAT_SERIES, 1, false);
  } else {
    ok = ok && add(a->X, a->x_stride, a->x, 0, a->L, a->N, GAT_WINDOW, 1, noise);
    ok = ok && add(a->X, a->x_stride, a->y, a->L, a->H, a->N, GAT_WINDOW, 1, false);
    ok = ok && add(a->M, a->m_stride, a->mask, a->L, a->H, a->N, GAT_WINDOW, 1, false);
  }
  ok = ok && add(a->marks, a->marks_stride, a->x_mark, 0, a->L, a->F, GAT_WINDOW, 1, false);
  ok = ok && add(a->marks, a->marks_stride, a->y_mark, a->L, a->H, a->F, GAT_WINDOW, 1, false);
  ok = ok && add(a->statics, a->Fs, a->static_out, 0, 1, a->Fs, GAT_SERIES, 0, false);
  ok = ok && add(a->ids, 2, a->id_out, 0, 1, 2, GAT_SERIES, 0, false);
  FTN_CHECK_ARG(ok, "%s: count=%lld items pass 64 bits", who, a->count);
  k.np = np; k.total = total;
  const dim3 grid((unsigned)(total < WIN_GRID_MAX ? total : WIN_GRID_MAX));
  hipLaunchKernelGGL(k_window_gather, grid, dim3(WIN_THREADS), 0, (hipStream_t)stream, k);
  FTN_CHECK_LAUNCH();
  return 0;
}
