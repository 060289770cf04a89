// Sliding windows of a wide table [T][N], formed on the device (include/flowtimes.h, "device windows"): one launch
// writes the pieces of items item0 .. item0 + count - 1 into rows 0 .. count - 1 of the caller's outputs.  Every value
// is moved as a 32-bit word (ids as two), so NaN payloads and -0 survive; nothing is computed.
//
// k_window_batch: the launch's work is a list of up to WIN_PIECES pieces (one per requested output), each a run of
// work units; a workgroup of 256 threads walks the units blockIdx.x, + gridDim.x, .. and finds each unit's piece.
//   WIN_TRANSPOSE    x, y and mask of FTN_WIN_SERIES: out[r][t] = tab[s_w + row_off + t][i] with k = item0 + r,
//                    w = k / N, i = k % N.  A unit is a tile (window w, WIN_TS series from a multiple of WIN_TS,
//                    WIN_TT time steps from a multiple of WIN_TT), clipped to the series the batch takes of that
//                    window (the first and last window of a batch are partial) and to the piece's J time steps.
//                    Read along the series (the contiguous direction of the table), a wave a time step - VEC: a lane
//                    a quad of series - into LDS [WIN_TT][WIN_TS + 1]; written along time, consecutive lanes on
//                    consecutive time steps of a series and on to the next series - a tile that spans all J steps is
//                    one contiguous run of the output.  The odd row stride puts element (t, i) on bank (t + i) mod 32:
//                    the stores of a 32-lane half walk i (VEC: 16 quads of two steps, banks t + 4 q + c) and the loads
//                    walk t (VEC: words t .. t + 3 of quads 4 apart), both without a conflict inside a series row;
//                    where a half crosses from one series to the next at J mod 32 != 0 a few lanes meet two-way.
//   WIN_ROWS_WINDOW  out[r][j][c] = tab[s_w + row_off + j][c]: the marks of both layouts (c < F) and x, y, mask of
//                    FTN_WIN_WIDE (c < N, w = item0 + r).  Row copies: a unit is WIN_CHUNK consecutive words of the
//                    output, a thread 4 of them (VEC: one 16-byte load and store).
//   WIN_ROWS_SERIES  out[r][c] = tab[i][c]: statics (c < Fs) and ids (two words) of FTN_WIN_SERIES.
// A piece without a table (mask when M is null) stores 1.0f and reads nothing.  The start rows are read from the
// device and clamped to 0 .. T - L - H, so a device copy that disagrees with the validated host copy cannot address
// anything outside the tables; rows r >= count and series outside the batch's share of a window are never touched.
#include "ftn_win.h"

#define WIN_LDS_STRIDE (FTN_WIN_TILE_SERIES + 1)
#define WIN_PIECES 7

typedef unsigned u4 __attribute__((ext_vector_type(4)));

enum { WIN_TRANSPOSE = 0, WIN_ROWS_WINDOW = 1, WIN_ROWS_SERIES = 2 };

struct WinPiece {
  const unsigned* tab;  unsigned* out;                          // tab null: a piece of ones
  long long stride, end;                                        // words between table rows; one past its last unit
  int row_off, J, Cw, kind, vec;                                // rows s_w + row_off + (0 .. J - 1), Cw words a row
};
struct WinLaunch {
  WinPiece p[WIN_PIECES];
  const int* starts;
  long long item0, count, total, w0, w1;                        // the batch's first and last window (series layout)
  int np, N, smax, series, lo0, hi1;                            // its series lo0 .. of window w0, .. hi1 - 1 of w1
};

__device__ __forceinline__ long long win_start(const WinLaunch& a, long long w) {
  const int s = a.starts[w];
  return s < 0 ? 0 : s > a.smax ? a.smax : s;
}

__device__ __forceinline__ void win_tile(const WinLaunch& a, const WinPiece& p, long long local, unsigned* lds) {
  const int tid = threadIdx.x;
  const int ntt = (p.J + FTN_WIN_TILE_STEPS - 1) / FTN_WIN_TILE_STEPS;
  const long long per = ((long long)a.N + FTN_WIN_TILE_SERIES - 1) / FTN_WIN_TILE_SERIES * ntt;     // tiles a window
  const long long wl = local / per, w = a.w0 + wl;
  const int rem = (int)(local - wl * per);                      // < 2^31: (L + H) N is (host check)
  const int i0 = rem / ntt * FTN_WIN_TILE_SERIES, t0 = rem % ntt * FTN_WIN_TILE_STEPS;
  const int lo = w == a.w0 ? a.lo0 : 0, hi = w == a.w1 ? a.hi1 : a.N;
  const int ia = (lo > i0 ? lo : i0) - i0;                      // the tile's series ia .. ib - 1 belong to the batch
  const int ib = (hi < i0 + FTN_WIN_TILE_SERIES ? hi : i0 + FTN_WIN_TILE_SERIES) - i0;
  if (ia >= ib) return;                                         // workgroup-uniform: before any barrier
  const int tt = p.J - t0 < FTN_WIN_TILE_STEPS ? p.J - t0 : FTN_WIN_TILE_STEPS;
  if (p.tab != nullptr) {
    const unsigned* src = p.tab + (win_start(a, w) + p.row_off + t0) * p.stride + i0;
    if (p.vec) {                                                // N % 4 == 0: a quad that starts below N ends below N
      const int q = (tid & 15) * 4;
      if (q + 4 > ia && q < ib) {
        for (int t = tid >> 4; t < tt; t += WIN_THREADS / 16) {
          const u4 v = *(const u4*)(src + t * p.stride + q);
          unsigned* d = lds + t * WIN_LDS_STRIDE + q;
          d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
      }
    } else {
      const int i = tid & 63;
      if (i >= ia && i < ib) {
        for (int t = tid >> 6; t < tt; t += WIN_THREADS / 64) lds[t * WIN_LDS_STRIDE + i] = src[t * p.stride + i];
      }
    }
    __syncthreads();
  }
  const long long rbase = w * a.N + i0 - a.item0;               // output row of the tile's series i: rbase + i >= 0
  const int ns = ib - ia;
  if (p.vec) {                                                  // J % 4 == 0: tt % 4 == 0
    const int tq = tt >> 2;
    for (int j = tid; j < ns * tq; j += WIN_THREADS) {
      const int i = ia + j / tq, l = j % tq * 4;
      u4 v = u4{WIN_ONE, WIN_ONE, WIN_ONE, WIN_ONE};
      if (p.tab != nullptr) {
        const unsigned* c = lds + l * WIN_LDS_STRIDE + i;
        v = u4{c[0], c[WIN_LDS_STRIDE], c[2 * WIN_LDS_STRIDE], c[3 * WIN_LDS_STRIDE]};
      }
      *(u4*)(p.out + (rbase + i) * p.J + t0 + l) = v;
    }
  } else {
    for (int j = tid; j < ns * tt; j += WIN_THREADS) {
      const int i = ia + j / tt, l = j % tt;
      p.out[(rbase + i) * p.J + t0 + l] = p.tab != nullptr ? lds[l * WIN_LDS_STRIDE + i] : WIN_ONE;
    }
  }
  if (p.tab != nullptr) __syncthreads();                        // the next tile writes the LDS image
}

__device__ __forceinline__ void win_rows(const WinLaunch& a, const WinPiece& p, long long local) {
  const unsigned JC = (unsigned)p.J * (unsigned)p.Cw, N = (unsigned)a.N;        // words of an item: < 2^31 (host check)
  const long long g0 = local * WIN_CHUNK, r0 = g0 / JC;         // the unit's first word: item row r0, word e0 of it
  const unsigned e0 = (unsigned)(g0 - r0 * JC);
  const long long k0 = a.item0 + r0;
  long long wb = k0;                                            // wide: item = window
  unsigned ibase = 0;
  if (a.series) {
    wb = k0 / N;
    ibase = (unsigned)(k0 - wb * N);
  }
  const unsigned step = p.vec ? 4 : 1;
  for (unsigned u = threadIdx.x * step; u < WIN_CHUNK; u += WIN_THREADS * step) {
    const unsigned v = e0 + u, dr = v / JC, e = v - dr * JC;    // e0 + u < 2^31 + WIN_CHUNK
    const long long r = r0 + dr;
    if (r >= a.count) break;
    const unsigned j = e / (unsigned)p.Cw, c = e - j * (unsigned)p.Cw;
    long long w = wb + dr;
    unsigned i = 0;
    if (a.series) {
      const unsigned ii = ibase + dr, dw = ii / N;              // ibase < N < 2^31 and dr <= WIN_CHUNK
      w = wb + dw;
      i = ii - dw * N;
    }
    unsigned* dst = p.out + r * JC + e;
    if (p.tab == nullptr) {
      if (p.vec) *(u4*)dst = u4{WIN_ONE, WIN_ONE, WIN_ONE, WIN_ONE};
      else *dst = WIN_ONE;
      continue;
    }
    const long long row = p.kind == WIN_ROWS_SERIES ? (long long)i : win_start(a, w) + p.row_off + j;
    const unsigned* src = p.tab + row * p.stride + c;
    if (p.vec) *(u4*)dst = *(const u4*)src;                     // JC, Cw, stride % 4 == 0: e, c % 4 == 0
    else *dst = *src;
  }
}

__global__ __launch_bounds__(WIN_THREADS) void k_window_batch(WinLaunch a) {
  __shared__ unsigned lds[FTN_WIN_TILE_STEPS * WIN_LDS_STRIDE];
  for (long long unit = blockIdx.x; unit < a.total; unit += gridDim.x) {
    int pi = 0;
    while (pi < a.np - 1 && unit >= a.p[pi].end) ++pi;
    const WinPiece& p = a.p[pi];
    const long long local = unit - (pi > 0 ? a.p[pi - 1].end : 0);
    if (p.kind == WIN_TRANSPOSE) win_tile(a, p, local, lds);
    else win_rows(a, p, local);
  }
}

// ---- host: one plan for ftn_window_batch_form and the launch ----
// The dimension checks every entry point shares (everything but the start rows and the item range).
int win_check_dims(const char* who, const FtnWindowArgs* a) {
  FTN_CHECK_ARG(a != nullptr, "%s: null arguments", who);
  FTN_CHECK_ARG(a->layout == FTN_WIN_SERIES || a->layout == FTN_WIN_WIDE, "%s: layout=%d is not FTN_WIN_SERIES or "
                "FTN_WIN_WIDE", who, a->layout);
  FTN_CHECK_ARG(a->N >= 1, "%s: N=%d is not positive", who, a->N);
  FTN_CHECK_ARG(a->L >= 1 && a->H >= 1, "%s: L=%d, H=%d must be positive", who, a->L, a->H);
  FTN_CHECK_ARG(a->F >= 0 && a->Fs >= 0, "%s: F=%d, Fs=%d must not be negative", who, a->F, a->Fs);
  int widest = a->N > a->F ? a->N : a->F;
  if (a->Fs > widest) widest = a->Fs;
  const long long span = (long long)a->L + a->H;
  FTN_CHECK_ARG(span * widest < (1LL << 31), "%s: (L + H) max(N, F, Fs) = %lld is not below 2^31", who, span * widest);
  FTN_CHECK_ARG(a->X != nullptr, "%s: null X", who);
  FTN_CHECK_ARG(a->x_stride >= a->N, "%s: X row stride %lld is below N=%d", who, a->x_stride, a->N);
  FTN_CHECK_ARG(a->M == nullptr || a->m_stride >= a->N, "%s: M row stride %lld is below N=%d", who, a->m_stride, a->N);
  FTN_CHECK_ARG(a->marks == nullptr || (a->F >= 1 && a->marks_stride >= a->F), "%s: marks need F >= 1 and a row "
                "stride >= F, got F=%d, stride %lld", who, a->F, a->marks_stride);
  FTN_CHECK_ARG(a->statics == nullptr || a->Fs >= 1, "%s: statics need Fs >= 1", who);
  FTN_CHECK_ARG((a->x_mark == nullptr && a->y_mark == nullptr) || a->marks != nullptr, "%s: mark outputs without "
                "marks", who);
  FTN_CHECK_ARG(a->static_out == nullptr || a->statics != nullptr, "%s: static output without statics", who);
  FTN_CHECK_ARG(a->id_out == nullptr || a->ids != nullptr, "%s: id output without ids", who);
  FTN_CHECK_ARG(a->layout == FTN_WIN_SERIES || (a->static_out == nullptr && a->id_out == nullptr), "%s: "
                "FTN_WIN_WIDE copies no statics and no ids", who);
  const uintptr_t all = (uintptr_t)a->X | (uintptr_t)a->M | (uintptr_t)a->marks | (uintptr_t)a->statics |
                        (uintptr_t)a->x | (uintptr_t)a->y | (uintptr_t)a->mask | (uintptr_t)a->x_mark |
                        (uintptr_t)a->y_mark | (uintptr_t)a->static_out | (uintptr_t)a->starts |
                        (uintptr_t)a->starts_host;
  FTN_CHECK_ARG((all & 3) == 0, "%s: operands must be 4-byte aligned", who);
  FTN_CHECK_ARG((((uintptr_t)a->ids | (uintptr_t)a->id_out) & 7) == 0, "%s: ids must be 8-byte aligned", who);
  FTN_CHECK_ARG(a->x || a->y || a->mask || a->x_mark || a->y_mark || a->static_out || a->id_out, "%s: no output "
                "requested", who);
  return 0;
}

int win_check_starts(const char* who, const FtnWindowArgs* a) {
  FTN_CHECK_ARG(a->starts != nullptr && a->starts_host != nullptr, "%s: null starts or starts_host", who);
  FTN_CHECK_ARG(a->W >= 1, "%s: W=%d windows", who, a->W);
  const long long span = (long long)a->L + a->H;
  FTN_CHECK_ARG(a->T >= span, "%s: T=%lld rows hold no window of L + H = %lld", who, a->T, span);
  long long reach = 0;                                          // every product in 64 bits
  FTN_CHECK_ARG(win_mul(a->T, a->x_stride, &reach) && (a->M == nullptr || win_mul(a->T, a->m_stride, &reach)) &&
                    (a->marks == nullptr || win_mul(a->T, a->marks_stride, &reach)),
                "%s: T=%lld rows at the given strides pass 64 bits", who, a->T);
  for (int w = 0; w < a->W; ++w)
    FTN_CHECK_ARG(a->starts_host[w] >= 0 && a->starts_host[w] + span <= a->T, "%s: window %d starts at row %d, outside "
                  "0..T - L - H = %lld", who, w, a->starts_host[w], a->T - span);
  return 0;
}

static bool win_vec(const void* tab, long long stride, const void* out, int cw, int run) {
  return cw % 4 == 0 && run % 4 == 0 && (tab == nullptr || stride % 4 == 0) &&
         ((((uintptr_t)tab | (uintptr_t)out) & 15) == 0);
}

// The pieces of a call, in the order x, y, mask, x_mark, y_mark, static, id, and its form word.  Unit counts are
// filled only when `count` is valid (the launch); the form needs none.
static int win_plan(const FtnWindowArgs* a, WinLaunch* k) {
  const bool series = a->layout == FTN_WIN_SERIES;
  int form = 0, np = 0;
  bool tiles = false;
  const auto add = [&](int bit, const void* tab, long long stride, void* out, int row_off, int J, int Cw, int kind) {
    if (out == nullptr) return;
    // a transposed piece loads quads along the series and stores quads along time; a row copy moves quads of a row
    const bool vec = bit >= 0 && (kind == WIN_TRANSPOSE ? win_vec(tab, stride, out, a->N, J)
                                                        : win_vec(tab, stride, out, Cw, 4));
    if (vec) form |= 1 << bit;
    tiles = tiles || kind == WIN_TRANSPOSE;
    WinPiece& p = k->p[np++];
    p.tab = (const unsigned*)tab; p.out = (unsigned*)out; p.stride = stride; p.end = 0;
    p.row_off = row_off; p.J = J; p.Cw = Cw; p.kind = kind; p.vec = vec;
  };
  const int vkind = series ? WIN_TRANSPOSE : WIN_ROWS_WINDOW, vcw = series ? 1 : a->N;
  add(0, a->X, a->x_stride, a->x, 0, a->L, vcw, vkind);
  add(1, a->X, a->x_stride, a->y, a->L, a->H, vcw, vkind);
  add(2, a->M, a->m_stride, a->mask, a->L, a->H, vcw, vkind);
  add(3, a->marks, a->marks_stride, a->x_mark, 0, a->L, a->F, WIN_ROWS_WINDOW);
  add(4, a->marks, a->marks_stride, a->y_mark, a->L, a->H, a->F, WIN_ROWS_WINDOW);
  add(-1, a->statics, a->Fs, a->static_out, 0, 1, a->Fs, WIN_ROWS_SERIES);
  add(-1, a->ids, 2, a->id_out, 0, 1, 2, WIN_ROWS_SERIES);
  k->np = np;
  if (tiles) form |= FTN_WIN_TILE_SERIES << 8 | FTN_WIN_TILE_STEPS << 16;
  return form;
}

extern "C" int ftn_window_batch_form(const FtnWindowArgs* a) {
  if (win_check_dims("ftn_window_batch_form", a) < 0) return -1;
  WinLaunch k = {};
  return win_plan(a, &k);
}

extern "C" int ftn_window_batch(const FtnWindowArgs* a, void* stream) {
  const char* who = "ftn_window_batch";
  if (win_check_dims(who, a) < 0) return -1;
  if (win_check_starts(who, a) < 0) return -1;
  const long long span = (long long)a->L + a->H;
  long long items = 0, words = 0;                               // every product in 64 bits
  const bool series = a->layout == FTN_WIN_SERIES;
  items = series ? (long long)a->W * a->N : a->W;               // W, N < 2^31
  FTN_CHECK_ARG(a->count >= 1, "%s: count=%lld is not positive", who, a->count);
  FTN_CHECK_ARG(a->item0 >= 0 && a->item0 <= items && a->count <= items - a->item0, "%s: items %lld.. (%lld of them) "
                "are outside 0..%lld", who, a->item0, a->count, items);
  WinLaunch k = {};
  win_plan(a, &k);
  k.starts = a->starts; k.item0 = a->item0; k.count = a->count; k.N = a->N; k.series = series;
  k.smax = (int)(a->T - span < 0x7fffffffLL ? a->T - span : 0x7fffffffLL);
  if (series) {
    k.w0 = a->item0 / a->N; k.w1 = (a->item0 + a->count - 1) / a->N;
    k.lo0 = (int)(a->item0 - k.w0 * a->N); k.hi1 = (int)(a->item0 + a->count - k.w1 * a->N);
  }
  long long total = 0;
  for (int i = 0; i < k.np; ++i) {
    WinPiece& p = k.p[i];
    long long units = 0;
    if (p.kind == WIN_TRANSPOSE) {
      const long long per = ((long long)a->N + FTN_WIN_TILE_SERIES - 1) / FTN_WIN_TILE_SERIES *
                            ((p.J + FTN_WIN_TILE_STEPS - 1) / FTN_WIN_TILE_STEPS);
      FTN_CHECK_ARG(win_mul(k.w1 - k.w0 + 1, per, &units) && win_mul(a->count, p.J, &words), "%s: count=%lld items "
                    "of %d steps pass 64 bits", who, a->count, p.J);
    } else {
      FTN_CHECK_ARG(win_mul(a->count, (long long)p.J * p.Cw, &words), "%s: count=%lld items of %lld words pass 64 bits",
                    who, a->count, (long long)p.J * p.Cw);
      units = (words + WIN_CHUNK - 1) / WIN_CHUNK;
    }
    FTN_CHECK_ARG(!__builtin_add_overflow(total, units, &total) && total <= (1LL << 61), "%s: the work of count=%lld "
                  "items passes 64 bits", who, a->count);
    p.end = total;
  }
  k.total = total;
  const dim3 grid((unsigned)(total < WIN_GRID_MAX ? total : WIN_GRID_MAX));
  hipLaunchKernelGGL(k_window_batch, grid, dim3(WIN_THREADS), 0, (hipStream_t)stream, k);
  FTN_CHECK_LAUNCH();
  return 0;
}
