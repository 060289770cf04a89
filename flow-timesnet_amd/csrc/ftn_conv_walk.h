// Which rows of a virtual branch's (tile, batch row) sequence a k_conv_bf_fast workgroup owns (plain arithmetic for
// host and device: tests/test_conv_walk_host.py runs it in a stand-alone program).  ftn_conv_split.h says how many
// workgroups a branch gets; this says which rows each of them walks.
//
// The sequence is tile-major: row r = tile r / B, batch row r % B.  A workgroup whose range crosses into the next
// tile pays that tile's per-lane bookkeeping and an exposed first-row DMA round trip - about 10 k cycles, one 7x7 row
// or two 3x3 rows - and with equal shares of rows the workgroups that cross are the last to finish.  So the walk
// shares out POSITIONS: a tile's B rows are followed by `sw` gap positions that stand for the switch, workgroup w of n
// gets positions [V w / n, V (w + 1) / n) of the V = tiles (B + sw), and walks the rows among them.  A workgroup that
// crosses a tile boundary therefore owns `sw` rows fewer than one that does not.  sw = 0 is the equal split of the
// rows themselves, [R w / n, R (w + 1) / n) with R = tiles B.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FTN_WALK_FN __host__ __device__ static inline
#else
#define FTN_WALK_FN static inline
#endif

// Positions [range[0], range[1]) of workgroup w of n; range[0] never stands on a gap.  Empty when range[0] >= range[1].
FTN_WALK_FN void ftn_conv_walk(long long tiles, int B, int sw, int n, int w, int range[2]) {
  const long long bs = (long long)B + sw, V = tiles * bs;
  long long lo = V * w / n;
  const long long hi = V * (w + 1) / n;
  const long long r = lo % bs;
  if (r >= B) lo += bs - r;                                     // starts in a gap: the next tile's first row
  range[0] = (int)lo;
  range[1] = (int)hi;
}

// The next stretch of rows inside one tile from position *v (not on a gap) up to position hi: batch rows
// [*b_begin, *b_end) of tile *tile; *v moves behind them, and over the gap when they reach the tile's end.
// false = the range is used up.
FTN_WALK_FN bool ftn_conv_walk_next(int B, int sw, int* v, int hi, int* tile, int* b_begin, int* b_end) {
  if (*v >= hi) return false;
  const int bs = B + sw, t = *v / bs, b0 = *v - t * bs;
  const int b1 = B - b0 < hi - *v ? B : b0 + (hi - *v);
  *tile = t; *b_begin = b0; *b_end = b1;
  *v += b1 - b0 + (b1 == B ? sw : 0);
  return true;
}

// rows of the sequence in front of position v (a gap position counts the whole tile before it)
FTN_WALK_FN long long ftn_conv_walk_row(int B, int sw, long long v) {
  const long long bs = (long long)B + sw, t = v / bs, b = v - t * bs;
  return t * B + (b < B ? b : B);
}
