// What the two window files share: the work-unit constants of the row copies and the host checks of the tables
// (windows.hip defines them; windows_gather.hip calls them on the FtnWindowArgs its argument record begins with).
#pragma once
#include "ftn_common.h"

#define WIN_THREADS 256
#define WIN_CHUNK 1024
#define WIN_GRID_MAX 4096
#define WIN_ONE 0x3f800000u

static inline bool win_mul(long long a, long long b, long long* out) {
  return !__builtin_mul_overflow(a, b, out) && *out <= (1LL << 61);
}

// The dimension checks every entry point shares (everything but the start rows and the item range).
int win_check_dims(const char* who, const FtnWindowArgs* a);
// starts and starts_host given, W >= 1, T >= L + H, T times every row stride within 64 bits, every host start row
// inside 0 .. T - L - H.
int win_check_starts(const char* who, const FtnWindowArgs* a);
