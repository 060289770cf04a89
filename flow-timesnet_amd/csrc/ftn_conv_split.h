// How k_conv_bf_fast's workgroups are shared out over the virtual branches (host arithmetic only, no HIP:
// tests/test_conv_split_host.py runs it in a stand-alone program).
#pragma once
#include "../../include/flowtimes.h"

#define FTN_CONV_MAXVB (2 * FTN_MAXBR)   // virtual branches = (branch, 16-channel output tile) pairs (ConvBfArgs.wg_off)

// One workgroup per CU, each bound to one virtual branch: nwg[v] of the ncu workgroups serve branch v, every branch
// at least one, sum = ncu (nvb <= ncu).  slabs[v] = the branch's K-32 slabs per input group, nci = 16-channel input
// groups, rows_est = estimated (tile, batch row) items of the launch, or <= 0 for none.
static inline void ftn_conv_split(int ncu, int nvb, const int* slabs, int nci, int rows_est, int* nwg) {
  // cost of a branch per batch row (~3.2 k cycles + 0.28 k per K-32 slab, beside a prologue worth ~17 k whatever the
  // kernel size: fitted to tools/stamps.py after the closed-form tap masks, late round 3)
  double cost[FTN_CONV_MAXVB], tot = 0.0;
  for (int v = 0; v < nvb; ++v) { cost[v] = 3.17 + 0.281 * slabs[v] * nci; tot += cost[v]; }
  // shares in proportion to the cost: the split when there is no row estimate or the search below finds nothing
  int used = 0;
  for (int k = 0; k < nvb; ++k) { nwg[k] = (int)(ncu * cost[k] / tot); if (nwg[k] < 1) nwg[k] = 1; used += nwg[k]; }
  for (int k = 0; used < ncu; k = (k + 1) % nvb) { ++nwg[k]; ++used; }     // leftovers round-robin from the first branch
  for (int k = 0; used > ncu && k < nvb; ++k) while (nwg[k] > 1 && used > ncu) { --nwg[k]; --used; }
  if (rows_est <= 0) return;
  // Rows are whole units: a 7x7 workgroup with 11 rows ends 9 % after one with 10 (tools/stamps.py: the launch
  // ended at 79 us with the median workgroup done at 66).  With an estimate of the row count (the descriptor is on
  // the device: groups bound x tiles of a typical grid x batch rows) pick the split that minimises
  // max_k ceil(rows / nwg_k) * cost_k; a wrong estimate only costs balance, the kernel derives the ranges itself.
  double bestT = 1e300;
  for (int kk = 0; kk < nvb; ++kk) {
    for (int r = 1; r <= rows_est; ++r) {
      const double T = r * cost[kk];                             // (the prologue is the same for every branch: it drops out)
      if (T >= bestT) break;
      int need[FTN_CONV_MAXVB], sum = 0;
      bool ok = true;
      for (int k = 0; k < nvb && ok; ++k) {
        const int per = (int)(T / cost[k] + 1e-9);
        if (per < 1) { ok = false; break; }
        need[k] = (rows_est + per - 1) / per;
        sum += need[k];
      }
      if (ok && sum <= ncu) { bestT = T; used = sum; for (int k = 0; k < nvb; ++k) nwg[k] = need[k]; break; }
    }
  }
  // spare workgroups go where they shorten the longest branch next
  for (; used < ncu; ++used) {
    int arg = 0; double worst = -1.0;
    for (int k = 0; k < nvb; ++k) {
      const double t = (double)((rows_est + nwg[k] - 1) / nwg[k]) * cost[k];
      if (t > worst) { worst = t; arg = k; }
    }
    ++nwg[arg];
  }
}
