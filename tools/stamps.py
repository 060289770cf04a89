#!/usr/bin/env python3
"""Diagnostic: per-workgroup phase timeline of k_conv / k_mlp from s_memtime stamps
(ftn_debug_stamps).  Usage on the GPU box: python tools/stamps.py [conv|mlp] [B] [--batch N] [--json FILE]
(`conv` = stage D, `conv B` = stage B; --json writes the conv summary: per branch the earliest / median / latest
workgroup end and the per-row cost by tile).

Record of a k_conv_bf_fast workgroup (8 words): 0 start, 1 first row landed, 2 second row landed, 3 end (s_memtime);
4 taps; 5 its rows [lo, hi) of the branch's (tile, batch row) sequence, lo << 32 | hi (csrc/ftn_conv_walk.h);
6 / 7 start / end on the real-time clock (100 MHz)."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge

ap = argparse.ArgumentParser()
ap.add_argument("which", nargs="?", default="conv", choices=("conv", "mlp"))
ap.add_argument("stage", nargs="?", default="D", choices=("B", "D"))
ap.add_argument("--batch", type=int, default=int(os.environ.get("STAMP_B", "256")))
ap.add_argument("--json", default=None)
args = ap.parse_args()
which = args.which
pkg = ge.load_package()
lib = pkg.lib.load()
T = pkg.models.timesnet
dev = torch.device("cuda:0")
B, L, C, K = args.batch, 336, 64, 5
ks = [(3, 3), (5, 5), (7, 7)]
params = pkg.synth.make_inception_params(C, 4 * C, ks, 4.0, seed=0)
blk = T.TimesBlock(C, ks, 0.0, "gelu", d_ff=4 * C, bottleneck_ratio=4.0)
blk.inception.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
blk.period_selector = T.FFTPeriodSelector(K, L)
blk = blk.eval().to(dev)
x = torch.from_numpy(pkg.synth.make_input(B, L, C, seed=0)).to(dev)
with torch.inference_mode():
    for _ in range(3):
        blk(x)
    torch.cuda.synchronize()
    nwg = 2_000_000
    buf = torch.zeros(nwg * 8, dtype=torch.int64, device=dev)
    lib.ftn_debug_stamps(buf.data_ptr(), buf.numel(), (5 if args.stage == 'B' else 1) if which == 'conv' else 2)
    blk(x)
    torch.cuda.synchronize()
    lib.ftn_debug_stamps(None, 0, 0)
s = buf.cpu().numpy().reshape(-1, 8)
# both conv launches and the mlp launch write the same buffer: conv D overwrites conv B; mlp uses blockIdx.x ids
allw = s[s[:, 6] > 0] if (s[:, 6] > 0).any() else s[s[:, 0] > 0]
print("dispatched workgroups", len(allw))
live = s[:, 3] > 0
s = s[live].astype(np.float64)
t0 = s[:, 0].min()
print("live workgroups", len(s))
if which == "conv":
    xcc = np.zeros(len(s), dtype=int)
    for xid in sorted(set(xcc)):
        m = xcc == xid
        print(f"  xcc {xid}: n={m.sum():4d} start {(s[m,6].min()-s[:,6].min())/100:7.1f} us  end {(s[m,7].max()-s[:,6].min())/100:7.1f} us")
    st = (s[:, 6] - s[:, 6].min()) / 100.0
    en = (s[:, 7] - s[:, 6].min()) / 100.0
    edges = np.linspace(0, en.max(), 13)
    print("  active WGs at t:", [int(((st <= e) & (en > e)).sum()) for e in edges[:-1]])
if which == "mlp" and (s[:, 7] > 0).all():
    for name, a, b in (("chunk 1 work", 2, 7), ("chunk 1 closing barrier", 7, 4), ("chunk 2 weight refill + barrier", 4, 6)):
        dt = (s[:, b] - s[:, a])
        print(f"{name:26s} mean {dt.mean():9.0f} cyc  p50 {np.median(dt):9.0f}  p90 {np.percentile(dt, 90):9.0f}")
for name, a, b in (("stage", 0, 1), ("compute", 1, 2), ("store", 2, 3), ("total", 0, 3)):
    dt = s[:, b] - s[:, a]
    print(f"{name:8s} mean {dt.mean():10.0f} p50 {np.median(dt):10.0f} p90 {np.percentile(dt, 90):10.0f} max {dt.max():10.0f}")
if which == "conv":
    for taps in sorted(set(s[:, 4].astype(int))):
        m = s[:, 4] == taps
        print(f"taps {taps:3d}: n={m.sum():5d} stage {np.mean(s[m,1]-s[m,0]):8.0f} compute {np.mean(s[m,2]-s[m,1]):8.0f} "
              f"total {np.mean(s[m,3]-s[m,0]):8.0f}  start-span {s[m,0].min()-t0:9.0f}..{s[m,0].max()-t0:9.0f}")
if which == "conv":
    tot = s[:, 3] - s[:, 0]
    order = np.argsort(-tot)[:12]
    print("slowest workgroups: (index in live list, taps, start offset us, total cycles, first-row stage cycles)")
    for i in order:
        print(f"  {i:4d} taps {int(s[i,4]):3d} start {(s[i,6]-s[:,6].min())/100:6.1f} us  end {(s[i,7]-s[:,6].min())/100:6.1f} us  total {tot[i]:9.0f}  stage {s[i,1]-s[i,0]:9.0f}")
    for taps in sorted(set(s[:, 4].astype(int))):
        m = s[:, 4] == taps
        e = (s[m, 7] - s[:, 6].min()) / 100
        print(f"taps {taps:3d}: end time us p10 {np.percentile(e,10):6.1f} p50 {np.median(e):6.1f} p90 {np.percentile(e,90):6.1f} max {e.max():6.1f}; start max {((s[m,6]-s[:,6].min())/100).max():5.1f}")


if which == "conv":
    raw = buf.cpu().numpy().reshape(-1, 8)[(buf.cpu().numpy().reshape(-1, 8)[:, 6] > 0)]
    raw = raw[raw[:, 3] > 0]
    lo = (raw[:, 5] >> 32).astype(np.int64); hi = (raw[:, 5] & 0xffffffff).astype(np.int64)
    nrows = hi - lo
    tot = (raw[:, 3] - raw[:, 0]).astype(np.float64)
    t_first = raw[:, 6].min()
    end_us = (raw[:, 7] - t_first) / 100.0
    summary = {"batch": B, "stage": args.stage, "launch_end_us": round(float(end_us.max()), 2), "branches": {}}
    for taps in sorted(set(raw[:, 4].astype(int))):
        m = raw[:, 4] == taps
        R = int(hi[m].max())
        ntile = (R + B - 1) // B
        # rows of every workgroup by tile, then total = prologue + sum_tile rows * cost: least squares over the branch
        A = np.zeros((int(m.sum()), ntile + 1))
        A[:, ntile] = 1.0
        for i, k in enumerate(np.nonzero(m)[0]):
            for r in range(int(lo[k]), int(hi[k])):
                A[i, r // B] += 1.0
        A = np.hstack([A, ((A[:, :ntile] > 0).sum(1, keepdims=True) - 1.0)])     # tile switches of the workgroup
        sol = np.linalg.lstsq(A, tot[m], rcond=None)[0]
        e = end_us[m]
        first_tile = np.array([int(np.nonzero(A[i, :ntile])[0][0]) for i in range(A.shape[0])])
        by_first = {int(t): round(float(np.median(e[first_tile == t])), 2) for t in sorted(set(first_tile))}
        print(f"taps {taps}: rows/wg {nrows[m].min()}..{nrows[m].max()}, end us earliest {e.min():6.1f} "
              f"median {np.median(e):6.1f} latest {e.max():6.1f}")
        print(f"    cycles/row by tile (least squares) {[int(round(v)) for v in sol[:ntile]]}  fixed part {sol[ntile]:8.0f}  tile switch {sol[ntile + 1]:8.0f}")
        print(f"    median end us by the workgroup's first tile {by_first}")
        summary["branches"][str(taps)] = {
            "workgroups": int(m.sum()), "rows_per_wg": [int(nrows[m].min()), int(nrows[m].max())],
            "end_us": {"earliest": round(float(e.min()), 2), "median": round(float(np.median(e)), 2), "latest": round(float(e.max()), 2)},
            "cycles_per_row_by_tile": [int(round(v)) for v in sol[:ntile]], "fixed_cycles": int(round(sol[ntile])),
            "tile_switch_cycles": int(round(sol[ntile + 1])),
            "median_end_us_by_first_tile": by_first}
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(summary, indent=1) + "\n")
