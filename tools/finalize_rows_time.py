"""Times the selector's finalize (``ftn_period_finalize``) over the batch size, in its two forms: the one workgroup that
also writes amps / w for every row (FTN_FIN_ROWS=0), and the workgroup followed by ``k_row_weights`` over a grid
(FTN_FIN_ROWS=1).  ``--baseline-lib`` adds a third variant, the same entry point of another build of the library (the
parent commit's), loaded through ctypes alone.  The library reads FTN_FIN_ROWS once per process, so every variant runs
in child processes of its own, alternated round by round; a child times every (L, B) with device events around
windows of at least 0.3 s after a warm-up.  Per (L, B): the median over the rounds of each variant, the ratio of the
grid form to the baseline, and from those the threshold - the smallest measured B >= 1024 from which the grid form
wins by more than the +-4 % spread of one box at that B and at every larger one (the largest over the L's).
Fails without a GPU.

    python tools/finalize_rows_time.py --out profiles/finalize_rows_time.json [--baseline-lib path/to/parent.so]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

BS = (256, 1024, 4096, 16384, 65535)
LS = (28, 336)                       # the pipeline layout's window (where large batches occur) and the bench window
K = 5
ROUNDS = 3
WINDOW_S = 0.3
SPREAD = 0.04
FLOOR = 1024


def worker(lib_path: str) -> None:
    import torch

    import __graft_entry__ as ge

    if not torch.cuda.is_available():
        raise SystemExit("finalize_rows_time: no GPU; nothing is measured without one")
    sig = ge.load_package().lib._SIGNATURES["ftn_period_finalize"]
    lib = C.CDLL(lib_path)                                   # (torch first: the library binds to its HIP runtime)
    fn = lib.ftn_period_finalize
    fn.restype, fn.argtypes = sig
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    out = {}
    for L in LS:
        F = L // 2 + 1
        for B in BS:
            g = torch.Generator(device=dev).manual_seed(B + L)
            med = torch.rand(B, F, device=dev, generator=g) * 3.0 + torch.linspace(2.0, 0.0, F, device=dev)
            psum = med.double().sum(0)
            desc = torch.empty(256, dtype=torch.int32, device=dev)
            amps = torch.empty(B, 16, device=dev)
            wts = torch.empty(B, 16, device=dev)

            def call():
                rc = fn(psum.data_ptr(), 1, B, med.data_ptr(), B, L, K, L, 1, 0, 0, 0.0, desc.data_ptr(), amps.data_ptr(),
                        wts.data_ptr(), st, None)
                assert rc == 0, rc

            def window(n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    call()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3 / n             # us per call

            for _ in range(20):
                call()
            torch.cuda.synchronize()
            n = max(10, math.ceil(WINDOW_S * 1e6 / window(50)))
            out[f"{L}/{B}"] = {"us": window(n), "calls": n, "weights_sum": float(wts.double().sum())}
    print("RESULT " + json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "finalize_rows_time.json"))
    ap.add_argument("--baseline-lib", default=None, help="libflowtimes_hip.so of the commit to compare against")
    ap.add_argument("--baseline-name", default="parent commit")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    own = os.environ.get("FLOWTIMES_LIB") or str(ROOT / "flow-timesnet_amd" / "csrc" / "libflowtimes_hip.so")
    variants = {"workgroup": (own, "0"), "grid": (own, "1")}
    if args.baseline_lib:
        variants = {"baseline": (str(Path(args.baseline_lib).resolve()), "0"), **variants}
    seen = {v: {} for v in variants}
    sums = {v: {} for v in variants}
    for r in range(ROUNDS):
        for name, (path, fin) in variants.items():
            p = subprocess.run([sys.executable, __file__, "--worker", path], env=dict(os.environ, FTN_FIN_ROWS=fin),
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                raise SystemExit(f"worker {name} failed:\n{p.stdout[-2000:]}{p.stderr[-4000:]}")
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            for key, v in res.items():
                seen[name].setdefault(key, []).append(v["us"])
                sums[name][key] = v["weights_sum"]
            print(f"round {r} {name}: " + " ".join(f"{k}={v['us']:.1f}us" for k, v in res.items()), flush=True)
    base = "baseline" if args.baseline_lib else "workgroup"
    rows, thresholds = [], {}
    for L in LS:
        wins = {}
        for B in BS:
            key = f"{L}/{B}"
            row = {"L": L, "B": B}
            for name in variants:
                row[name + "_us"] = statistics.median(seen[name][key])
                row[name + "_us_rounds"] = seen[name][key]
            row["grid_over_" + base] = row["grid_us"] / row[base + "_us"]
            row["same_weights_sum"] = len({sums[n][key] for n in variants}) == 1
            wins[B] = row["grid_over_" + base] < 1.0 - SPREAD
            rows.append(row)
        ok = [B for B in BS if B >= FLOOR and all(wins[b] for b in BS if b >= B)]
        thresholds[str(L)] = min(ok) if ok else None
    found = [t for t in thresholds.values() if t is not None]
    threshold = max(found) if len(found) == len(LS) else None
    import torch

    doc = {"device": torch.cuda.get_device_name(0), "k_periods": K, "rounds": ROUNDS, "window_s": WINDOW_S,
           "variants": {"workgroup": "FTN_FIN_ROWS=0: one launch, the row loop inside the finalize workgroup",
                        "grid": "FTN_FIN_ROWS=1: the finalize workgroup, then k_row_weights over ceil(B / 256) workgroups",
                        **({"baseline": args.baseline_name + ": ftn_period_finalize of that build"} if args.baseline_lib else {})},
           "compared_against": base, "spread": SPREAD, "floor": FLOOR, "rows": rows, "threshold_by_L": thresholds,
           "threshold": threshold,
           "rule": "smallest measured B >= floor from which grid / baseline < 1 - spread at it and at every larger "
                   "measured B, the largest over the L's; null = the grid form wins nowhere"}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({"threshold_by_L": thresholds, "threshold": threshold}))


if __name__ == "__main__":
    main()
