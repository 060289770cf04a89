"""Times ``ftn_path_summary`` (``score.path_summary(..., backend="hip")``) at samples [P, 8, 96, 512] for P = 16, 64,
256, 1024 with window 1 and window 8, beside the torch backend of the same call on the same tensors: one process,
the two alternated round by round, device events around windows of at least 0.3 s after a warm-up of every shape.
Per row: the kernel's time per call, the bytes the algorithm needs, 4 (P B H N + B H N + outputs), the share of the
HBM peak those bytes give, and the torch time.  Fails without a GPU.

    python tools/path_time.py --out profiles/path_time.json
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

BHN = (8, 96, 512)
PATHS = (16, 64, 256, 1024)
WINDOWS = (1, 8)
LEVELS = [0.05, 0.5, 0.95]
HBM_PEAK = 8.0e12            # bytes / s, the datasheet figure
WINDOW_S = 0.3
ROUNDS = 3


def window(fn, n):
    """Microseconds per call over n back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def alternated(fns):
    """``{name: (median, min)}`` microseconds per call: a warm-up, a count per variant that fills WINDOW_S, then ROUNDS
    rounds that take every variant in turn."""
    counts = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        counts[name] = max(1, math.ceil(WINDOW_S * 1e6 / window(fn, 2)))
    seen = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            seen[name].append(window(fn, counts[name]))
    return {name: (statistics.median(v), min(v)) for name, v in seen.items()}, counts


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "path_time.json"))
    ap.add_argument("--paths", type=int, nargs="*", default=list(PATHS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("path_time: no GPU; nothing is measured without one")
    ftn = ge.load_package()
    sc, rt = ftn.score, ftn.runtime
    dev = torch.device("cuda:0")
    B, H, N = BHN
    g = torch.Generator(device=dev).manual_seed(B + N)
    y = torch.poisson(torch.full((B, H, N), 4.0, device=dev), generator=g)
    rows = []
    for P in args.paths:
        x = torch.poisson(torch.full((P, B, H, N), 4.0, device=dev), generator=g)
        for w in WINDOWS:
            with torch.inference_mode():
                hip = sc.path_summary(x, LEVELS, y, window=w, backend="hip")
                ref = sc.path_summary(x, LEVELS, y, window=w, backend="torch")
                same = all(torch.equal(hip[k], ref[k]) for k in ("quantiles", "mean", "crps"))
                del hip, ref
                times, counts = alternated({
                    "hip": lambda: sc.path_summary(x, LEVELS, y, window=w, backend="hip"),
                    "torch": lambda: sc.path_summary(x, LEVELS, y, window=w, backend="torch")})
            outputs = (len(LEVELS) + 2) * B * (H // w) * N
            nbytes = 4 * (P * B * H * N + B * H * N + outputs)
            us, us_min = times["hip"]
            rows.append({"P": P, "shape": [B, H, N], "window": w, "levels": LEVELS, "form": rt.path_summary_form(x, y, w),
                         "equal_to_torch": same, "calls_per_window": counts, "rounds": ROUNDS,
                         "path_summary_us": us, "path_summary_us_min": us_min, "algorithmic_bytes": nbytes,
                         "bytes_per_s": nbytes / (us * 1e-6), "share_of_hbm_peak": nbytes / (us * 1e-6) / HBM_PEAK,
                         "torch_us": times["torch"][0], "torch_us_min": times["torch"][1],
                         "torch_over_hip": times["torch"][0] / us})
            print(json.dumps(rows[-1]), flush=True)
        del x
        torch.cuda.empty_cache()
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
                                          "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
