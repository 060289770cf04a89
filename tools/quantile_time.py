"""Times ``k_nb_cdf`` and ``k_nb_quantile`` (5 levels: 0.025, 0.1, 0.5, 0.9, 0.975) with device events, beside
``k_score_cols`` on the same tensors as the memory-bound yardstick.  Warm-up, then the median of 20 runs.  The cost
per element depends on the data, so each row states its regime: rate log-uniform in [mu_lo, mu_hi], dispersion
log-uniform in [alpha_lo, alpha_hi], y ~ Poisson(rate).

    python tools/quantile_time.py --out profiles/quantile_time.json
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

SHAPES = [(256, 96, 512), (64, 96, 4096)]
LEVELS = [0.025, 0.1, 0.5, 0.9, 0.975]
REGIMES = {"fixtures": ((1e-3, 2e3), (1e-3, 5.0)), "counts": ((0.5, 50.0), (0.05, 1.0))}


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out), min(out)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "quantile_time.json"))
    args = ap.parse_args()
    ftn = ge.load_package()
    rt = ftn.runtime
    dev = torch.device("cuda:0")
    rows = []
    for B, H, N in SHAPES:
        for regime, ((mlo, mhi), (alo, ahi)) in REGIMES.items():
            g = torch.Generator(device=dev).manual_seed(B + N)
            u = lambda lo, hi: torch.exp(torch.rand(B, H, N, generator=g, device=dev) * math.log(hi / lo) + math.log(lo))
            rate, disp = u(mlo, mhi), u(alo, ahi)
            y = torch.poisson(rate, generator=g)
            out = torch.empty(len(LEVELS), B, H, N, device=dev)
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            with torch.inference_mode():
                us_cdf, min_cdf = timed(lambda: rt.nb_cdf(y, rate, disp))
                us_q, min_q = timed(lambda: rt.nb_quantiles(rate, disp, LEVELS, out=out, flag=flag))
                us_cols, _ = timed(lambda: rt.score_columns(y, rate, disp))
            n = B * H * N
            rows.append({"shape": [B, H, N], "regime": regime, "mu": [mlo, mhi], "alpha": [alo, ahi],
                         "form": rt.nbq_form(rate, disp, y), "levels": LEVELS, "flag": int(flag),
                         "k_nb_cdf_us": us_cdf, "k_nb_cdf_us_min": min_cdf, "k_nb_cdf_ns_per_element": us_cdf * 1e3 / n,
                         "k_nb_quantile_us": us_q, "k_nb_quantile_us_min": min_q,
                         "k_nb_quantile_ns_per_element_level": us_q * 1e3 / (n * len(LEVELS)),
                         "k_score_cols_us": us_cols})
            print(json.dumps(rows[-1]))
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "reps": 20, "rows": rows},
                                         indent=1) + "\n")


if __name__ == "__main__":
    main()
