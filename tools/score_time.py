"""Times ``ForecastScorer.update`` (``k_score_cols`` + ``k_score_fold``) against the same math composed from stock
PyTorch ops on the same device in the same run: the reference's ``negative_binomial_nll`` formula plus the masked sMAPE
terms and their per-series sums, without the reference's Python column loop.  Device events, median of 3 after a
warm-up.

    python tools/score_time.py --out profiles/score_time.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

SHAPES = [(256, 96, 512), (64, 96, 4096)]


def timed(fn, reps=3, warm=2):
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
    return statistics.median(out), out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "score_time.json"))
    args = ap.parse_args()
    ftn = ge.load_package()
    sc, rt = ftn.score, ftn.runtime
    dev = torch.device("cuda:0")
    rows = []
    for B, H, N in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B + N)
        rate = torch.exp(torch.rand(B, H, N, generator=g, device=dev) * 12.0 - 4.0)
        disp = torch.exp(torch.rand(B, H, N, generator=g, device=dev) * 15.8 - 13.8)
        y = torch.poisson(rate.clamp(max=1e4), generator=g)
        mask = torch.rand(B, H, N, generator=g, device=dev) >= 0.2
        scorer = sc.ForecastScorer(N, dev)
        acc = torch.zeros(N, 4, dtype=torch.float64, device=dev)

        def composed():
            ll, yc, mu, alpha = sc._nb_ll_torch(y, rate, disp, 1e-8)
            valid = sc.negative_binomial_mask(yc, mu, alpha, mask)
            terms, counts = sc._smape_terms_torch(y, rate, valid)
            neg = torch.where(valid, -ll, torch.zeros_like(ll))
            acc[:, 0] += neg.sum((0, 1), dtype=torch.float64)
            acc[:, 1] += terms.sum((0, 1), dtype=torch.float64)
            acc[:, 2] += valid.sum((0, 1))
            acc[:, 3] += counts.sum((0, 1))

        with torch.inference_mode():
            for maskname, m in (("none", None), ("bool", mask)):
                us_update, all_update = timed(lambda: scorer.update(y, rate, disp, m))
                us_cols, _ = timed(lambda: rt.score_columns(y, rate, disp, m))
                part, _ = rt.score_columns(y, rate, disp, m)
                err = torch.zeros(1, dtype=torch.int32, device=dev)
                acc2 = torch.zeros(N * 24, dtype=torch.uint8, device=dev)
                us_fold, _ = timed(lambda: rt.score_fold(part, B, N, acc2, err))
                us_torch, all_torch = timed(composed)
                nbytes = 4 * 3 * B * H * N + (B * H * N if m is not None else 0)
                rows.append({"shape": [B, H, N], "mask": maskname, "form": list(rt.score_form(y, rate, disp, m)),
                             "bytes": nbytes, "update_us": us_update, "update_us_all": all_update,
                             "k_score_cols_us": us_cols, "k_score_fold_us": us_fold,
                             "k_score_cols_TBps": nbytes / us_cols * 1e-6, "update_TBps": nbytes / us_update * 1e-6,
                             "torch_composed_us": us_torch, "torch_composed_us_all": all_torch,
                             "speedup_vs_torch": us_torch / us_update})
                print(json.dumps(rows[-1]))
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
