"""Times the table preparation (``table.series_features``, ``SeriesScaler.fit`` / ``transform`` / ``inverse``), three
alternatives per call in one process:
  (a) the HIP backend (csrc/table.hip);
  (b) the same result composed from torch ops on the device (reductions, ``torch.fft.rfft``, elementwise ops);
  (c) the torch backend on the host cores (the reference's numpy restated) - a host clock, one call.
Shapes: T in {731, 1913, 4096} x N in {512, 4096, 30490} with a 10 % gap mask, and ``inverse`` also at the pipeline
layout [B, H, 1] = [65536, 28, 1] with a row-to-series map into 30490 columns.
(a) and (b) are alternated round by round between device events, windows of at least 0.3 s after a warm-up, the median
of 3 rounds.  The kernels of (a) are also timed alone (moments, spectrum) and held against the chip: the spectrum as
2 T^2 N fp32 matrix operations (cos and sin products of T / 2 bins) over the fp32 matrix peak, the moments and the
affine pass as the bytes they must move over the HBM peak (MI355X: 157.3 TFLOP/s, 8.0 TB/s spec).  Fails without a GPU.

    python tools/table_time.py --out profiles/table_time.json [--quick]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import __graft_entry__ as ge  # noqa: E402
from group_time import ROUNDS, window  # noqa: E402

WINDOW_S = 0.3
PEAK_F32_MATRIX, PEAK_HBM = 157.3e12, 8.0e12
TS, NS = (731, 1913, 4096), (512, 4096, 30490)


def alternated(fns, window_s=WINDOW_S):
    counts = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        counts[name] = max(3, int(window_s * 1e6 / window(fn, 2)) + 1)
    seen = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            seen[name].append(window(fn, counts[name]))
    return {name: {"us": statistics.median(v), "us_min": min(v), "calls_per_window": counts[name]}
            for name, v in seen.items()}


def composed_features(X, M):
    """compute_series_features as torch ops on the device (fp32 throughout, as the reference)."""
    T = X.shape[0]
    cnt = M.sum(0)
    mean = (X * M).sum(0) / cnt.clamp_min(1e-6)
    cen = (X - mean) * M
    std = ((cen * cen).sum(0) / cnt.clamp_min(1.0)).clamp_min(0).sqrt()
    d, dm = X[1:] - X[:-1], M[1:] * M[:-1]
    dcnt = dm.sum(0)
    dmean = (d * dm).sum(0) / dcnt.clamp_min(1e-6)
    dc = (d - dmean) * dm
    dstd = ((dc * dc).sum(0) / dcnt.clamp_min(1.0)).clamp_min(0).sqrt()
    P = torch.fft.rfft(torch.where(M > 0, X - mean, torch.zeros((), device=X.device)), dim=0).abs()[1:] ** 2
    peak, idx = P.max(0)
    tot = P.sum(0)
    strength = peak / tot.clamp_min(1e-6)
    period = torch.where(tot > 1e-6, T / (idx + 1).to(torch.float32), torch.zeros((), device=X.device))
    return torch.stack([mean, std, dstd, strength, period], dim=1)


def composed_fit(X):
    mu, sd = X.mean(0), X.std(0, unbiased=False)
    return mu, torch.where(sd < 1e-8, torch.ones_like(sd), sd)


def host_once(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "table_time.json"))
    ap.add_argument("--quick", action="store_true", help="the smallest and the largest shape only, shorter windows")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("table_time: no GPU; nothing is measured without one")
    ftn = ge.load_package()
    tb, rt = ftn.table, ftn.runtime
    dev = torch.device("cuda:0")
    win = 0.1 if args.quick else WINDOW_S
    shapes = [(T, N) for T in TS for N in NS]
    if args.quick:
        shapes = [shapes[0], shapes[-1]]
    rows = []
    for T, N in shapes:
        g = torch.Generator().manual_seed(T * 7 + N)
        t = torch.arange(T, dtype=torch.float32)[:, None]
        rate = (2 + 30 * torch.rand(1, N, generator=g)) * (1 + 0.5 * torch.sin(2 * torch.pi * t / 7 + 6 * torch.rand(1, N, generator=g)))
        Mh = (torch.rand(T, N, generator=g) >= 0.1).float()
        Xh = torch.poisson(rate, generator=g) * Mh
        X, M = Xh.to(dev), Mh.to(dev)
        row = {"T": T, "N": N, "table_bytes": T * N * 4,
               "forms": {"moments": rt.table_moments(X, M, diffs=True, form=True),
                         "spectrum": rt.table_spectrum(X, None, M, form=True)}}
        feats = tb.series_features(X, M)
        assert tb._last_backend == "hip"
        try:
            comp = composed_features(X, M)
            row["features_agree"] = {"dominant_period_equal_share": float((comp[:, 4] == feats[:, 4]).float().mean()),
                                     "seasonal_strength_max_rel": float(((comp[:, 3] - feats[:, 3]).abs()
                                                                         / comp[:, 3].abs().clamp_min(1e-30)).max())}
            fns = {"hip": lambda: tb.series_features(X, M), "torch_composed": lambda: composed_features(X, M)}
        except RuntimeError as exc:                             # an fft length the library refuses, or memory
            row["torch_composed_error"] = str(exc)[:200]
            fns = {"hip": lambda: tb.series_features(X, M)}
        row["series_features"] = alternated(fns, win)
        stats = rt.table_moments(X, M, diffs=True)
        mean = stats[2].to(torch.float32)
        parts = alternated({"moments": lambda: rt.table_moments(X, M, diffs=True),
                            "spectrum": lambda: rt.table_spectrum(X, mean, M)}, win)
        s_us, m_us = parts["spectrum"]["us"], parts["moments"]["us"]
        parts["spectrum"].update(tflops=2.0 * T * T * N / s_us / 1e6,
                                 share_of_fp32_matrix_peak=2.0 * T * T * N / (s_us * 1e-6) / PEAK_F32_MATRIX)
        parts["moments"].update(tb_per_s=4.0 * T * N * 4 / m_us / 1e6,
                                share_of_hbm_peak=4.0 * T * N * 4 / (m_us * 1e-6) / PEAK_HBM)
        row["kernels"] = parts
        row["fit_zscore"] = alternated({"hip": lambda: tb.SeriesScaler.fit(X, "zscore"),
                                        "torch_composed": lambda: composed_fit(X)}, win)
        sc = tb.SeriesScaler.fit(X, "zscore")
        out = torch.empty_like(X)
        row["transform"] = alternated({"hip": lambda: sc.transform(X, out=out),
                                       "torch_composed": lambda: torch.div(torch.sub(X, sc.loc), sc.scale, out=out)}, win)
        row["inverse"] = alternated({"hip": lambda: sc.inverse(X, out=out),
                                     "torch_composed": lambda: torch.clamp_min(X * sc.scale + sc.loc, 0)}, win)
        for k in ("transform", "inverse"):
            us = row[k]["hip"]["us"]
            row[k]["hip"].update(tb_per_s=2.0 * T * N * 4 / us / 1e6, share_of_hbm_peak=2.0 * T * N * 4 / (us * 1e-6) / PEAK_HBM)
        row["host_torch_backend_us"] = {"series_features": host_once(lambda: tb.series_features(Xh, Mh)),
                                        "fit_zscore": host_once(lambda: tb.SeriesScaler.fit(Xh, "zscore"))}
        hs = tb.SeriesScaler.fit(Xh, "zscore")
        row["host_torch_backend_us"]["transform"] = host_once(lambda: hs.transform(Xh))
        row["host_torch_backend_us"]["inverse"] = host_once(lambda: hs.inverse(Xh))
        for k in ("series_features", "fit_zscore", "transform", "inverse"):
            if "torch_composed" in row[k]:
                row[k]["hip_over_torch_composed"] = row[k]["hip"]["us"] / row[k]["torch_composed"]["us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del X, M, out, feats, stats
        torch.cuda.empty_cache()
    # the pipeline layout: a forecast [B, H, 1] whose batch rows are series of a 30490-column table
    B, H, Ncols = 65536, 28, 30490
    g = torch.Generator().manual_seed(5)
    pairs = torch.stack([torch.rand(Ncols, generator=g) * 20, torch.rand(Ncols, generator=g) * 5 + 0.5], dim=1)
    sc = tb.SeriesScaler.from_pairs("zscore", pairs.numpy(), device=dev)
    ids = torch.randint(0, Ncols, (B,), generator=g).to(dev)
    x = torch.randn(B, H, 1, generator=g).to(dev)
    out = torch.empty_like(x)
    pipe = {"B": B, "H": H, "columns": Ncols,
            "form": rt.table_affine(x, sc.loc, sc.inv_scale, axis=0, series=ids, inverse=True, form=True)}
    pipe.update(alternated({"hip": lambda: sc.inverse(x, axis=0, series=ids, out=out),
                            "torch_composed": lambda: torch.clamp_min(x * sc.inv_scale[ids].view(B, 1, 1)
                                                                      + sc.loc[ids].view(B, 1, 1), 0)}, win))
    pipe["hip"].update(share_of_hbm_peak=2.0 * B * H * 4 / (pipe["hip"]["us"] * 1e-6) / PEAK_HBM)
    pipe["hip_over_torch_composed"] = pipe["hip"]["us"] / pipe["torch_composed"]["us"]
    xh, idh = x.cpu(), ids.cpu()
    hsc = tb.SeriesScaler.from_pairs("zscore", pairs.numpy(), device="cpu")
    pipe["host_torch_backend_us"] = host_once(lambda: hsc.inverse(xh, axis=0, series=idh))
    print(json.dumps(pipe), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": ROUNDS, "window_s": win,
                                          "peaks": {"fp32_matrix_flops": PEAK_F32_MATRIX, "hbm_bytes_per_s": PEAK_HBM},
                                          "rows": rows, "inverse_pipeline_layout": pipe}, indent=1) + "\n")


if __name__ == "__main__":
    main()
