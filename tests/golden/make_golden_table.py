"""Writes tests/golden/table_cases.npz, the fixture of tests/test_table_host.py and tests/test_gpu_table.py, from the
reference checkout (Flow-TimesNet, ``src/timesnet_forecast``): small wide tables and what the reference's own
``compute_series_features``, ``fit_series_scaler``, ``_transform_dataframe``, ``inverse_transform`` (plus the clip at 0
of predict.py:961), ``make_holdout_slices`` and ``make_rolling_slices`` returned on them.  Inputs and the reference's
outputs only.  Run once, with the reference checkout's root as argument:

    python tests/golden/make_golden_table.py REFERENCE_ROOT

Keys of the npz:
  meta                          one JSON string: {"tables": {name: {T, N, train: [r0, r1], val: [r0, r1], clip}},
                                "splits": [{T, kind, args, ranges}]}
  <t>:X / <t>:M                 the table (gaps filled with 0, as train.py:832 fills them) and its validity mask
  <t>:features                  compute_series_features(X, M)                                   [N, 5] fp32
  <t>:<method>:<ps|gl>:pairs    the scaler fit_series_scaler fitted on the train rows            [N, 2] fp64
  <t>:<method>:<ps|gl>:Xn       its normalised train rows (small tables only)                    fp32
  <t>:<method>:<ps|gl>:val      _transform_dataframe of the val rows with that scaler           fp32
                                (val and inv: every fit of the small tables, the per-series fits of ``planted``)
  <t>:pred                      a normalised forecast [H, N] fp32
  <t>:<method>:<ps|gl>:inv      clip(inverse_transform(pred), 0)                                [H, N] fp32

Tables: ``planted`` (T = 731, N = 37: Poisson counts whose rate carries a weekly and a yearly wave, 10 % gaps; the
generator asserts that the top two spectral bins of every column are at least 0.15 apart, relative), ``mixed``
(T = 97, N = 9: intermittent columns, an all-zero column, a constant column, a fully masked column and a column that is
constant below eps = 1e-8; its spectral totals are exactly 0, below 1e-12 or above 1), ``neg`` (T = 50, N = 6: signed
noise with a -0, fitted after ``clip(lower=0)`` as train.py:834-835 does) and ``t1``, ``t2``, ``t3`` (T = 1, 2, 3).
"""
from __future__ import annotations

import importlib
import json
import sys
from pathlib import Path

import numpy as np
import pandas as pd

HERE = Path(__file__).resolve().parent
FITS = [("zscore", True), ("zscore", False), ("minmax", True), ("minmax", False)]


def planted(g, T=731, N=37):
    t = np.arange(T)[:, None]
    base = g.uniform(2.0, 40.0, size=(1, N))
    weekly = g.uniform(0.35, 0.6, size=(1, N))
    yearly = g.uniform(0.05, 0.15, size=(1, N))
    ph = g.uniform(0, 2 * np.pi, size=(2, 1, N))
    # 731 = 104 weeks + 3 days: the weekly wave sits between bins 104 and 105, nearer 104
    rate = base * (1.0 + weekly * np.sin(2 * np.pi * t / 7.0 + ph[0]) + yearly * np.sin(2 * np.pi * t / 365.25 + ph[1]))
    X = g.poisson(rate).astype(np.float32)
    M = (g.random((T, N)) >= 0.10).astype(np.float32)
    return X * M, M


def mixed(g, T=97, N=9):
    X = (g.poisson(0.3, size=(T, N)) * g.integers(1, 9, size=(T, N))).astype(np.float32)
    M = (g.random((T, N)) >= 0.10).astype(np.float32)
    X[:, 2] = 0.0                                               # all zero
    X[:, 4] = 7.0                                               # constant
    M[:, 6] = 0.0                                               # fully masked
    X[:, 7] = np.where(np.arange(T) % 3 == 0, 3e-9, 0.0).astype(np.float32)     # constant below eps, not constant
    M[:, 7] = 1.0
    return X * M, M


def neg(g, T=50, N=6):
    X = (g.standard_normal((T, N)) * 5.0).astype(np.float32)
    X[3, 1] = -0.0
    return X, np.ones((T, N), np.float32)


def tiny(g, T, N=4):
    X = g.poisson(5.0, size=(T, N)).astype(np.float32)
    M = np.ones((T, N), np.float32)
    if T > 1:
        M[0, 1] = 0.0
        X[0, 1] = 0.0
    return X, M


def main(ref_root: Path) -> None:
    sys.path.insert(0, str(ref_root / "src"))
    feats = importlib.import_module("timesnet_forecast.utils.static_features").compute_series_features
    io = importlib.import_module("timesnet_forecast.utils.io")
    split = importlib.import_module("timesnet_forecast.data.split")
    transform = importlib.import_module("timesnet_forecast.train")._transform_dataframe
    g = np.random.default_rng(20240713)
    tables = {
        "planted": (*planted(g), (0, 600), (600, 731), False, False),
        "mixed": (*mixed(g), (0, 70), (70, 97), False, True),
        "neg": (*neg(g), (0, 36), (36, 50), True, True),
        "t1": (*tiny(g, 1), (0, 1), (0, 1), False, True),
        "t2": (*tiny(g, 2), (0, 2), (0, 2), False, True),
        "t3": (*tiny(g, 3), (0, 2), (2, 3), False, True),
    }
    out, meta = {}, {"tables": {}, "splits": []}
    for name, (X, M, trn, val, clip, keep_xn) in tables.items():
        T, N = X.shape
        ids = [f"s{j:03d}" for j in range(N)]
        wide, mask = pd.DataFrame(X, columns=ids), pd.DataFrame(M, columns=ids)
        out[f"{name}:X"], out[f"{name}:M"] = X, M
        f, names = feats(wide, mask)
        assert names == ["mean", "std", "diff_std", "seasonal_strength", "dominant_period"] and f.dtype == np.float32
        out[f"{name}:features"] = f
        if T > 1:                                               # how far apart the top two bins and the threshold are
            d = np.where(M > 0, X - f[:, 0][None, :], 0.0).astype(np.float64)
            P = np.abs(np.fft.rfft(d, axis=0))[1:] ** 2
            tot = P.sum(axis=0)
            assert all(t == 0 or t < 1e-12 or t > 1.0 for t in tot), (name, tot)
            if name == "planted":
                top = np.sort(P, axis=0)[::-1]
                gap = (top[0] - top[1]) / top[0]
                assert gap.min() >= 0.15, (name, gap.min())
                print(name, "smallest top-two gap", gap.min())
        fit_df = wide.clip(lower=0.0) if clip else wide         # train.py:834-835
        pred = (g.standard_normal((28 if T > 3 else 2, N)) * 1.5).astype(np.float32)
        out[f"{name}:pred"] = pred
        for method, per_series in FITS:
            key = f"{name}:{method}:{'ps' if per_series else 'gl'}"
            scaler, xn = io.fit_series_scaler(fit_df.iloc[trn[0]:trn[1]], method=method, per_series=per_series)
            out[f"{key}:pairs"] = np.array([scaler[c] for c in ids], dtype=np.float64)
            if keep_xn:
                out[f"{key}:Xn"] = xn.to_numpy(dtype=np.float32)
            if keep_xn or per_series:                           # the large table keeps these for the per-series fits only
                out[f"{key}:val"] = transform(fit_df.iloc[val[0]:val[1]], ids, scaler, method).to_numpy(dtype=np.float32)
                out[f"{key}:inv"] = np.clip(io.inverse_transform(pred, ids, scaler, method), 0.0, None)
        meta["tables"][name] = {"T": T, "N": N, "train": list(trn), "val": list(val), "clip": clip, "xn": keep_xn}
    for T in (1, 5, 40):
        df = pd.DataFrame(np.arange(T, dtype=np.float64).reshape(T, 1))
        rng = lambda part: [int(part.iloc[0, 0]), int(part.iloc[-1, 0]) + 1] if len(part) else [0, 0]
        for h in (1, 3, 5, 60):
            trn, val = split.make_holdout_slices(df, h)
            meta["splits"].append({"T": T, "kind": "holdout", "args": [h], "ranges": [[rng(trn), rng(val)]]})
        for args in ((3, 7, 10), (4, 10, 10), (9, 5, 8), (2, 1, 100), (3, 0, 4)):
            folds = [[rng(a), rng(b)] for a, b in split.make_rolling_slices(df, *args)]
            meta["splits"].append({"T": T, "kind": "rolling", "args": list(args), "ranges": folds})
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(HERE / "table_cases.npz", **out)
    print(len(out), "arrays,", (HERE / "table_cases.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
