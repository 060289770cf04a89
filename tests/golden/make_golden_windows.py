"""Writes tests/golden/windows_cases.npz, the fixture of tests/test_windows_host.py and tests/test_gpu_windows.py, from
the reference checkout (Flow-TimesNet, ``src/timesnet_forecast``): small wide tables and every batch that the
reference's own ``data.dataset.SlidingWindowDataset`` behind ``torch.utils.data.DataLoader(shuffle=False,
drop_last=False)`` yielded on them.  Run once, with the reference checkout's root as argument:

    python tests/golden/make_golden_windows.py REFERENCE_ROOT

Keys of the npz:
  cases                     one JSON string: {case: {"parts": [{T, N, L, pred_len, mode, recursive_pred_len, stride,
                            mask, F, Fs, ids}, ...], "batch": batch size, "batches": n, "pieces": tuple length}}
  <case>:p<k>:X / M / marks / static / ids     the tables of part k (absent: not given)
  <case>:b<i>:<j>           piece j of batch i as the loader returned it

Cases: ``probe`` (T=23, N=5, L=7, H=3, stride 2, batch 4, every optional piece; batch 1 straddles windows 0 and 1),
``bare`` (the same without any optional piece: marks [B, 0]), ``rec3`` / ``rec1`` (recursive mode with
recursive_pred_len 3 / the default 1), ``one`` (T = L + H: one window), ``none`` (T = L + H - 1: no batch) and
``concat`` (a ConcatDataset of two tables of 5 and 3 series, batch 6).
"""
from __future__ import annotations

import importlib
import json
import sys
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import ConcatDataset, DataLoader

HERE = Path(__file__).resolve().parent

FULL = dict(mask=True, F=3, Fs=2, ids=True)
BARE = dict(mask=False, F=0, Fs=0, ids=False)


def part(T, N, L, pred_len, mode="direct", recursive_pred_len=None, stride=1, **opt):
    return dict(T=T, N=N, L=L, pred_len=pred_len, mode=mode, recursive_pred_len=recursive_pred_len, stride=stride,
                **{**FULL, **opt})


CASES = {
    "probe": ([part(23, 5, 7, 3, stride=2)], 4),
    "bare": ([part(23, 5, 7, 3, stride=2, **BARE)], 4),
    "rec3": ([part(19, 4, 6, 5, mode="recursive", recursive_pred_len=3, stride=3)], 5),
    "rec1": ([part(12, 3, 5, 4, mode="recursive", F=1, Fs=0)], 7),
    "one": ([part(10, 5, 7, 3)], 4),
    "none": ([part(9, 5, 7, 3)], 4),
    "concat": ([part(14, 5, 7, 3, stride=2), part(16, 3, 7, 3, stride=3)], 6),
}


def tables(p, g):
    T, N = p["T"], p["N"]
    t = {"X": g.standard_normal((T, N)).astype(np.float32) * 10.0}
    if p["mask"]:
        t["M"] = (g.random((T, N)) >= 0.25).astype(np.float32)
    if p["F"]:
        t["marks"] = g.standard_normal((T, p["F"])).astype(np.float32)
    if p["Fs"]:
        t["static"] = g.standard_normal((N, p["Fs"])).astype(np.float32)
    if p["ids"]:
        t["ids"] = g.permutation(1000)[:N].astype(np.int64)
    return t


def main(ref_root: Path) -> None:
    sys.path.insert(0, str(ref_root / "src"))
    Dataset = importlib.import_module("timesnet_forecast.data.dataset").SlidingWindowDataset
    g = np.random.default_rng(20240611)
    out, meta = {}, {}
    for case, (parts, batch) in CASES.items():
        sets = []
        for k, p in enumerate(parts):
            t = tables(p, g)
            for name, arr in t.items():
                out[f"{case}:p{k}:{name}"] = arr
            sets.append(Dataset(t["X"], p["L"], p["pred_len"], p["mode"], recursive_pred_len=p["recursive_pred_len"],
                                stride=p["stride"], valid_mask=t.get("M"), series_static=t.get("static"),
                                series_ids=t.get("ids"), time_features=t.get("marks")))
        ds = sets[0] if len(sets) == 1 else ConcatDataset(sets)
        n, pieces = 0, 0
        if len(ds):
            for n, b in enumerate(DataLoader(ds, batch_size=batch, shuffle=False, drop_last=False), 1):
                pieces = len(b)
                for j, piece in enumerate(b):
                    out[f"{case}:b{n - 1}:{j}"] = piece.numpy()
        meta[case] = {"parts": parts, "batch": batch, "batches": n, "pieces": pieces}
    out["cases"] = np.array(json.dumps(meta))
    np.savez_compressed(HERE / "windows_cases.npz", **out)
    print({c: (m["batches"], m["pieces"]) for c, m in meta.items()}, (HERE / "windows_cases.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main(Path(sys.argv[1]))
