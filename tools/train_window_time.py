"""Times the batches of the training loader (``windows.DeviceWindows(shuffle=True, augment=...)``), in one process:
  hip                 shuffled + time-shifted + noised batches from ``ftn_window_gather`` (backend "hip");
  hip_shift_only      the same without noise: what the Philox calls and the fp64 Box-Muller of the noise cost;
  (a) torch           the torch backend on the same device (its noise goes through numpy on the host);
      torch_shift_only  the torch backend without noise: index arithmetic and advanced indexing on the device;
  (b) inorder         the in-order ``ftn_window_batch`` of the validation loader at the same shape.
Shapes: the pipeline shape (series layout, B=256, L=336, H=96, N=512, T=2000, 4 time features, 2 statics, ids, mask)
and a wide shape (B=32 windows of all 512 series, same table).  Every variant cycles through the batches of epoch 0
(the order is formed once, outside the timed region; its time is reported apart as ``order_us``); the variants are
alternated round by round, device events around windows of at least 0.3 s (at least 3 batches, at most 200) after a
warm-up; reported: the median, minimum and maximum of ROUNDS rounds.  Fails without a GPU.

    python tools/train_window_time.py --out profiles/train_window_time.json

The kernels alone: ``--dispatch-only K`` times nothing; per shape it forms batches 0 .. K of ``hip``, then of
``hip_shift_only``, then of ``inorder`` (the first call allocates, the K others fill the same ``out=`` buffers), for a
kernel trace in a run of its own; ``--summarise-trace CSV K`` then reads the trace's kernel rows in dispatch order
and writes the median, minimum and maximum of each run of K dispatches:

    rocprofv3 --kernel-trace --output-format csv -d trace -- python tools/train_window_time.py --dispatch-only 50
    python tools/train_window_time.py --summarise-trace trace/.../*_kernel_trace.csv 50 \
        --out profiles/train_window_kernel_time.json
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
sys.path.insert(0, str(ROOT / "tools"))
import __graft_entry__ as ge  # noqa: E402
from group_time import window  # noqa: E402

ROUNDS, WINDOW_S, MIN_BATCHES, MAX_BATCHES = 5, 0.3, 3, 200
DIMS = dict(T=2000, N=512, L=336, H=96)
SHAPES = (("pipeline_series_b256", "series", 256), ("wide_b32", "wide", 32))
AUGMENT = {"add_noise_std": 0.1, "time_shift": 3}


def tables(T, N, seed, series):
    g = torch.Generator().manual_seed(seed)
    t = dict(X=torch.poisson(torch.full((T, N), 4.0), generator=g), M=(torch.rand(T, N, generator=g) >= 0.1).float(),
             marks=torch.randn(T, 4, generator=g))
    if series:
        t.update(static=torch.randn(N, 2, generator=g), ids=torch.arange(N))
    return t


def cycle(w, epoch):
    state = {"i": 0}

    def step():
        b = w.batch(state["i"] % len(w)) if epoch is None else w.batch(state["i"] % len(w), epoch=epoch)
        state["i"] += 1
        return b
    return step


def alternated(fns):
    counts = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        counts[name] = min(MAX_BATCHES, max(MIN_BATCHES, int(WINDOW_S * 1e6 / window(fn, 2)) + 1))
    seen = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            seen[name].append(window(fn, counts[name]))
    return {name: {"us": statistics.median(v), "us_min": min(v), "us_max": max(v), "batches_per_window": counts[name]}
            for name, v in seen.items()}


DISPATCH_ORDER = ("hip", "hip_shift_only", "inorder")
KERNEL_OF = {"hip": "k_window_gather", "hip_shift_only": "k_window_gather", "inorder": "k_window_batch"}


def summarise_trace(path: str, K: int, out: str) -> None:
    """The kernel rows of a ``--dispatch-only K`` trace, in dispatch order: per shape and variant a run of K + 1
    dispatches of its kernel (the first, into fresh tensors, is dropped)."""
    import csv

    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    col = {k.lower(): k for k in rows[0]}
    name, start, end = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    rows.sort(key=lambda r: int(r[start]))
    seen = {k: [int(r[end]) - int(r[start]) for r in rows if k in r[name]]
            for k in set(KERNEL_OF.values())}
    at = {k: 0 for k in seen}
    result = []
    for shape, layout, batch in SHAPES:
        row = {"shape_name": shape, "layout": layout, **DIMS, "batch": batch, "dispatches": K}
        for variant in DISPATCH_ORDER:
            k = KERNEL_OF[variant]
            ns = seen[k][at[k] + 1:at[k] + 1 + K]
            at[k] += K + 1
            if len(ns) != K:
                raise SystemExit(f"summarise_trace: {k} has too few dispatches for {shape} / {variant}")
            row[variant] = {"kernel_us": statistics.median(ns) / 1e3, "kernel_us_min": min(ns) / 1e3,
                            "kernel_us_max": max(ns) / 1e3}
        result.append(row)
        print(json.dumps(row), flush=True)
    left = {k: len(v) - at[k] for k, v in seen.items()}
    if any(left.values()):
        raise SystemExit(f"summarise_trace: dispatches left over {left}: not a --dispatch-only {K} trace")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps({"source": "kernel trace", "augment": AUGMENT, "rows": result}, indent=1) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "train_window_time.json"))
    ap.add_argument("--dispatch-only", type=int, default=0, metavar="K")
    ap.add_argument("--summarise-trace", nargs=2, metavar=("CSV", "K"))
    args = ap.parse_args()
    if args.summarise_trace:
        summarise_trace(args.summarise_trace[0], int(args.summarise_trace[1]), args.out)
        return
    if not torch.cuda.is_available():
        raise SystemExit("train_window_time: no GPU; nothing is measured without one")
    ftn = ge.load_package()
    DW = ftn.windows.DeviceWindows
    dev = torch.device("cuda:0")
    rows = []
    for name, layout, batch in SHAPES:
        series = layout == "series"
        d = {k: v.to(dev) for k, v in tables(DIMS["T"], DIMS["N"], 1, series).items()}
        kw = dict(valid_mask=d["M"], time_features=d["marks"], series_static=d.get("static"), series_ids=d.get("ids"),
                  batch_size=batch, layout=layout)
        train = dict(shuffle=True, drop_last=True, seed=1)
        if args.dispatch_only:
            for variant in DISPATCH_ORDER:
                aug = {} if variant == "inorder" else dict(train, augment=AUGMENT if variant == "hip" else
                                                           {"time_shift": 3})
                w = DW(d["X"], DIMS["L"], DIMS["H"], backend="hip", **aug, **kw)
                call = (lambda i, out=None: w.batch(i, out=out)) if variant == "inorder" else (
                    lambda i, out=None: w.batch(i, out=out, epoch=0))
                bufs = call(0)
                for i in range(1, args.dispatch_only + 1):
                    call(i % (len(w) - 1), out=bufs)            # never the short last batch
                torch.cuda.synchronize()
            continue
        made = {"hip": DW(d["X"], DIMS["L"], DIMS["H"], backend="hip", augment=AUGMENT, **train, **kw),
                "hip_shift_only": DW(d["X"], DIMS["L"], DIMS["H"], backend="hip", augment={"time_shift": 3}, **train, **kw),
                "torch": DW(d["X"], DIMS["L"], DIMS["H"], backend="torch", augment=AUGMENT, **train, **kw),
                "torch_shift_only": DW(d["X"], DIMS["L"], DIMS["H"], backend="torch", augment={"time_shift": 3}, **train,
                                       **kw),
                "inorder": DW(d["X"], DIMS["L"], DIMS["H"], backend="hip", **kw)}
        hip, tor = made["hip_shift_only"], made["torch_shift_only"]
        order_us = window(lambda: (hip._orders.clear(), hip.order(0)), 20)
        same = torch.equal(hip.order(0), tor.order(0)) and all(
            torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                        b.view(torch.int32) if b.dtype == torch.float32 else b)
            for i in (0, len(hip) // 2, len(hip) - 1) for a, b in zip(hip.batch(i, epoch=0), tor.batch(i, epoch=0)))
        first = made["hip"].batch(0, epoch=0)
        noise_diff = float((first[0] - made["torch"].batch(0, epoch=0)[0]).abs().max())
        row = {"shape_name": name, "layout": layout, **DIMS, "batch": batch, "F": 4, "Fs": 2 if series else 0,
               "items": hip.n_items, "batches": len(hip), "augment": AUGMENT, "order_us": order_us,
               "bit_equal_hip_torch_shift_only": same, "noise_max_abs_diff_hip_torch": noise_diff,
               "bytes_written_per_batch": sum(p.numel() * p.element_size() for p in first[:7 if series else 5])}
        row.update(alternated({k: cycle(w, None if k == "inorder" else 0) for k, w in made.items()}))
        row["hip_over_torch"] = row["hip"]["us"] / row["torch"]["us"]
        row["hip_shift_only_over_torch_shift_only"] = row["hip_shift_only"]["us"] / row["torch_shift_only"]["us"]
        row["hip_over_inorder"] = row["hip"]["us"] / row["inorder"]["us"]
        row["hip_shift_only_over_inorder"] = row["hip_shift_only"]["us"] / row["inorder"]["us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d, made, hip, tor, first
        torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
                                          "window_s": WINDOW_S, "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
