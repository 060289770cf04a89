"""Times batch formation for a rolling-origin backtest (``windows.DeviceWindows``), three alternatives in one process:
  (a) the HIP launch (``ftn_window_batch``, backend "hip"), batches formed into fresh tensors;
  (b) the torch composition on the device (backend "torch": index arithmetic and advanced indexing);
  (c) a host restatement of the reference's loader: one ``__getitem__`` per item (slices cloned piece by piece),
      default collation (a stack per piece), and the copy of the batch to the device.
Shapes: the pipeline layout N=193, L=28, H=7, stride 1, T=730 (mask, 3 time features, 2 statics, ids) with batch 4096
and with batch 65 536, and the bench layout (wide) N=512, L=336, H=96, T=2000 with batch 256.
(a) and (b) are alternated round by round, device events around windows of at least 0.3 s and at least 200 batches
after a warm-up, the batches of the table taken in turn, the median of 3 rounds; (c) is a host clock around whole
batches ended by a device synchronise (at least 3 batches and 0.5 s; it takes milliseconds to seconds a batch).
Also: the share of a whole ``score.eval_metrics`` pass (a small TimesNet, pipeline layout, batch 4096, T=120) that
batch formation takes with (a) and with (c): the pass, and the same batches formed without the model, both by the
host clock with a synchronise at the end.  Fails without a GPU.

    python tools/window_time.py --out profiles/window_time.json

``--dispatch-only K`` times nothing: it forms batch 0 of every shape K times into the same buffers (``out=``), shape
after shape, for a kernel trace (``rocprofv3 --kernel-trace --stats -- python tools/window_time.py --dispatch-only 50``:
the dispatches of ``k_window_batch`` come in the order of the shapes).
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

MIN_BATCHES, WINDOW_S = 200, 0.3
SHAPES = (("pipeline_b4096", "series", dict(T=730, N=193, L=28, H=7), 4096),
          ("pipeline_b65536", "series", dict(T=730, N=193, L=28, H=7), 65536),
          ("bench_wide_b256", "wide", dict(T=2000, N=512, L=336, H=96), 256))


def tables(T, N, seed, series):
    g = torch.Generator().manual_seed(seed)
    t = dict(X=torch.poisson(torch.full((T, N), 4.0), generator=g), M=(torch.rand(T, N, generator=g) >= 0.1).float(),
             marks=torch.randn(T, 3, generator=g))
    if series:
        t.update(static=torch.randn(N, 2, generator=g), ids=torch.arange(N))
    return t


def host_loader(t, L, H, layout, batch, dev):
    """The reference's loop restated: items in order, every piece a cloned slice, a stack per piece, then the copy."""
    X, M, marks, static, ids = t["X"], t["M"], t["marks"], t.get("static"), t.get("ids")
    T, N = X.shape
    series = layout == "series"
    n_items = (T - L - H + 1) * (N if series else 1)

    def item(k):
        s, i = (k // N, k % N) if series else (k, None)
        e = s + L
        cols = slice(i, i + 1) if series else slice(None)
        out = [X[s:e, cols].clone(), X[e:e + H, cols].clone(), M[e:e + H, cols].clone(), marks[s:e].clone(),
               marks[e:e + H].clone()]
        if series:
            out += [static[i:i + 1].clone(), ids[i:i + 1].clone()]
        return out

    for k0 in range(0, n_items, batch):
        items = [item(k) for k in range(k0, min(k0 + batch, n_items))]
        yield tuple(torch.stack(p).to(dev, non_blocking=True) for p in zip(*items))


def alternated(fns):
    counts = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        counts[name] = max(MIN_BATCHES, int(WINDOW_S * 1e6 / window(fn, 8)) + 1)
    seen = {name: [] for name in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            seen[name].append(window(fn, counts[name]))
    return {name: {"us": statistics.median(v), "us_min": min(v), "batches_per_window": counts[name]}
            for name, v in seen.items()}


def cycle(w):
    state = {"i": 0}

    def step():
        b = w.batch(state["i"] % len(w))
        state["i"] += 1
        return b
    return step


def host_clock(make_iter, consume, min_batches=3, min_s=0.5):
    """Seconds per batch of ``consume(batch)`` over the iterator, at least ``min_batches`` and ``min_s``."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while n < min_batches or time.perf_counter() - t0 < min_s:
        for b in make_iter():
            consume(b)
            n += 1
            if n >= min_batches and time.perf_counter() - t0 >= min_s:
                break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, n


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "window_time.json"))
    ap.add_argument("--dispatch-only", type=int, default=0, metavar="K")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("window_time: no GPU; nothing is measured without one")
    ftn = ge.load_package()
    DW, rt = ftn.windows.DeviceWindows, ftn.runtime
    dev = torch.device("cuda:0")
    rows = []
    for name, layout, dims, batch in SHAPES:
        series = layout == "series"
        t = tables(dims["T"], dims["N"], 1, series)
        d = {k: v.to(dev) for k, v in t.items()}
        kw = dict(valid_mask=d["M"], time_features=d["marks"], series_static=d.get("static"), series_ids=d.get("ids"),
                  batch_size=batch, layout=layout)
        hip, tor = (DW(d["X"], dims["L"], dims["H"], backend=b, **kw) for b in ("hip", "torch"))
        first = hip.batch(0)
        if args.dispatch_only:
            for _ in range(args.dispatch_only):
                hip.batch(0, out=first)
            torch.cuda.synchronize()
            continue
        same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b)
                   for i in range(len(hip)) for a, b in zip(hip.batch(i), tor.batch(i)))
        outs = dict(zip(rt.WINDOW_PIECES if series else rt.WINDOW_PIECES[:5], first))
        form = rt.window_batch_form(d["X"], dims["L"], dims["H"], outs, M=d["M"], marks=d["marks"],
                                    statics=d.get("static"), ids=d.get("ids"), layout=layout)
        row = {"shape_name": name, "layout": layout, **dims, "batch": batch, "F": 3, "Fs": 2 if series else 0,
               "items": hip.n_items, "batches": len(hip), "bit_equal_hip_torch": same,
               "form": {"vec": list(form["vec"]), "tile": form["tile"]},
               "bytes_written_per_full_batch": sum(p.numel() * p.element_size() for p in first[:7 if series else 5])}
        row.update(alternated({"hip": cycle(hip), "torch_composition": cycle(tor)}))
        sec, n = host_clock(lambda: host_loader(t, dims["L"], dims["H"], layout, batch, dev), lambda b: None)
        row["host_loader"] = {"us": sec * 1e6, "batches_timed": n}
        row["hip_over_torch_composition"] = row["hip"]["us"] / row["torch_composition"]["us"]
        row["host_loader_over_hip"] = row["host_loader"]["us"] / row["hip"]["us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d, hip, tor, first
        torch.cuda.empty_cache()

    if args.dispatch_only:
        return
    # the share of an eval_metrics pass
    L, H, N, T, batch = 28, 7, 193, 120, 4096
    t = tables(T, N, 2, True)
    cfg = dict(input_len=L, pred_len=H, d_model=32, d_ff=64, n_layers=2, k_periods=3, kernel_set=[(3, 3), (5, 5)],
               dropout=0.0, activation="gelu", mode="direct", use_checkpoint=False, id_embed_dim=4)
    torch.manual_seed(0)
    model = ftn.models.TimesNet(**cfg).eval()
    with torch.no_grad():
        model(torch.rand(2, L, 1) + 1.0, x_mark=torch.randn(2, L, 3), series_static=torch.rand(2, 1, 2),
              series_ids=torch.tensor([[N - 1], [0]]))
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape))
    model = model.to(dev)
    w = DW(t["X"], L, H, valid_mask=t["M"], time_features=t["marks"], series_static=t["static"], series_ids=t["ids"],
           batch_size=batch, device=dev, backend="hip")
    share = {"T": T, "N": N, "L": L, "H": H, "batch": batch, "batches": len(w), "d_model": 32, "n_layers": 2}

    def pass_s(make):
        ftn.score.eval_metrics(model, make(), "direct", H, use_loss_mask=True, n_series=N)      # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ftn.score.eval_metrics(model, make(), "direct", H, use_loss_mask=True, n_series=N)      # result() synchronises
        return time.perf_counter() - t0

    def form_s(make):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in make():
            pass
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for key, make in (("hip", lambda: w), ("host_loader", lambda: host_loader(t, L, H, "series", batch, dev))):
        p, f = pass_s(make), form_s(make)
        share[key] = {"pass_s": p, "formation_s": f, "formation_share_of_pass": f / p}
    print(json.dumps(share), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": ROUNDS,
                                          "min_batches_per_window": MIN_BATCHES, "rows": rows,
                                          "eval_metrics_share": share}, indent=1) + "\n")


if __name__ == "__main__":
    main()
