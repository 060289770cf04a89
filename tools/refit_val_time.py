"""Times the end of a validated refit's epoch (``fit.GraphedCachedEval`` + ``fit.EpochEnd``) at the two shapes of
tools/refit_cache_time.py (pipeline [4096, 28, 1] -> 7 steps, series layout; bench [256, 336, 512] -> 96 steps, wide
layout), in the same run:

  (a) device: the validation pass over the held-out windows from their ``OutputCache`` (one replay of a
      ``GraphedCachedEval`` per batch) followed by ``EpochEnd.end_epoch`` - nothing read on the host; the window
      ends in a device event
  (b) host-driven, the way the code before this change allows it: ``score.eval_metrics`` on the whole model over the
      same held-out windows (its ``result()`` is a synchronisation), Python comparisons, and a clone of the six
      tensors by the host
  (c) ``ftn_refit_epoch_end`` alone (the decide kernel; no tensors to keep) for 1, 512 and 4096 slots

Method of tools/refit_step_time.py: the sides alternate round by round; device events surround ``--iters`` epochs
after a warm-up; the median of ``--rounds`` rounds is kept beside all of them and their spread (max - min).

    python tools/refit_val_time.py --out profiles/refit_val_time.json
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
from refit_cache_time import LR, SHAPES, build, rounds  # noqa: E402


def held_out(ftn, dev, shape):
    """A default loader over a table of the training table's size from another seed."""
    name, B, L, D, S, N, layout, series, windows = shape
    g = torch.Generator(device=dev).manual_seed(B + N + 1)
    T = L + S + windows - 1
    t = torch.arange(T, dtype=torch.float32, device=dev).view(T, 1)
    table = torch.poisson(2.0 + torch.sin(2 * torch.pi * t / 7.0) + torch.rand(T, series, generator=g, device=dev),
                          generator=g)
    valid = (torch.rand(T, series, generator=g, device=dev) >= 0.2).float()
    return ftn.windows.DeviceWindows(table, L, S, valid_mask=valid, batch_size=B, layout=layout)


def shape_row(ftn, dev, shape, args):
    fit, score = ftn.fit, ftn.score
    name, B, L, D, S, N, layout, series, windows = shape
    model, _ = build(ftn, dev, shape)
    val = held_out(ftn, dev, shape)
    nb = len(val)
    params = fit._refit_params(model)
    vcache = fit.OutputCache(model, val, use_loss_mask=True)
    opt = fit.DeviceAdamW(params, lr=LR)
    end = fit.EpochEnd(params, N, 1 << 16, LR, patience=None, plateau=dict(factor=0.5, patience=2))
    evaluator = fit.GraphedCachedEval(vcache, model, end.accumulators, B)
    rows = torch.arange(val.n_items, dtype=torch.int64, device=dev)

    def device(n):
        for _ in range(n):
            for k0 in range(0, val.n_items, B):
                evaluator.run(rows[k0:k0 + B])
            end.end_epoch(opt)

    best = {"nll": float("inf")}

    def host(n):
        for _ in range(n):
            r = score.eval_metrics(model, val, "direct", S, use_loss_mask=True, n_series=N)
            if r["nll"] <= best["nll"]:                         # every epoch keeps a copy, as the first epochs do
                best["nll"], best["state"] = r["nll"], [p.detach().clone() for p in params]

    t = rounds({"device": device, "host": host}, args.iters, 2, args.rounds)
    hist = end.history()
    r = score.eval_metrics(model, val, "direct", S, use_loss_mask=True, n_series=N)
    row = {"shape": name, "x": [B, L, N], "d_model": D, "steps": S, "layout": layout, "held_out_items": val.n_items,
           "batches": nb, "iters": args.iters, "a_device_epoch_end": t["device"], "b_host_driven_epoch_end": t["host"],
           "host_over_device": t["host"]["us"] / t["device"]["us"],
           "same_val_nll": hist["rows"][0, 0].item() == r["nll"], "val_nll": r["nll"],
           "flagged": [int(evaluator.bad_seen), int(evaluator.rows_seen)]}
    print(json.dumps(row), flush=True)
    return row


def decide_rows(ftn, dev, args):
    rt = ftn.runtime
    out = {}
    for n_slots in (1, 512, 4096):
        acc = torch.zeros(n_slots * 24, dtype=torch.uint8, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        den, seen = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        state = torch.zeros(64, dtype=torch.uint8, device=dev)
        state.view(torch.float64)[:3] = float("inf")
        lr = torch.full((1,), LR, dtype=torch.float32, device=dev)
        log = torch.zeros(1 << 16, 5, dtype=torch.float64, device=dev)

        def run(n):
            for _ in range(n):
                rt.refit_epoch_end(acc, err, den, seen, state, lr, log, None, (0.5, 2, 1e-4, 0.0))

        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            run(3)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run(args.kernel_iters)
        # one replay is kernel_iters calls whatever count it is asked for: back-to-back kernels without the host
        t = rounds({"eager": run, "graphed": lambda n: graph.replay()}, args.kernel_iters, 10, args.rounds)
        out[str(n_slots)] = {"eager_call": t["eager"], "in_a_graph": t["graphed"]}
    print(json.dumps(out), flush=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "refit_val_time.json"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    ftn = ge.load_package()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "what": "us per epoch end: (a) validation from the cache + EpochEnd on the device, (b) eval_metrics on the "
                   "whole model + result() + a clone of the six tensors, driven by the host; (c) us per "
                   "ftn_refit_epoch_end without tensors, as eager calls (the host's enqueue included) and as kernel_iters "
                   "calls captured in one graph",
           "shapes": [shape_row(ftn, dev, s, args) for s in SHAPES], "c_decide_by_slots": decide_rows(ftn, dev, args)}
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
