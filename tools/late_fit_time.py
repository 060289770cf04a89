"""Times the late-bias refit (csrc/latefit.hip, ``fit.GraphedCachedStep(..., late_bias=True)``) at the pipeline layout
(batch 4096, N = 1, the series rows per item and read through a row list) and the bench layout (batch 256, N = 512, one
shared block of rows), S = 96 steps and ctx = 64, in one process:

  (a) ``runtime.late_fit_forward`` + ``runtime.late_backward`` replayed as one HIP graph, against the torch composition
      (``F.layer_norm``, ``F.linear``, the gate, autograd of ``sum(late * d_pre)``) on the same tensors, replayed as a
      graph too and also run eagerly
  (b) a replayed ``fit.GraphedCachedStep`` with ``late_bias=True`` (eleven tensors, ``fit.DeviceAdamWList``) against the
      step with ``late_bias=False`` (six tensors, ``fit.DeviceAdamW``: the launches of the cached step as it was before
      the late-bias refit, tests/test_gpu_late_refit.py pins the list) on the same windows

Method of tools/refit_step_time.py: the sides alternate round by round; device events surround ``--iters`` iterations
after a warm-up; the median of ``--rounds`` rounds is kept beside all of them and their spread (max - min).

    python tools/late_fit_time.py --out profiles/late_fit_time.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
LR, WD, CLIP, EPS = 1e-3, 0.01, 1.0, 1e-5
S, CTX = 96, 64
# name, batch, row blocks Bc, N, items of the row store (0: no row list)
KERNEL_SHAPES = [("pipeline", 4096, 4096, 1, 8192), ("bench", 256, 1, 512, 0)]
# name, batch, L, d_model, N of a batch, layout, series of the table, windows of the table
STEP_SHAPES = [("pipeline", 4096, 28, 64, 1, "series", 1024, 8), ("bench", 256, 336, 64, 512, "wide", 512, 512)]


def rounds(fns, iters, warm, reps):
    """us per iteration of every function (each runs ``iters`` iterations itself), alternated round by round."""
    for fn in fns.values():
        fn(warm)
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(iters)
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: {"us": statistics.median(v), "all": v, "spread": max(v) - min(v)} for k, v in out.items()}


def captured(fn):
    """``fn`` warmed up on a side stream, captured, and a function that replays it n times."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()

    def run(n):
        for _ in range(n):
            graph.replay()

    run.keep = keep
    return run


def kernel_row(ftn, dev, shape, args):
    rt = ftn.runtime
    name, B, Bc, N, items = shape
    g = torch.Generator(device=dev).manual_seed(B + N)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
    store = rnd(items, CTX) if items else rnd(Bc, N, CTX)
    index = torch.randint(0, items, (B,), generator=g, device=dev) if items else None
    params = [1.0 + 0.1 * rnd(CTX), 0.1 * rnd(CTX), rnd(S, CTX) / 8.0, 0.1 * rnd(S), (0.05 + 0.01 * rnd(S)).reshape(1, S, 1)]
    d_pre = rnd(B, S, N) / (B * S * N)
    ws = torch.empty(rt.late_backward_workspace(B, Bc, N, CTX, S), dtype=torch.uint8, device=dev)
    late = torch.empty(Bc if not items else B, S, N, device=dev)
    outs = [torch.empty_like(p).reshape(-1) if k != 2 else torch.empty_like(p) for k, p in enumerate(params)]

    def hip():
        rt.late_fit_forward(store, *params, EPS, rows=index, out=late)
        return rt.late_backward(d_pre, store, *params, EPS, rows=index, out=outs, workspace=ws)

    leaves = [p.clone().requires_grad_() for p in params]

    def composition():
        r = store if index is None else store.index_select(0, index).unsqueeze(1)
        lb = F.linear(F.layer_norm(r, (CTX,), leaves[0], leaves[1], EPS), leaves[2], leaves[3])
        out = leaves[4] * lb.transpose(1, 2)
        return torch.autograd.grad((out * d_pre).sum(), leaves)

    def eager(n):
        for _ in range(n):
            composition()

    t = rounds({"hip_graph": captured(hip), "torch_graph": captured(composition), "torch_eager": eager},
               args.kernel_iters, 10, args.rounds)
    got, want = hip(), composition()
    torch.cuda.synchronize()
    dist = max(float((a.reshape(-1) - b.reshape(-1)).abs().max()) for a, b in zip(got, want))
    row = {"shape": name, "B": B, "Bc": Bc, "N": N, "S": S, "ctx": CTX, "row_list_items": items,
           "form": list(rt.late_backward_form_of(B, Bc, N, CTX, S)), "workspace_bytes": ws.numel(),
           "iters": args.kernel_iters, **t, "torch_graph_over_hip_graph": t["torch_graph"]["us"] / t["hip_graph"]["us"],
           "max_abs_gradient_distance_to_torch": dist}
    print(json.dumps(row), flush=True)
    return row


def build(ftn, dev, shape):
    """The model of tools/refit_cache_time.py with statics (8 features -> 32) beside the id embedding (32): ctx = 64."""
    name, B, L, D, N, layout, series, windows = shape
    torch.manual_seed(B + N)
    model = ftn.models.TimesNet(input_len=L, pred_len=S, d_model=D, d_ff=4 * D, n_layers=2, k_periods=3,
                                kernel_set=[(3, 3), (5, 5), (7, 7)], dropout=0.0, activation="gelu", mode="direct",
                                use_checkpoint=False, id_embed_dim=32, static_proj_dim=32,
                                use_late_bias_head=True).eval().to(dev)
    g = torch.Generator(device=dev).manual_seed(B + N)
    T = L + S + windows - 1
    t = torch.arange(T, dtype=torch.float32, device=dev).view(T, 1)
    table = torch.poisson(2.0 + torch.sin(2 * torch.pi * t / 7.0) + torch.rand(T, series, generator=g, device=dev),
                          generator=g)
    valid = (torch.rand(T, series, generator=g, device=dev) >= 0.2).float()
    win = ftn.windows.DeviceWindows(table, L, S, valid_mask=valid, batch_size=B, layout=layout, shuffle=True,
                                    drop_last=True, seed=1, series_static=torch.randn(series, 8, generator=g, device=dev),
                                    series_ids=torch.arange(series))
    with torch.no_grad():
        xb, _, _, x_mark, _, static, ids = ftn.score._unpack_batch(win.batch(0, epoch=0))
        model(xb[:2], None if x_mark is None else x_mark[:2], static if static is None or static.dim() == 2 else static[:2],
              ids if ids is None or ids.dim() == 1 else ids[:2])
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g, device=dev))
        model.output_inputs(xb, x_mark, static, ids)
    return model, win


def step_row(ftn, dev, shape, args):
    fit = ftn.fit
    name, B = shape[0], shape[1]
    model, win = build(ftn, dev, shape)
    runs, info = {}, {}
    for flag in (False, True):
        cache = fit.OutputCache(model, win, use_loss_mask=True, late_bias=flag)
        params = fit._refit_params(model) + (fit._late_params(model) if flag else [])
        opt = (fit.DeviceAdamWList if flag else fit.DeviceAdamW)(params, lr=LR, weight_decay=WD, max_norm=CLIP)
        step = fit.GraphedCachedStep(cache, model, opt, B, late_bias=flag)
        step.rows.copy_(win.order(0)[:B])
        key = "eleven_late_bias" if flag else "six"

        def run(n, step=step):
            for _ in range(n):
                step.replay()

        runs[key] = run
        info[key] = {"cache_bytes": cache.nbytes, "late_per_item": cache.late_per_item, "optimizer": opt}
    t = rounds(runs, args.iters, 3, args.rounds)
    row = {"shape": name, "x": [B, shape[2], shape[4]], "d_model": shape[3], "steps": S, "layout": shape[5],
           "ctx": int(model.late_bias_head.in_features), "iters": args.iters, **t,
           "added_us": t["eleven_late_bias"]["us"] - t["six"]["us"],
           "cache_bytes": {k: v["cache_bytes"] for k, v in info.items()},
           "late_per_item": info["six"]["late_per_item"],
           "flagged_steps": {k: int((v["optimizer"].history()[:, 3] != 0).sum()) for k, v in info.items()}}
    print(json.dumps(row), flush=True)
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "late_fit_time.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernel-iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    ftn = ge.load_package()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "what": "us per iteration: median of the rounds, all rounds, spread = max - min; sides alternate by round",
           "a_late_forward_backward": [kernel_row(ftn, dev, s, args) for s in KERNEL_SHAPES],
           "b_cached_step": [step_row(ftn, dev, s, args) for s in STEP_SHAPES]}
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
