"""Times the cached refit (``fit.OutputCache`` / ``fit.GraphedCachedStep``) at the pipeline shape ([4096, 28, 1],
d_model 64 -> 7 steps; series layout) and the bench shape ([256, 336, 512], d_model 64 -> 96 steps; wide layout), in
the same run:

  (a) a replayed ``fit.GraphedCachedStep`` on a batch of an epoch's shuffled order
  (b) a replayed ``fit.GraphedRefitStep`` on a batch of the same windows: the step with the backbone in it, which the
      cache does not touch.  ``--parent-tree DIR`` (a checkout of the parent commit with its library built) times it
      there in a child process instead; the file says which.
  (c) the fill of the cache per canonical batch, and the number of epochs from which fill + cached epochs undercut
      uncached epochs
  (d) ``timeproj_forward`` and ``timeproj_backward`` with an identity row list against the unmapped call on the same
      tensor

Method of tools/refit_step_time.py: the sides alternate round by round; device events surround ``--iters`` iterations
after a warm-up; the median of ``--rounds`` rounds is kept beside all of them and their spread (max - min).

    python tools/refit_cache_time.py --out profiles/refit_cache_time.json --error-out profiles/refit_cache_error.json

``--error-out``: on the tiny model of the tests, the distance between the six tensors after a cached shuffled refit
and after ``fit.refit_output`` on the same shuffled windows (which re-selects periods in every shuffled batch).
"""
from __future__ import annotations

import argparse
import copy
import json
import math
import os
import statistics
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
LR, WD, CLIP = 1e-3, 0.01, 1.0
# name, batch, L, d_model, steps, N of a batch, layout, series of the table, windows of the table
SHAPES = [("pipeline", 4096, 28, 64, 7, 1, "series", 1024, 8), ("bench", 256, 336, 64, 96, 512, "wide", 512, 512)]


def rounds(fns, iters, warm, reps):
    """us per iteration of every function (each runs ``iters`` iterations itself), alternated round by round."""
    for fn in fns.values():
        fn(warm)
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


def build(ftn, dev, shape):
    """The model (two TimesBlocks with the bench's kernel set) and shuffled windows of two or more batches."""
    name, B, L, D, S, N, layout, series, windows = shape
    torch.manual_seed(B + N)
    model = ftn.models.TimesNet(input_len=L, pred_len=S, d_model=D, d_ff=4 * D, n_layers=2, k_periods=3,
                                kernel_set=[(3, 3), (5, 5), (7, 7)], dropout=0.0, activation="gelu", mode="direct",
                                use_checkpoint=False).eval().to(dev)
    g = torch.Generator(device=dev).manual_seed(B + N)
    T = L + S + windows - 1
    t = torch.arange(T, dtype=torch.float32, device=dev).view(T, 1)
    table = torch.poisson(2.0 + torch.sin(2 * torch.pi * t / 7.0) + torch.rand(T, series, generator=g, device=dev),
                          generator=g)
    valid = (torch.rand(T, series, generator=g, device=dev) >= 0.2).float()
    win = ftn.windows.DeviceWindows(table, L, S, valid_mask=valid, batch_size=B, layout=layout, shuffle=True,
                                    drop_last=True, seed=1)
    with torch.no_grad():
        model(win.batch(0, epoch=0)[0][:2])                     # lazy build, on the device
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g, device=dev))
    return model, win


def uncached_step(ftn, dev, shape, iters, reps):
    """(b) alone: what a child process in the parent's tree runs."""
    fit = ftn.fit
    model, win = build(ftn, dev, shape)
    opt = fit.DeviceAdamW(fit._refit_params(model), lr=LR, weight_decay=WD, max_norm=CLIP)
    step = fit.GraphedRefitStep(model, win.batch(0, epoch=0)[:3], opt, use_loss_mask=True)

    def run(n):
        for _ in range(n):
            step.replay()

    return rounds({"uncached": run}, iters, 3, reps)["uncached"]


def shape_row(ftn, dev, shape, args):
    fit, rt = ftn.fit, ftn.runtime
    name, B, L, D, S, N, layout, series, windows = shape
    model, win = build(ftn, dev, shape)
    twin = copy.deepcopy(model)
    nb = -(-win.n_items // B)

    def fill(n):
        for _ in range(n):
            fit.OutputCache(model, win, use_loss_mask=True)

    t_fill = rounds({"fill": fill}, 1, 1, args.rounds)["fill"]
    cache = fit.OutputCache(model, win, use_loss_mask=True)
    opt = fit.DeviceAdamW(fit._refit_params(model), lr=LR, weight_decay=WD, max_norm=CLIP)
    cached = fit.GraphedCachedStep(cache, model, opt, B)
    cached.rows.copy_(win.order(0)[:B])
    opt2 = fit.DeviceAdamW(fit._refit_params(twin), lr=LR, weight_decay=WD, max_norm=CLIP)
    plain = fit.GraphedRefitStep(twin, win.batch(0, epoch=0)[:3], opt2, use_loss_mask=True)

    def a(n):
        for _ in range(n):
            cached.replay()

    def b(n):
        for _ in range(n):
            plain.replay()

    t = rounds({"cached": a, "uncached": b}, args.iters, 3, args.rounds)
    where = "same tree (GraphedRefitStep is untouched by this change)"
    if args.parent_tree:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child", name, "--iters", str(args.iters), "--rounds",
               str(args.rounds), "--tree", args.parent_tree]
        env = dict(os.environ)
        if "FLOWTIMES_LIB" in env:                              # a pinned library here: the parent's own there
            env["FLOWTIMES_LIB"] = str(Path(args.parent_tree) / "flow-timesnet_amd" / "csrc" / "libflowtimes_hip.so")
        got = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=600, env=env)
        if got.returncode == 0:
            t["uncached_same_tree"] = t["uncached"]
            t["uncached"] = json.loads(got.stdout.strip().splitlines()[-1])
            where = "the parent's tree and library, in a child process"
    # (d) on one batch of the store
    store = cache.seq[:B].contiguous()
    ident = torch.arange(B, dtype=torch.int64, device=dev)
    wt, bt = model.forecast_time_proj.weight.detach()[-S:], model.forecast_time_proj.bias.detach()[-S:]
    dh = torch.randn(B, S, D, device=dev)
    dw, db = torch.empty(S, L, device=dev), torch.empty(S, device=dev)

    def call(fn, *a_, **kw):
        def run(n):
            for _ in range(n):
                fn(*a_, **kw)
        return run

    d = rounds({"forward": call(rt.timeproj_forward, store, wt, bt),
                "forward_rows": call(rt.timeproj_forward, store, wt, bt, rows=ident),
                "backward": call(rt.timeproj_backward, store, dh, dw=dw, db=db),
                "backward_rows": call(rt.timeproj_backward, store, dh, dw=dw, db=db, rows=ident)},
               args.kernel_iters, 10, args.rounds)
    gain = t["uncached"]["us"] - t["cached"]["us"]
    fill_per_batch = t_fill["us"] / nb
    row = {"shape": name, "x": [B, L, N], "d_model": D, "steps": S, "layout": layout, "items": win.n_items,
           "batches": nb, "cache_bytes": cache.nbytes, "iters": args.iters,
           "a_cached_step": t["cached"], "b_uncached_step": t["uncached"], "b_ran_in": where,
           "b_uncached_step_same_tree": t.get("uncached_same_tree"),
           "uncached_over_cached": t["uncached"]["us"] / t["cached"]["us"],
           "c_fill": {"us_per_batch": fill_per_batch, "all_us": t_fill["all"], "spread_us": t_fill["spread"],
                      "epochs_to_break_even": math.floor(fill_per_batch / gain) + 1 if gain > 0 else None},
           "d_identity_map": d, "kernel_iters": args.kernel_iters,
           "flagged_steps": int((opt.history()[:, 3] != 0).sum())}
    print(json.dumps(row), flush=True)
    return row


def error_file(ftn, dev, path: Path) -> None:
    """The tiny model of the tests (L 24, H 4, d_model 16): six tensors after 3 shuffled epochs, cached against
    ``refit_output`` with the same ``DeviceAdamW`` settings on the same orders."""
    fit = ftn.fit
    out = {"what": "max |cached - refit_output| over each of the six tensors after 3 shuffled epochs of batch 4 over "
                   "13 items (lr 1e-2), beside max |p| and the distance either run moved the tensor",
           "device": torch.cuda.get_device_name(0), "cases": {}}
    for N, layout in ((1, "series"), (5, "wide")):
        g = torch.Generator().manual_seed(21 + N)
        T, L, H = 40, 24, 4
        t = torch.arange(T, dtype=torch.float32).view(T, 1)
        table = torch.poisson(2.0 + torch.sin(2 * torch.pi * t / 6.0) + torch.rand(T, N, generator=g), generator=g)
        win = ftn.windows.DeviceWindows(table.to(dev), L, H, batch_size=4, layout=layout, shuffle=True, drop_last=True,
                                        seed=7)
        torch.manual_seed(0)
        model = ftn.models.TimesNet(input_len=L, pred_len=H, d_model=16, d_ff=32, n_layers=2, k_periods=3,
                                    kernel_set=[(3, 3), (5, 5)], dropout=0.0, activation="gelu", mode="direct",
                                    use_checkpoint=False).eval().to(dev)
        with torch.no_grad():
            model(win.batch(0, epoch=0)[0])
            for p in model.parameters():
                if float(p.abs().sum()) == 0.0:
                    p.copy_(0.1 * torch.randn(p.shape, generator=g).to(dev))
        twin = copy.deepcopy(model)
        start = [p.detach().clone() for p in fit._refit_params(model)]
        win.set_epoch(0)
        fit.refit_output_cached(model, win, epochs=3, lr=1e-2)
        win.set_epoch(0)
        fit.refit_output(twin, win, epochs=3, optimizer=fit.DeviceAdamW(fit._refit_params(twin), lr=1e-2))
        names = ("mu_head.weight", "mu_head.bias", "sigma_head.weight", "sigma_head.bias",
                 "forecast_time_proj.weight", "forecast_time_proj.bias")
        out["cases"][f"N={N} ({layout})"] = {
            n: {"distance": float((a - b).abs().max()), "max_abs_p": float(b.abs().max()),
                "moved": float((b - s).abs().max())}
            for n, a, b, s in zip(names, (p.detach() for p in fit._refit_params(model)),
                                  (p.detach() for p in fit._refit_params(twin)), start)}
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["cases"]), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "refit_cache_time.json"))
    ap.add_argument("--error-out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=str(ROOT), help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    import __graft_entry__ as ge

    ftn = ge.load_package()
    dev = torch.device("cuda:0")
    if args.child:
        shape = next(s for s in SHAPES if s[0] == args.child)
        print(json.dumps(uncached_step(ftn, dev, shape, args.iters, args.rounds)), flush=True)
        return
    out = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "shapes": [shape_row(ftn, dev, s, args) for s in SHAPES]}
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    if args.error_out:
        error_file(ftn, dev, Path(args.error_out))


if __name__ == "__main__":
    main()
