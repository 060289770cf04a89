"""Times the refit step on the device at the three shapes of profiles/output_fit_time.json, three ways in the same run:

  (a) a replayed ``fit.GraphedRefitStep``: backbone forward, time projection, heads, loss, both backwards and
      ``ftn_refit_update`` as one graph launch
  (b) the parent's step: the body of ``fit.refit_output`` with ``torch.optim.AdamW`` and ``clip_grad_norm_``
      (``--iters`` batches per call, so its one synchronisation is shared by all of them)
  (c) the update alone: ``ftn_refit_update`` in each form it can take against ``clip_grad_norm_`` + ``AdamW.step``
      on the same six tensors, at the three layouts and at totals on both sides of the form threshold

The sides alternate round by round; device events surround ``--iters`` iterations after a warm-up; the median of
``--rounds`` rounds is kept beside all of them and their spread (max - min).  The backbone is two TimesBlocks with the
bench's kernel set.

    python tools/refit_step_time.py --out profiles/refit_step_time.json --error-out profiles/refit_step_error.json

``--error-out`` also runs tests/test_gpu_refit_step.py and records the ``REFIT_STEP`` distances of its five-step case.
"""
from __future__ import annotations

import argparse
import copy
import json
import re
import statistics
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

SHAPES = [("pipeline", 4096, 28, 64, 7, 1), ("bench", 256, 336, 64, 96, 512), ("configs[4] shard", 64, 720, 128, 96, 4096)]
LR, WD, CLIP = 1e-3, 0.01, 1.0


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


def six(m):
    return [m.mu_head.weight, m.mu_head.bias, m.sigma_head.weight, m.sigma_head.bias, m.forecast_time_proj.weight,
            m.forecast_time_proj.bias]


def step_rows(ftn, dev, args):
    fit = ftn.fit
    rows = []
    for name, B, L, D, S, N in SHAPES:
        torch.manual_seed(B + N)
        model = ftn.models.TimesNet(input_len=L, pred_len=S, d_model=D, d_ff=4 * D, n_layers=2, k_periods=3,
                                    kernel_set=[(3, 3), (5, 5), (7, 7)], dropout=0.0, activation="gelu", mode="direct",
                                    use_checkpoint=False).eval().to(dev)
        g = torch.Generator(device=dev).manual_seed(B + N)
        t = torch.arange(L, dtype=torch.float32, device=dev).view(1, L, 1)
        x = torch.rand(B, L, N, generator=g, device=dev) + 1.5 + torch.sin(2 * torch.pi * t / 7.0)
        y = torch.poisson(torch.full((B, S, N), 2.0, device=dev), generator=g)
        mask = (torch.rand(B, S, N, generator=g, device=dev) >= 0.2).float()
        batch = (x, y, mask)
        with torch.no_grad():
            model(x[:2])                                        # lazy build, on the device
            for p in model.parameters():
                if float(p.abs().sum()) == 0.0:
                    p.copy_(0.1 * torch.randn(p.shape, generator=g, device=dev))
        twin = copy.deepcopy(model)
        opt = fit.DeviceAdamW(six(model), lr=LR, weight_decay=WD, max_norm=CLIP)
        step = fit.GraphedRefitStep(model, batch, opt, use_loss_mask=True)
        adamw = torch.optim.AdamW(six(twin), lr=LR, weight_decay=WD)

        def graphed(n):
            for _ in range(n):
                step.replay()

        def parent(n):
            fit.refit_output(twin, [batch] * n, use_loss_mask=True, optimizer=adamw, grad_clip=CLIP)

        t = rounds({"graphed": graphed, "parent": parent}, args.step_iters, 3, args.rounds)
        flags = opt.history()[:, 3]
        rows.append({"shape": name, "x": [B, L, N], "d_model": D, "steps": S, "iters": args.step_iters,
                     "parameters": sum(p.numel() for p in six(model)),
                     "update_form": list(ftn.runtime.refit_update_form_of([p.numel() for p in six(model)])),
                     "graphed_step": t["graphed"], "parent_step": t["parent"],
                     "parent_over_graphed": t["parent"]["us"] / t["graphed"]["us"],
                     "flagged_steps": int((flags != 0).sum())})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def update_rows(ftn, dev, args):
    rt = ftn.runtime
    layouts = [("pipeline", [64, 1, 64, 1, 7 * 28, 7]), ("total 4096", [2048, 8, 2000, 8, 24, 8]),
               ("total 8192 (last of k_refit_one)", [4096, 8, 4056, 8, 16, 8]),
               ("total 8224 (first of the grid)", [4096, 8, 4088, 8, 16, 8]),
               ("total 16384", [8192, 8, 8152, 8, 16, 8]),
               ("total 32768", [16384, 8, 16352, 8, 8, 8]), ("total 65536", [32768, 8, 32736, 8, 8, 8]),
               ("bench", [512 * 64, 512, 512 * 64, 512, 96 * 336, 96]),
               ("configs[4] shard", [4096 * 128, 4096, 4096 * 128, 4096, 96 * 720, 96])]
    rows = []
    for name, counts in layouts:
        g = torch.Generator(device=dev).manual_seed(sum(counts))
        ps = [torch.randn(n, generator=g, device=dev).requires_grad_() for n in counts]
        gs = [0.1 * torch.randn(n, generator=g, device=dev) for n in counts]
        for p, gr in zip(ps, gs):
            p.grad = gr.clone()
        own = [p.detach().clone() for p in ps]
        ms, vs = [torch.zeros_like(p) for p in own], [torch.zeros_like(p) for p in own]
        lr, state = torch.full((1,), LR, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
        ws = torch.empty(8 * 1024 + 16, dtype=torch.uint8, device=dev)
        chunks = rt.refit_update_form_of(counts)[2]

        def ours(form):
            def run(n):
                for _ in range(n):
                    rt.refit_update(own, gs, ms, vs, lr, state, weight_decay=WD, max_norm=CLIP, workspace=ws,
                                    force_form=form)
            return run

        def torch_side(foreach):
            opt = torch.optim.AdamW(ps, lr=LR, weight_decay=WD, foreach=foreach)

            def run(n):
                for _ in range(n):
                    for p, gr in zip(ps, gs):
                        p.grad.copy_(gr)                        # the clip scales the gradient in memory
                    torch.nn.utils.clip_grad_norm_(ps, CLIP, foreach=foreach)
                    opt.step()
            return run

        def grad_copies(n):
            for _ in range(n):
                for p, gr in zip(ps, gs):
                    p.grad.copy_(gr)

        fns = {"grid": ours("grid"), "torch": torch_side(None), "torch_single_tensor": torch_side(False),
               "torch_side_gradient_copies": grad_copies}
        if chunks <= 64:
            fns["one"] = ours("one")
        t = rounds(fns, args.iters, 10, args.rounds)
        rows.append({"layout": name, "counts": counts, "total": sum(counts), "chunks": chunks,
                     "form": rt.refit_update_form_of(counts)[0], "iters": args.iters,
                     "k_refit_one": t.get("one"), "k_refit_norm+k_refit_apply": t["grid"],
                     "torch_clip_adamw": t["torch"], "torch_clip_adamw_foreach_false": t["torch_single_tensor"],
                     "torch_side_gradient_copies": t["torch_side_gradient_copies"]})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def error_file(path: Path) -> None:
    cmd = [sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", "-m", "gpu",
           str(ROOT / "tests" / "test_gpu_refit_step.py")]
    text = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    out = {"bound": "graphed <= 4 d_ref + 5 2^-23 max|p|, distances to the fp64-master run after five steps",
           "device": torch.cuda.get_device_name(0), "five_steps": {}}
    for m in re.finditer(r"REFIT_STEP (N=\d+): .*? run ([\d.e+-]+), the parent's fp32 loop to it ([\d.e+-]+), "
                         r"max\|p\| ([\d.e+-]+)", text):
        out["five_steps"][m[1]] = {"graphed": float(m[2]), "d_ref": float(m[3]), "max_abs_p": float(m[4])}
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(text[-1500:])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "refit_step_time.json"))
    ap.add_argument("--error-out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("update", "step"), default=None)
    args = ap.parse_args()
    ftn = ge.load_package()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName}
    if args.only != "step":
        out["update_alone"] = update_rows(ftn, dev, args)
    if args.only != "update":
        out["step"] = step_rows(ftn, dev, args)
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    if args.error_out:
        error_file(Path(args.error_out))


if __name__ == "__main__":
    main()
