"""Times one refit step of the heads on the device, forward plus backward, two ways in the same run:

  (a) ``fit.head_nll``: ``ftn_head_fit_forward``, ``ftn_nb_nll_grad`` and ``ftn_head_backward``
  (b) the same heads under ``score._nll_torch``, the reference's fp32 formula under autograd - what a head parameter
      that requires grad gets without ``fit``

the loss node alone, ``fit.negative_binomial_nll`` against ``score._nll_torch`` on given rate and dispersion, and the
head forward and the head backward (no ``d_hidden``) alone.
The two sides alternate round by round; device events surround ``--iters`` iterations after a warm-up; the median of 3
rounds is kept.  Shapes: hidden [B, S, D] and N series - the pipeline layout, the bench shape and a configs[4] shard.

    python tools/head_fit_time.py --out profiles/head_fit_time.json
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

SHAPES = [("pipeline", 4096, 7, 64, 1), ("bench", 256, 96, 64, 512), ("configs[4] shard", 64, 96, 128, 4096)]


def rounds(fns, iters, warm, reps=3):
    """us per iteration of every function, alternated round by round: ``{name: (median, all)}``."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: (statistics.median(v), v) for k, v in out.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "head_fit_time.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    ftn = ge.load_package()
    fit, sc, rt = ftn.fit, ftn.score, ftn.runtime
    dev = torch.device("cuda:0")
    rows = []
    for name, B, S, D, N in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B + N)
        hidden = torch.randn(B, S, D, generator=g, device=dev)
        heads = [(0.1 * torch.randn(shape, generator=g, device=dev)).requires_grad_()
                 for shape in ((N, D), (N,), (N, D), (N,))]
        tail = torch.rand(B, S, N, generator=g, device=dev) + 1.0
        y = torch.poisson(torch.full((B, S, N), 2.0, device=dev), generator=g)
        mask = torch.rand(B, S, N, generator=g, device=dev) >= 0.2

        def step_fit():
            loss, _ = fit.head_nll(hidden, *heads, tail, S, y, mask)
            torch.autograd.grad(loss, heads)

        def step_torch():
            rate, disp, _ = fit._heads_torch(hidden, *heads, tail, S, None, None, 1e-3)
            torch.autograd.grad(sc._nll_torch(y, rate, disp, mask, 1e-8), heads)

        with torch.no_grad():
            rate0, disp0, _ = fit._heads_torch(hidden, *heads, tail, S, None, None, 1e-3)
        rate0, disp0 = rate0.requires_grad_(), disp0.requires_grad_()

        def loss_fit():
            torch.autograd.grad(fit.negative_binomial_nll(y, rate0, disp0, mask), (rate0, disp0))

        def loss_torch():
            torch.autograd.grad(sc._nll_torch(y, rate0, disp0, mask, 1e-8), (rate0, disp0))

        with torch.no_grad():
            raw = [t.detach() for t in heads]
            _, _, sig_mu, sig_sg, _ = rt.head_fit_forward(hidden, *raw, tail, S, None, None, 1e-3)
            words, g_rate, g_disp = rt.nb_nll_grad(y, rate0.detach(), disp0.detach(), mask, scaled=False)

        def k_forward():
            rt.head_fit_forward(hidden, *raw, tail, S, None, None, 1e-3)

        def k_backward():
            rt.head_backward(hidden, g_rate, g_disp, sig_mu, sig_sg, words[1:2])

        t = rounds({"head_nll": step_fit, "torch": step_torch, "loss_fit": loss_fit, "loss_torch": loss_torch,
                    "k_forward": k_forward, "k_backward": k_backward}, args.iters, args.warmup)
        rows.append({"shape": name, "hidden": [B, S, D], "N": N, "iters": args.iters,
                     "form": list(rt.nb_nll_grad_form(y, rate0.detach(), disp0.detach(), mask)),
                     "backward_form": list(rt.head_backward_form_of(B * S, N, D)),
                     "head_fit_forward_us": t["k_forward"][0], "head_backward_us": t["k_backward"][0],
                     "head_nll_us": t["head_nll"][0], "head_nll_us_all": t["head_nll"][1],
                     "torch_autograd_us": t["torch"][0], "torch_autograd_us_all": t["torch"][1],
                     "step_speedup": t["torch"][0] / t["head_nll"][0],
                     "loss_node_us": t["loss_fit"][0], "loss_node_us_all": t["loss_fit"][1],
                     "loss_torch_autograd_us": t["loss_torch"][0], "loss_torch_autograd_us_all": t["loss_torch"][1],
                     "loss_speedup": t["loss_torch"][0] / t["loss_fit"][0]})
        print(json.dumps(rows[-1]))
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0),
                                          "arch": torch.cuda.get_device_properties(0).gcnArchName, "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
