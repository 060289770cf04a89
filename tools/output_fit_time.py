"""Times one refit step of the whole output side on the device, forward plus backward, two ways in the same run:

  (a) ``fit.output_nll``: ``ftn_timeproj_forward``, the head kernels of ``fit.head_nll`` and, backward,
      ``ftn_head_backward`` (with ``d_hidden``) and ``ftn_timeproj_backward``
  (b) ``torch.matmul(wt, seq) + bt`` under autograd feeding the same ``fit.head_nll`` - what the step costs without
      the time projection's own node (the library GEMM forward and twice backward)

and ``ftn_timeproj_backward`` alone with the bytes of ``seq`` and ``d_hidden`` it reads per second.  The two sides
alternate round by round; device events surround ``--iters`` iterations after a warm-up; the median of 3 rounds is
kept.  Shapes: seq [B, L, D] -> S steps and N series - the pipeline layout, the bench shape and a configs[4] shard.

    python tools/output_fit_time.py --out profiles/output_fit_time.json
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import __graft_entry__ as ge  # noqa: E402
from head_fit_time import rounds  # noqa: E402

SHAPES = [("pipeline", 4096, 28, 64, 7, 1), ("bench", 256, 336, 64, 96, 512), ("configs[4] shard", 64, 720, 128, 96, 4096)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "output_fit_time.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    ftn = ge.load_package()
    fit, rt = ftn.fit, ftn.runtime
    dev = torch.device("cuda:0")
    rows = []
    for name, B, L, D, S, N in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B + N)
        seq = torch.randn(B, L, D, generator=g, device=dev)
        wt = (torch.randn(S, L, generator=g, device=dev) / L ** 0.5).requires_grad_()
        bt = (0.1 * torch.randn(S, generator=g, device=dev)).requires_grad_()
        heads = [(0.1 * torch.randn(shape, generator=g, device=dev)).requires_grad_()
                 for shape in ((N, D), (N,), (N, D), (N,))]
        six = [wt, bt] + heads
        tail = torch.rand(B, S, N, generator=g, device=dev) + 1.0
        y = torch.poisson(torch.full((B, S, N), 2.0, device=dev), generator=g)
        mask = torch.rand(B, S, N, generator=g, device=dev) >= 0.2
        d_hidden = torch.randn(B, S, D, generator=g, device=dev)

        def step_fit():
            loss, _ = fit.output_nll(seq, *six, tail, S, y, mask)
            torch.autograd.grad(loss, six)

        def step_torch():
            loss, _ = fit.head_nll(torch.matmul(wt, seq) + bt.view(1, -1, 1), *heads, tail, S, y, mask)
            torch.autograd.grad(loss, six)

        def k_backward():
            rt.timeproj_backward(seq, d_hidden)

        def k_forward():
            rt.timeproj_forward(seq, wt.detach(), bt.detach())

        def torch_backward():                                   # the library GEMM for dW_t and the sum for db_t alone
            torch.einsum("bsd,bld->sl", d_hidden, seq)
            d_hidden.sum((0, 2))

        t = rounds({"output_nll": step_fit, "torch": step_torch, "k_backward": k_backward, "k_forward": k_forward,
                    "torch_backward": torch_backward}, args.iters, args.warmup)
        step_fit()
        assert fit._last_timeproj_backend == "hip" and fit._last_head_backend == "hip"
        nbytes = 4 * (seq.numel() + d_hidden.numel())
        rows.append({"shape": name, "seq": [B, L, D], "S": S, "N": N, "iters": args.iters,
                     "backward_form": list(rt.timeproj_backward_form_of(B, L, S, D)),
                     "timeproj_backward_us": t["k_backward"][0], "timeproj_backward_us_all": t["k_backward"][1],
                     "timeproj_backward_GBps_of_seq_and_dH": nbytes / t["k_backward"][0] * 1e-3,
                     "torch_einsum_backward_us": t["torch_backward"][0],
                     "timeproj_forward_us": t["k_forward"][0],
                     "output_nll_us": t["output_nll"][0], "output_nll_us_all": t["output_nll"][1],
                     "torch_matmul_autograd_us": t["torch"][0], "torch_matmul_autograd_us_all": t["torch"][1],
                     "step_speedup": t["torch"][0] / t["output_nll"][0]})
        print(json.dumps(rows[-1]))
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0),
                                          "arch": torch.cuda.get_device_properties(0).gcnArchName, "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
