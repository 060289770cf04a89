#!/usr/bin/env python3
"""The wide model shell (128 < d_model <= 512) beside the torch ops the shell ran in its place before, and the graphed
whole-model forward with and without it.

    python tools/shell_wide_time.py [--out profiles/shell_wide_time.json] [--launches 200] [--warmup 30]

Kernels: one process, the same tensors, the two calls issued alternately (A, B, A, B, ...), each launch between its
own pair of device events; the figure is the median over ``--launches`` launches of each after ``--warmup``
alternations (the method of ``tools/timeproj_time.py``).  Per entry point: the wide kernel against ``F.linear`` + add
(+ ``layer_norm``) for the embedding, ``baddbmm`` for the time projection and the torch expression of
``TimesNet._rate_dispersion`` for the heads (without its finite-positive check, which synchronises with the host).
Also reported: the bytes of the main operand per second of the median and the kernel form.

Whole model: a d_model 256 TimesNet in a fresh child process per configuration because ``FTN_SHELL_WIDE`` is read once:
switch off, feature on, switch off again - the two "off" runs show the run-to-run spread the comparison has to be read
against.  The eager forward is timed in every configuration (device events around the call, median); the
``graph.GraphedForward`` replay only with the feature on: with the switch off the torch heads read the device for their
finite-positive check, and such a forward cannot be captured at all."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
# name: B, L, N, H, D
SHAPES = {"bench_wide": (256, 336, 512, 96, 256), "pipeline": (4096, 28, 1, 7, 256)}
MODEL = dict(B=64, L=336, N=512, H=96, d_model=256, d_ff=256, n_layers=2)


def _ab(calls, launches, warmup):
    import torch

    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    events = {k: [] for k in calls}
    for _ in range(launches):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    single = {k: [1e3 * a.elapsed_time(b) for a, b in v] for k, v in events.items()}
    return {k: statistics.median(v) for k, v in single.items()}, {k: min(v) for k, v in single.items()}


def run_shape(pkg, name, launches, warmup):
    import torch
    import torch.nn.functional as F

    rt = pkg.runtime
    B, L, N, H, D = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g)
    x = (r(B, L, N).abs() + 0.5).to(dev)
    w, add = (r(D, N) / N ** 0.5).to(dev), r(1, L, D).to(dev)
    ln = ((torch.rand(D, generator=g) + 0.5).to(dev), r(D).to(dev), 1e-5)
    seq = r(B, L, D).to(dev)
    wt, bt = (r(H, L) / L ** 0.5).to(dev), r(H).to(dev)
    hidden = r(B, H, D).to(dev)
    w_mu, w_sg, b_mu, b_sg = (0.05 * r(N, D)).to(dev), (0.05 * r(N, D)).to(dev), r(N).to(dev), r(N).to(dev)
    hist = min(H, L)
    tail = x[:, -hist:, :]

    def torch_heads():
        pre = F.linear(hidden, w_mu, b_mu) + tail
        rate = F.softplus(pre, beta=1.0, threshold=20) + 1e-6
        spread = F.softplus(F.linear(hidden, w_sg, b_sg), beta=1.0, threshold=20)
        return rate, spread + torch.full_like(rate, 1e-3) + 1e-6

    pairs = {
        "embed": (lambda: rt.embed_forward(x, w, add, None), lambda: F.linear(x, w) + add, rt.embed_form(x, w), x.numel() * 4),
        "embed_layernorm": (lambda: rt.embed_forward(x, w, add, ln),
                            lambda: F.layer_norm(F.linear(x, w) + add, (D,), ln[0], ln[1], ln[2]), rt.embed_form(x, w),
                            x.numel() * 4),
        "timeproj": (lambda: rt.timeproj_forward(seq, wt, bt),
                     lambda: torch.baddbmm(bt.view(1, -1, 1), wt.unsqueeze(0).expand(B, -1, -1), seq),
                     rt.timeproj_form(seq, wt), seq.numel() * 4),
        "heads": (lambda: rt.head_forward(hidden, w_mu, b_mu, w_sg, b_sg, tail, hist, None, None, 1e-3), torch_heads,
                  rt.head_form(hidden, w_mu, tail)[0], hidden.numel() * 4 + 2 * B * H * N * 4),
    }
    out = {"B": B, "L": L, "N": N, "H": H, "D": D, "launches": launches, "warmup": warmup, "entries": {}}
    with torch.inference_mode():
        for entry, (ours, theirs, form, nbytes) in pairs.items():
            a, b = ours(), theirs()
            a, b = (a[0], b[0]) if isinstance(b, tuple) else (a, b)
            diff = float((a - b).abs().max())
            del a, b
            med, lo = _ab({"hip": ours, "torch": theirs}, launches, warmup)
            out["entries"][entry] = {"form": form, "median_us": med, "min_us": lo, "bytes": nbytes,
                                     "GBps": {k: nbytes / (v * 1e-6) / 1e9 for k, v in med.items()},
                                     "max_abs_diff": diff, "not_slower": med["hip"] <= med["torch"]}
            print(f"{name:10s} {entry:16s} {form:24s} hip {med['hip']:9.2f} us   torch {med['torch']:9.2f} us   "
                  f"{out['entries'][entry]['GBps']['hip']:.0f} GB/s")
    return out


def model_child(replays, warmup):
    """One configuration of the whole-model run (this process's FTN_SHELL_WIDE): prints one JSON line."""
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    m, dev = MODEL, torch.device("cuda:0")
    torch.manual_seed(0)
    net = pkg.models.TimesNet(input_len=m["L"], pred_len=m["H"], d_model=m["d_model"], d_ff=m["d_ff"],
                              n_layers=m["n_layers"], k_periods=3, kernel_set=[(3, 3), (5, 5)], dropout=0.0,
                              activation="gelu", mode="direct", use_checkpoint=False).eval().to(dev)
    g = torch.Generator().manual_seed(1)
    t = torch.arange(m["L"], dtype=torch.float32).view(1, -1, 1)
    x = (torch.rand(m["B"], m["L"], m["N"], generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 24.0)).to(dev)
    with torch.inference_mode():
        net(x)
        for p in net.parameters():
            if float(p.detach().abs().sum()) == 0.0:
                p.copy_((0.05 * torch.randn(p.shape, generator=g)).to(dev))
        net(x)
    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ev = []
        for _ in range(replays):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        times = [1e3 * a.elapsed_time(b) for a, b in ev]
        return {"median_us": statistics.median(times), "min_us": min(times)}

    wide = os.environ.get("FTN_SHELL_WIDE", "1") != "0"
    with torch.inference_mode():
        eager = timed(lambda: net(x))
    backends = [net._last_embed_backend, net._last_timeproj_backend, net._last_head_backend]
    # the torch heads read the device for their finite-positive check: such a forward cannot be captured
    graphed = None
    if wide:
        gf = pkg.graph.GraphedForward(net, x)
        graphed = timed(lambda: gf(x))
    print(json.dumps({"shell_wide": "1" if wide else "0", "eager": eager, "graphed": graphed, "replays": replays,
                      "backends": backends}))


def run_model(replays, warmup):
    runs = []
    for value in ("0", "1", "0"):
        env = dict(os.environ, FTN_SHELL_WIDE=value)
        r = subprocess.run([sys.executable, __file__, "--model-child", "--launches", str(replays), "--warmup", str(warmup)],
                           env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"whole-model run (FTN_SHELL_WIDE={value}) failed:\n{r.stderr[-2000:]}")
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(f"model      FTN_SHELL_WIDE={value}  eager {runs[-1]['eager']['median_us']:10.1f} us   graphed "
              f"{runs[-1]['graphed'] and runs[-1]['graphed']['median_us']}   shell {runs[-1]['backends']}")
    off = [r["eager"]["median_us"] for r in runs if r["shell_wide"] == "0"]
    on = [r["eager"]["median_us"] for r in runs if r["shell_wide"] == "1"][0]
    spread = abs(off[0] - off[1])
    return {"config": MODEL, "runs": runs, "spread_us": spread, "on_minus_slower_off_us": on - max(off),
            "not_slower_beyond_spread": on <= max(off) + spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--model-replays", type=int, default=60)
    ap.add_argument("--model-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    if a.model_child:
        model_child(a.launches, a.warmup)
        return 0
    model = run_model(a.model_replays, 10) if a.model_replays > 0 else None      # children first: one process at a time
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    result = {"device": torch.cuda.get_device_name(0), "method": "device events per launch, A/B interleaved, median",
              "shapes": {}, "model": model}
    for name in a.shapes.split(","):
        result["shapes"][name] = run_shape(pkg, name, a.launches, a.warmup)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    return 0 if model is None or model["not_slower_beyond_spread"] else 1


if __name__ == "__main__":
    sys.exit(main())
