#!/usr/bin/env python3
"""The time projection, ``ftn_timeproj_forward`` against ``torch.baddbmm``, in one process on the same tensors.

    python tools/timeproj_time.py [--out profiles/r05_timeproj_time.json] [--launches 300] [--warmup 40]

Per shape the two calls are issued alternately (A, B, A, B, ...), each launch between its own pair of device events;
the figure is the median over ``--launches`` launches of each after ``--warmup`` alternations.  ``baddbmm`` is issued
the way ``TimesNet._heads`` issued it before the HIP kernel took its place.  A second figure, ``back_to_back_us``, is
for information: 20 launches of one kind between one pair of events, per launch - it leaves out the idle time a
single short launch spends waiting for the host.  Also reported: the bytes of ``seq`` per second of the median, the
kernel form, and whether the two results agree to the shell's tolerance.  Exit status 1 when a shape's median is above
``baddbmm``'s."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
# name: B, L, S, D
SHAPES = {"bench": (256, 336, 96, 64), "c4_shard": (64, 720, 96, 128), "recursive": (256, 336, 1, 64)}


def run_shape(pkg, name, launches, warmup):
    import torch

    rt = pkg.runtime
    B, L, S, D = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    seq = torch.randn(B, L, D, generator=g).to(dev)
    weight = (torch.randn(96, L, generator=g) / L ** 0.5).to(dev)
    bias = torch.randn(96, generator=g).to(dev)
    wt, bt = (weight, bias) if S == 96 else (weight[-S:], bias[-S:])      # the recursive model's row slice

    def ours():
        return rt.timeproj_forward(seq, wt, bt)

    def blas():
        return torch.baddbmm(bt.view(1, -1, 1), wt.unsqueeze(0).expand(B, -1, -1), seq)

    calls = {"timeproj": ours, "baddbmm": blas}
    with torch.inference_mode():
        diff = float((ours() - blas()).abs().max())
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
        burst = {k: [] for k in calls}
        for _ in range(max(10, launches // 20)):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    fn()
                e1.record()
                burst[k].append((e0, e1))
        torch.cuda.synchronize()
        burst = {k: [1e3 * a.elapsed_time(b) / 20 for a, b in v] for k, v in burst.items()}
    med = {k: statistics.median(v) for k, v in single.items()}
    seq_bytes = B * L * D * 4
    return {"B": B, "L": L, "S": S, "D": D, "form": rt.timeproj_form(seq, wt), "launches": launches, "warmup": warmup,
            "median_us": med, "min_us": {k: min(v) for k, v in single.items()},
            "back_to_back_us": {k: statistics.median(v) for k, v in burst.items()},
            "seq_bytes": seq_bytes, "seq_read_GBps": {k: seq_bytes / (v * 1e-6) / 1e9 for k, v in med.items()},
            "max_abs_diff": diff, "not_slower": med["timeproj"] <= med["baddbmm"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    if a.launches < 200 or a.warmup < 30:
        ap.error("at least 200 launches and 30 warm-ups")
    sys.path.insert(0, str(ROOT))
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    result = {"device": torch.cuda.get_device_name(0), "method": "device events per launch, A/B interleaved, median",
              "shapes": {}}
    for name in a.shapes.split(","):
        r = result["shapes"][name] = run_shape(pkg, name, a.launches, a.warmup)
        print(f"{name:10s} {r['form']:24s} timeproj {r['median_us']['timeproj']:8.2f} us   baddbmm "
              f"{r['median_us']['baddbmm']:8.2f} us   (back to back {r['back_to_back_us']['timeproj']:.2f} / "
              f"{r['back_to_back_us']['baddbmm']:.2f})   seq read {r['seq_read_GBps']['timeproj']:.0f} GB/s")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    return 0 if all(r["not_slower"] for r in result["shapes"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
