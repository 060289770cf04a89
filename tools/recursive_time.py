#!/usr/bin/env python3
"""Recursive forecast, four ways, at two shapes.

    python tools/recursive_time.py [--out profiles/r04_recursive_time.json] [--repeats 5] [--shapes bench,c4_shard]

Per shape, one ``TimesNet(mode="recursive")`` with randomised (non-zero) heads and context, and four ways to run the
same H-step forecast:

  loop_eager      the reference's ``forecast_recursive_batch`` host loop over the eager model
  loop_graphed    the same loop, each step one ``graph.GraphedForward`` replay (window copied into its input)
  device          ``forecast.forecast_recursive_batch`` on the device path (ring of embedded rows, no host sync)
  replay          ``forecast.RecursiveForecaster``: the whole forecast as one HIP graph

Each number is device events around one whole forecast, after warm-up, ``--repeats`` forecasts per variant; the
JSON keeps every forecast, the table prints the median.  The four outputs are compared with ``torch.equal``."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
# name: B, L, N, d_model, d_ff, H
SHAPES = {"bench": (256, 336, 512, 64, 256, 24), "c4_shard": (64, 720, 4096, 128, 512, 96)}


def _model(pkg, dev, B, L, N, D, d_ff):
    import torch

    torch.manual_seed(0)
    model = pkg.models.TimesNet(input_len=L, pred_len=1, d_model=D, d_ff=d_ff, n_layers=3, k_periods=5,
                                kernel_set=[(3, 3), (5, 5), (7, 7)], dropout=0.0, activation="gelu",
                                mode="recursive", bottleneck_ratio=4.0, use_checkpoint=True, id_embed_dim=32,
                                use_zero_mean_context=True, context_rank=16).eval().to(dev)
    x = torch.from_numpy(pkg.synth.make_input(B, L, N, seed=7)).to(dev)
    x = x - x.amin() + 1.0                                      # positive, like the sales series it forecasts
    ids = torch.arange(N, device=dev)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        model(x[:2], series_ids=ids)                            # lazy build, on the device
        for p in model.parameters():
            if float(p.detach().abs().sum()) == 0.0:
                p.copy_(0.05 * torch.randn(p.shape, generator=g).to(p.device))
    return model, x, ids


def _time(fn, repeats):
    import torch

    fn()
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def run_shape(pkg, name, repeats):
    import torch

    B, L, N, D, d_ff, H = SHAPES[name]
    dev = torch.device("cuda:0")
    F = pkg.forecast
    model, x, ids = _model(pkg, dev, B, L, N, D, d_ff)
    res = {"B": B, "L": L, "N": N, "d_model": D, "d_ff": d_ff, "H": H, "n_layers": 3, "k_periods": 5,
           "context_rank": 16}
    outs = {}
    with torch.inference_mode():
        def loop_eager():
            outs["loop_eager"] = F.forecast_recursive_batch_loop(model, x, H, series_ids=ids)

        gf = pkg.graph.GraphedForward(model, x, series_ids=ids)

        def loop_graphed():
            rates, disps, seq = [], [], x
            for _ in range(H):
                r, d = gf(seq, series_ids=ids)
                rates.append(r.clone())
                disps.append(d.clone())
                seq = torch.cat([seq[:, 1:, :], rates[-1]], dim=1)
            outs["loop_graphed"] = (torch.cat(rates, 1), torch.cat(disps, 1))

        def device():
            outs["device"] = F.forecast_recursive_batch(model, x, H, series_ids=ids)

        fc = F.RecursiveForecaster(model, x, H, series_ids=ids)

        def replay():
            outs["replay"] = fc(x)

        times = {}
        for key, fn in (("loop_eager", loop_eager), ("loop_graphed", loop_graphed), ("device", device),
                        ("replay", replay)):
            times[key] = _time(fn, repeats)
            print(f"  {name} {key:13s} median {statistics.median(times[key]):9.3f} ms", flush=True)
    want = outs["loop_eager"]
    res["outputs_equal"] = {k: bool(torch.equal(v[0], want[0]) and torch.equal(v[1], want[1]))
                            for k, v in outs.items()}
    res["ms_per_forecast"] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
                              for k, v in times.items()}
    res["ms_per_step"] = {k: statistics.median(v) / H for k, v in times.items()}
    med = {k: statistics.median(v) for k, v in times.items()}
    res["saving_vs_loop_eager"] = {k: 1.0 - med[k] / med["loop_eager"] for k in ("device", "replay")}
    res["saving_vs_loop_graphed"] = {k: 1.0 - med[k] / med["loop_graphed"] for k in ("device", "replay")}
    res["periods"] = model.period_selector.last_selected_periods.tolist()
    res["engines"] = [b.engine or "default" for b in model.blocks]
    del fc, gf
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="bench,c4_shard")
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    result = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "shapes": {}}
    for name in a.shapes.split(","):
        result["shapes"][name] = run_shape(pkg, name, a.repeats)
        r = result["shapes"][name]
        print(f"{name}: equal {r['outputs_equal']}  saving vs eager loop {r['saving_vs_loop_eager']}  "
              f"vs graphed loop {r['saving_vs_loop_graphed']}", flush=True)
    text = json.dumps(result, indent=1)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    print(json.dumps({k: {kk: r[kk] for kk in ("ms_per_forecast", "outputs_equal")} for k, r in result["shapes"].items()},
                     default=lambda o: None)[:4000])


if __name__ == "__main__":
    main()
