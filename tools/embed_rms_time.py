#!/usr/bin/env python3
"""``embed_norm_mode="rms"`` on the HIP path beside ``"layer"``, and beside what an "rms" model ran before the
embedding kernels took the mode (the torch composition and the host loop).

    python tools/embed_rms_time.py [--out profiles/embed_rms_time.json] [--launches 200] [--warmup 30]
                                   [--parent-root DIR [--parent-lib SO]]

Embedding launch alone: one process, the same window, weight and ``add``, ``runtime.embed_forward`` with the RMS norm
and with LayerNorm issued alternately (A, B, A, B, ...), each between its own pair of device events, eager and as
one-launch graphs; the figure is the median over ``--launches`` of each after ``--warmup`` alternations (the method of
``tools/context_time.py``).  The RMS epilogue does strictly less than LayerNorm's, so it should be no slower beyond the
pool's +-4 % box spread; the result records where it is.

Whole forward: ``graph.GraphedForward`` replays of an "rms" model and a "layer" model that differ in nothing else,
alternated in one process.

Recursive forecast: H = 28 steps of an "rms" model, ``forecast_recursive_batch`` (device path: ring, no host
synchronisation per step) against ``forecast_recursive_batch_loop`` (what the mode fell to before), wall time around a
device synchronisation, alternated.

Parent commit: with ``--parent-root`` (a checkout of the parent commit; ``--parent-lib`` its built library, otherwise
it builds its own on first use) the "rms" graphed forward runs in fresh child processes - parent, this tree, parent -
so the torch composition the parent runs for this mode is measured by the parent's own code on the same box; the two
parent runs show the run-to-run spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
# name: B, L, N, H, d_model, per-sample context
SHAPES = {"bench": (256, 336, 512, 96, 64, False), "pipeline_d64": (4096, 28, 1, 7, 64, True),
          "pipeline_d256": (4096, 28, 1, 7, 256, True)}
F_STATIC, STATIC_DIM, ID_DIM, RANK, TIME_DIM = 8, 16, 32, 8, 4
BOX_SPREAD = 0.04


def build(pkg, name, norm, mode="direct", n_layers=2):
    """The model of a shape with the whole context front end in this norm mode, and its inputs on the device."""
    import torch

    B, L, N, H, D, per_sample = SHAPES[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = pkg.models.TimesNet(input_len=L, pred_len=H, d_model=D, d_ff=D, n_layers=n_layers, k_periods=3,
                              kernel_set=[(3, 3), (5, 5)], dropout=0.0, activation="gelu", mode=mode,
                              use_checkpoint=False, embed_norm_mode=norm, id_embed_dim=ID_DIM,
                              static_proj_dim=STATIC_DIM, use_zero_mean_context=True, context_rank=RANK,
                              use_constant_context_bias=True, use_late_bias_head=True).eval()
    g = torch.Generator().manual_seed(1)
    t = torch.arange(L, dtype=torch.float32).view(1, -1, 1)
    x = (torch.rand(B, L, N, generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 7.0)).to(dev)
    if per_sample:
        kw = dict(series_static=torch.randn(B, N, F_STATIC, generator=g).to(dev),
                  series_ids=torch.randint(0, 3000, (B, N), generator=g).to(dev))
        kw["series_ids"][0, 0] = 2999                                              # the vocabulary the table is built for
    else:
        kw = dict(series_static=torch.randn(N, F_STATIC, generator=g).to(dev), series_ids=torch.arange(N, device=dev))
    with torch.inference_mode():
        net(x, **kw)
        for p in net.parameters():                              # wake the zero-initialised heads / context maps
            if float(p.detach().abs().sum()) == 0.0:
                p.copy_((0.05 * torch.randn(p.shape, generator=g)).to(dev))
        net(x, **kw)
    return net, x, kw


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
    return {k: {"median_us": statistics.median(v), "min_us": min(v)} for k, v in single.items()}


def run_embed(pkg, name, launches, warmup):
    """``embed_forward`` alone at this layout: the same operands, the RMS norm against LayerNorm."""
    import torch

    rt = pkg.runtime
    B, L, N, _, D, _ = SHAPES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, L, N, generator=g).to(dev)
    w = (torch.randn(D, N, generator=g) / N ** 0.5).to(dev)
    add = torch.randn(1, L, D, generator=g).to(dev)
    gamma, beta = (torch.rand(D, generator=g) + 0.5).to(dev), torch.randn(D, generator=g).to(dev)
    norms = {"rms": (gamma, beta, 1e-5, "rms"), "layer": (gamma, beta, 1e-5)}
    res = {"form": rt.embed_form(x, w), "shape": dict(B=B, L=L, N=N, d_model=D),
           "mbytes": (x.numel() + B * L * D) * 4 / 1e6}
    with torch.inference_mode():
        res["eager"] = _ab({k: (lambda n=n: rt.embed_forward(x, w, add, n)) for k, n in norms.items()}, launches, warmup)
        graphs = {}
        for k, n in norms.items():
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                keep = rt.embed_forward(x, w, add, n)
            graphs[k] = (gr, keep)
        res["graphed"] = _ab({k: v[0].replay for k, v in graphs.items()}, launches, warmup)
    for mode in ("eager", "graphed"):
        r = res[mode]
        r["rms_over_layer"] = r["rms"]["median_us"] / r["layer"]["median_us"]
        print(f"embed {name:14s} {mode:8s} rms {r['rms']['median_us']:8.1f} us   layer {r['layer']['median_us']:8.1f} us   "
              f"rms / layer {r['rms_over_layer']:.3f}   {res['form']}")
    return res


def run_forward(pkg, name, replays, warmup):
    """Graphed whole forwards of an "rms" and a "layer" model, alternated in one process."""
    gfs = {}
    for norm in ("rms", "layer"):
        net, x, kw = build(pkg, name, norm)
        gfs[norm] = (pkg.graph.GraphedForward(net, x, **kw), net)
        assert net._last_embed_backend == "hip", f"{norm}: the HIP embedding did not run"
    res = _ab({k: (lambda gf=v[0]: gf.replay(check=False)) for k, v in gfs.items()}, replays, warmup)
    res["rms_over_layer"] = res["rms"]["median_us"] / res["layer"]["median_us"]
    res["backends"] = {k: [v[1]._last_embed_backend, v[1]._last_context_backend] for k, v in gfs.items()}
    print(f"forward {name:14s} graphed rms {res['rms']['median_us']:9.1f} us   layer {res['layer']['median_us']:9.1f} us   "
          f"rms / layer {res['rms_over_layer']:.3f}")
    return res


def run_forecast(pkg, name, H, runs):
    """An H-step recursive forecast of an "rms" model: the device path against the reference's host loop."""
    import torch

    F = pkg.forecast
    net, x, kw = build(pkg, name, "rms", mode="recursive")
    times = {"device": [], "loop": []}
    with torch.inference_mode():
        assert F._device_ok(net, x, H, None, None, kw["series_static"], kw["series_ids"]), "no device path"
        calls = {"device": lambda: F.forecast_recursive_batch(net, x, H, **kw),
                 "loop": lambda: F.forecast_recursive_batch_loop(net, x, H, **kw)}
        outs = {k: fn() for k, fn in calls.items()}                                # warm: lazy builds, packs, workspace
        equal = all(torch.equal(a, b) for a, b in zip(outs["device"], outs["loop"]))
        for _ in range(runs):
            for k, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append(1e3 * (time.perf_counter() - t0))
    B, L, N, _, D, _ = SHAPES[name]
    res = {"shape": dict(B=B, L=L, N=N, d_model=D, H=H), "bit_equal": equal,
           **{k: {"median_ms": statistics.median(v), "min_ms": min(v)} for k, v in times.items()}}
    res["loop_over_device"] = res["loop"]["median_ms"] / res["device"]["median_ms"]
    print(f"forecast {name:14s} H={H}  device {res['device']['median_ms']:8.2f} ms   loop {res['loop']['median_ms']:8.2f} ms   "
          f"loop / device {res['loop_over_device']:.2f}   bit-equal {equal}")
    return res


def forward_child(root, name, replays, warmup):
    """The "rms" graphed forward of the checkout at ``root`` (this tree or the parent commit)."""
    sys.path.insert(0, str(root))
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    net, x, kw = build(pkg, name, "rms")
    gf = pkg.graph.GraphedForward(net, x, **kw)
    res = _ab({"rms": lambda: gf.replay(check=False)}, replays, warmup)["rms"]
    print(json.dumps({"embed_backend": net._last_embed_backend,
                      "context_backend": getattr(net, "_last_context_backend", None), **res}))


def run_parent(parent_root, parent_lib, name, replays, warmup):
    runs = []
    for which in ("parent", "this", "parent"):
        root = parent_root if which == "parent" else ROOT
        env = dict(os.environ)
        if which == "parent":
            env.pop("FLOWTIMES_LIB", None)
            if parent_lib:
                env["FLOWTIMES_LIB"] = str(parent_lib)
        r = subprocess.run([sys.executable, __file__, "--forward-child", name, "--root", str(root), "--replays",
                            str(replays), "--warmup", str(warmup)], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"forward of the {which} checkout failed:\n{r.stderr[-2000:]}")
        runs.append(dict(json.loads(r.stdout.strip().splitlines()[-1]), which=which))
        print(f"parent {name:14s} {which:6s} graphed rms forward {runs[-1]['median_us']:9.1f} us   "
              f"embedding {runs[-1]['embed_backend']}  context {runs[-1]['context_backend']}")
    old = [r["median_us"] for r in runs if r["which"] == "parent"]
    new = [r["median_us"] for r in runs if r["which"] == "this"][0]
    return {"runs": runs, "spread_us": abs(old[0] - old[1]), "parent_over_this": statistics.mean(old) / new}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--replays", type=int, default=60)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--forward-shapes", default="bench,pipeline_d256")
    ap.add_argument("--forecast-shape", default="pipeline_d64")
    ap.add_argument("--forecast-steps", type=int, default=28)
    ap.add_argument("--forecast-runs", type=int, default=7)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--forward-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=str(ROOT), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.forward_child:
        forward_child(Path(a.root), a.forward_child, a.replays, a.warmup)
        return 0
    parent = {}
    if a.parent_root:                                            # children first: one process at a time on the device
        for name in filter(None, a.forward_shapes.split(",")):
            parent[name] = run_parent(Path(a.parent_root).resolve(), a.parent_lib, name, a.replays, 10)
    sys.path.insert(0, str(ROOT))
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    result = {"device": torch.cuda.get_device_name(0),
              "method": "device events per launch / replay, A/B interleaved in one process, median; forecast: wall "
                        "time around a device synchronisation, alternated; parent: graph replays in fresh processes, "
                        "parent, this tree, parent",
              "embed": {}, "forward": {}, "parent_rms_forward": parent}
    for name in filter(None, a.shapes.split(",")):
        result["embed"][name] = run_embed(pkg, name, a.launches, a.warmup)
    for name in filter(None, a.forward_shapes.split(",")):
        result["forward"][name] = run_forward(pkg, name, a.replays, 10)
    if a.forecast_shape:
        result["forecast"] = run_forecast(pkg, a.forecast_shape, a.forecast_steps, a.forecast_runs)
    result["rms_embedding_slower_than_layer_beyond_box_spread_at"] = [
        f"{n}/{m}" for n, r in result["embed"].items() for m in ("eager", "graphed")
        if r[m]["rms_over_layer"] > 1.0 + BOX_SPREAD]
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
