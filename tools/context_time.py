#!/usr/bin/env python3
"""The context front end in HIP (``csrc/context.hip``) beside the torch composition it replaces, and the graphed
whole-model forward with and without it.

    python tools/context_time.py [--out profiles/context_time.json] [--launches 200] [--warmup 30]

Front end alone: one process, the same model and tensors, the two versions issued alternately (A, B, A, B, ...), each
between its own pair of device events; the figure is the median over ``--launches`` of each after ``--warmup``
alternations (the method of ``tools/shell_wide_time.py``).  A is what the model runs: ``_rows_of`` ->
``_context_terms`` -> ``_hip_embed_terms`` -> ``_late_bias`` (three launches).  B is ``torch_front_end`` below: the
torch ops those bodies composed before the kernels existed, restated here from the modules of the same model, so B
does not depend on the code under test or on ``FTN_CTX_HIP``.  Both produce ``add [B|1, L, D]`` and ``late``.

Whole model: ``graph.GraphedForward`` replays in a fresh child process per configuration because ``FTN_CTX_HIP`` is
read once: switch off, feature on, switch off again - the two "off" runs show the run-to-run spread the comparison
has to be read against."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
# name: B, L, N, H, d_model, per-sample context
SHAPES = {"pipeline_d64": (4096, 28, 1, 7, 64, True), "pipeline_d256": (4096, 28, 1, 7, 256, True),
          "bench_model": (256, 336, 512, 96, 64, False)}
F_STATIC, STATIC_DIM, ID_DIM, RANK, TIME_DIM = 8, 16, 32, 8, 4


def build(pkg, name, n_layers=1):
    """The model of a shape with the whole context front end, and its inputs ``(x, mark, kw)`` on the device."""
    import torch

    B, L, N, H, D, per_sample = SHAPES[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = pkg.models.TimesNet(input_len=L, pred_len=H, d_model=D, d_ff=D, n_layers=n_layers, k_periods=3,
                              kernel_set=[(3, 3), (5, 5)], dropout=0.0, activation="gelu", mode="direct",
                              use_checkpoint=False, id_embed_dim=ID_DIM, static_proj_dim=STATIC_DIM,
                              use_zero_mean_context=True, context_rank=RANK, use_constant_context_bias=True,
                              use_late_bias_head=True).eval()
    g = torch.Generator().manual_seed(1)
    t = torch.arange(L, dtype=torch.float32).view(1, -1, 1)
    x = (torch.rand(B, L, N, generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 7.0)).to(dev)
    mark = torch.randn(1, L, TIME_DIM, generator=g).to(dev).expand(B, -1, -1)          # the pipeline's expanded marks
    if per_sample:
        kw = dict(series_static=torch.randn(B, N, F_STATIC, generator=g).to(dev),
                  series_ids=torch.randint(0, 3000, (B, N), generator=g).to(dev))
        kw["series_ids"][0, 0] = 2999                                              # the vocabulary the table is built for
    else:
        kw = dict(series_static=torch.randn(N, F_STATIC, generator=g).to(dev), series_ids=torch.arange(N, device=dev))
    with torch.inference_mode():
        net(x, mark, **kw)
        for p in net.parameters():                              # wake the zero-initialised heads / context maps
            if float(p.detach().abs().sum()) == 0.0:
                p.copy_((0.05 * torch.randn(p.shape, generator=g)).to(dev))
        net(x, mark, **kw)
    return net, x, mark, kw


def torch_front_end(net, window, mark, static, ids):
    """The torch composition of the context front end (series rows, context terms through the value weight, the
    embedding's ``add``, the late bias), op for op what ``models/shell.py`` ran before ``csrc/context.hip``."""
    import torch
    import torch.nn.functional as F

    B, L = window.size(0), window.size(1)
    shared = static.ndim == 2 and ids.size(0) == 1
    Bc = 1 if shared else B
    st = static if static.ndim == 3 else static.unsqueeze(0).expand(Bc, -1, -1)
    ln = lambda m, v: F.layer_norm(v, m.normalized_shape, m.weight, m.bias, m.eps)
    cols = [ln(net.static_norm, net.static_proj(st)), net.series_embedding(ids.expand(Bc, -1) if ids.size(0) != Bc else ids)]
    rows = ln(net.context_norm, torch.cat(cols, dim=-1))
    coeff = net.context_coeff(rows)
    bias = net.context_proj(rows).squeeze(-1)
    emb = net.embedding
    w = emb.value_embedding.weight
    aux = emb.position_embedding(window[:1]) + emb.temporal_embedding(mark)
    if emb.aux_norm is not None:
        aux = emb.gate * ln(emb.aux_norm, aux)
    add = aux + emb.value_embedding.bias
    add = add + net.temporal_context.project(coeff.float(), L, w)
    add = add + (bias.float() @ w.t()).unsqueeze(1)
    add = add.float().contiguous()
    lb = net.late_bias_head(ln(net.late_bias_norm, rows))
    late = (net.late_bias_gate * lb.transpose(1, 2)).float().contiguous()
    return add, late


def hip_front_end(net, window, mark, static, ids):
    rows = net._rows_of(window, static, ids)
    coeff, bias = net._context_terms(rows)
    _, add, _ = net._hip_embed_terms(window, mark, coeff, bias)
    return add, net._late_bias(rows)


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


def run_shape(pkg, name, launches, warmup):
    import torch

    net, x, mark, kw = build(pkg, name)
    static, ids = kw["series_static"], kw["series_ids"]
    ids2 = ids.view(1, -1) if ids.ndim == 1 else ids
    with torch.inference_mode():
        a_add, a_late = hip_front_end(net, x, mark, static, ids2)
        assert net._last_context_backend == "hip", "the HIP front end did not run (FTN_CTX_HIP=0?)"
        b_add, b_late = torch_front_end(net, x, mark, static, ids2)
        diff = max(float((a_add - b_add).abs().max()), float((a_late - b_late).abs().max()))
        assert diff < 1e-4, f"the two front ends disagree: {diff}"
        # eager: the launches of either version are enqueued back to back; graphed: what a replay of the forward pays
        res = {"eager": _ab({"hip": lambda: hip_front_end(net, x, mark, static, ids2),
                             "torch": lambda: torch_front_end(net, x, mark, static, ids2)}, launches, warmup)}
        graphs = {}
        for key, fn in (("hip", hip_front_end), ("torch", torch_front_end)):
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                keep = fn(net, x, mark, static, ids2)
            graphs[key] = (gr, keep)
        res["graphed"] = _ab({k: v[0].replay for k, v in graphs.items()}, launches, warmup)
    B, L, N, H, D, per_sample = SHAPES[name]
    res.update(shape=dict(B=B, L=L, N=N, H=H, d_model=D, Bc=B if per_sample else 1), add_rows=int(a_add.shape[0]),
               add_mbytes=a_add.numel() * 4 / 1e6, max_abs_diff=diff)
    for mode in ("eager", "graphed"):
        r = res[mode]
        r["torch_over_hip"] = r["torch"]["median_us"] / r["hip"]["median_us"]
        print(f"{name:14s} {mode:8s} hip {r['hip']['median_us']:9.1f} us   torch {r['torch']['median_us']:9.1f} us   "
              f"torch / hip {r['torch_over_hip']:.2f}")
    return res


def model_child(name, replays, warmup):
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    net, x, mark, kw = build(pkg, name, n_layers=2)
    gf = pkg.graph.GraphedForward(net, x, mark, **kw)
    for _ in range(warmup):
        gf.replay(check=False)
    torch.cuda.synchronize()
    ev = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        gf.replay(check=False)
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    times = [1e3 * a.elapsed_time(b) for a, b in ev]
    print(json.dumps({"ctx_hip": os.environ.get("FTN_CTX_HIP", "1"), "median_us": statistics.median(times),
                      "min_us": min(times), "replays": replays, "context_backend": net._last_context_backend}))


def run_model(name, replays, warmup):
    runs = []
    for value in ("0", "1", "0"):
        env = dict(os.environ, FTN_CTX_HIP=value)
        r = subprocess.run([sys.executable, __file__, "--model-child", name, "--model-replays", str(replays),
                            "--warmup", str(warmup)], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"whole-model run (FTN_CTX_HIP={value}) failed:\n{r.stderr[-2000:]}")
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(f"model {name:14s} FTN_CTX_HIP={value}  graphed replay {runs[-1]['median_us']:9.1f} us   "
              f"context {runs[-1]['context_backend']}")
    off = [r["median_us"] for r in runs if r["ctx_hip"] == "0"]
    on = [r["median_us"] for r in runs if r["ctx_hip"] == "1"][0]
    spread = abs(off[0] - off[1])
    return {"runs": runs, "spread_us": spread, "on_minus_slower_off_us": on - max(off),
            "not_slower_beyond_spread": on <= max(off) + spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--model-shapes", default="pipeline_d256,bench_model")
    ap.add_argument("--model-replays", type=int, default=60)
    ap.add_argument("--model-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    if a.model_child:
        model_child(a.model_child, a.model_replays, a.warmup)
        return 0
    models = {}
    if a.model_replays > 0:                                      # children first: one process at a time on the device
        for name in filter(None, a.model_shapes.split(",")):
            models[name] = run_model(name, a.model_replays, 10)
    import torch
    import __graft_entry__ as ge

    pkg = ge.load_package()
    result = {"device": torch.cuda.get_device_name(0),
              "method": "device events per launch, A/B interleaved in one process, median; whole model: graph replays "
                        "in fresh processes, FTN_CTX_HIP = 0, 1, 0",
              "shapes": {}, "model": models}
    for name in filter(None, a.shapes.split(",")):
        result["shapes"][name] = run_shape(pkg, name, a.launches, a.warmup)
    slower = [n for n, r in result["shapes"].items()
              if any(r[m]["hip"]["median_us"] > r[m]["torch"]["median_us"] for m in ("eager", "graphed"))]
    result["front_end_slower_at"] = slower
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    return 0 if not slower and all(m["not_slower_beyond_spread"] for m in models.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
