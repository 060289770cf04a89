#!/usr/bin/env python3
"""Batch-sharded TimesNet forward, eager vs HIP-graph replay, over the capturable IPC exchange.

    python tools/shard_graph_time.py [--out profiles/shard_graph_time.json] [--iters 50] [--repeats 5]

Starts two fresh rank processes that share GPU 0, each under its own ``timeout -k``, and times on every rank
``ShardedTimesNet(model, exchange=IpcExchange(..., capturable=True))`` called eagerly and replayed through
``graph.GraphedForward`` (gather=False).  Then, in a third fresh process, the unsharded ``GraphedForward(model)``
(and the eager model) at the same per-rank batch.  Each number is device events around a window of ``--iters``
forwards that starts after a device synchronise (and, for the ranks, a barrier), ``--repeats`` windows per mode;
the JSON keeps every window, the tables print the median and the min-max spread.

Two processes on one GPU overlap each other's kernels, so these numbers show what the graph removes (the host's
per-launch cost), not multi-GPU scaling."""
import argparse
import json
import os
import socket
import statistics
import subprocess
import sys
import tempfile
from datetime import timedelta
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
# (name, global batch over 2 ranks, L, H, N, d_model)
SHAPES = (("bench_model", 64, 336, 96, 512, 64), ("c4_shard", 128, 720, 96, 4096, 128))
WORLD = 2


def _model(pkg, dev, B, L, H, N, D):
    import torch

    ks = [(3, 3), (5, 5), (7, 7)]
    torch.manual_seed(0)
    model = pkg.models.TimesNet(input_len=L, pred_len=H, d_model=D, d_ff=4 * D, n_layers=3, k_periods=5,
                                kernel_set=ks, dropout=0.0, activation="gelu", mode="direct", bottleneck_ratio=4.0,
                                use_checkpoint=True, id_embed_dim=32, use_zero_mean_context=True,
                                context_rank=16).eval().to(dev)
    x = torch.from_numpy(pkg.synth.make_input(B, L, N, seed=7)).to(dev)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        model(x[:2])                                            # lazy build, on the device (as bench.py)
        for p in model.parameters():
            if float(p.detach().abs().sum()) == 0.0:
                p.copy_(0.05 * torch.randn(p.shape, generator=g).to(p.device))
    return model, x


def _windows(fn, iters, repeats, barrier=None):
    import torch

    for _ in range(3):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        if barrier is not None:
            barrier()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def rank_main(rank, port, out_path, iters, repeats):
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=timedelta(seconds=120))
    res = {}
    try:
        dev = torch.device("cuda:0")
        for name, B, L, H, N, D in SHAPES:
            model, x = _model(pkg, dev, B, L, H, N, D)
            xl = x.chunk(WORLD, dim=0)[rank].contiguous()
            xch = pkg.dist.IpcExchange(None, dev, f_cap=L // 2 + 1, capturable=True)
            runner = pkg.dist.ShardedTimesNet(model, exchange=xch)
            with torch.inference_mode():
                eager = _windows(lambda: runner(xl, gather=False), iters, repeats, dist.barrier)
            g = pkg.graph.GraphedForward(runner, xl, gather=False)
            graph = _windows(lambda: g(g.inputs[0], gather=False), iters, repeats, dist.barrier)
            xch.check()
            res[name] = {"rows_per_rank": B // WORLD, "eager_ms": eager, "graph_ms": graph, "exchanges": xch.calls()}
            del g, runner
            xch.close()
            del model, x, xl
            torch.cuda.empty_cache()
    finally:
        dist.destroy_process_group()
    Path(out_path).write_text(json.dumps(res))


def single_main(out_path, iters, repeats):
    import torch

    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    res = {}
    for name, B, L, H, N, D in SHAPES:
        model, x = _model(pkg, dev, B // WORLD, L, H, N, D)
        with torch.inference_mode():
            eager = _windows(lambda: model(x), iters, repeats)
        g = pkg.graph.GraphedForward(model, x)
        graph = _windows(lambda: g(g.inputs[0]), iters, repeats)
        res[name] = {"rows": B // WORLD, "eager_ms": eager, "graph_ms": graph}
        del g, model, x
        torch.cuda.empty_cache()
    Path(out_path).write_text(json.dumps(res))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shard_graph_time.json"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit-s", type=int, default=600, help="time limit of each child process")
    ap.add_argument("--rank", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--port", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--single", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rank is not None:
        return rank_main(a.rank, a.port, a.child_out, a.iters, a.repeats)
    if a.single:
        return single_main(a.child_out, a.iters, a.repeats)

    me = [sys.executable, str(Path(__file__).resolve()), "--iters", str(a.iters), "--repeats", str(a.repeats)]
    lim = ["timeout", "-k", "10", str(a.limit_s)]
    with tempfile.TemporaryDirectory() as tmp:
        port = _free_port()
        outs = [os.path.join(tmp, f"rank{r}.json") for r in range(WORLD)]
        procs = [subprocess.Popen(lim + me + ["--rank", str(r), "--port", str(port), "--child-out", outs[r]])
                 for r in range(WORLD)]
        rcs = [p.wait() for p in procs]
        if any(rcs):
            sys.exit(f"rank processes failed: exit codes {rcs}")
        single_out = os.path.join(tmp, "single.json")
        rc = subprocess.run(lim + me + ["--single", "--child-out", single_out]).returncode
        if rc:
            sys.exit(f"unsharded process failed: exit code {rc}")
        ranks = [json.loads(Path(o).read_text()) for o in outs]
        single = json.loads(Path(single_out).read_text())

    import torch

    med = statistics.median
    result = {"tool": "tools/shard_graph_time.py", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available()
              else None, "world": WORLD, "placement": "two rank processes sharing GPU 0", "iters": a.iters,
              "repeats": a.repeats, "shapes": {}}
    print(f"{'shape':12s} {'run':28s} {'eager ms':>18s} {'graph ms':>18s}")
    for name, B, L, H, N, D in SHAPES:
        entry = {"config": f"TimesNet B={B} (= {WORLD} x {B // WORLD}) L={L}->H={H} N={N} d_model={D} d_ff={4 * D} "
                           f"layers=3 k=5 context_rank=16", "ranks": [r[name] for r in ranks], "single": single[name]}
        result["shapes"][name] = entry
        rows = [(f"sharded rank {r}", ranks[r][name]) for r in range(WORLD)]
        rows.append((f"unsharded B={B // WORLD}", single[name]))
        for label, d in rows:
            ce = f"{med(d['eager_ms']):.3f} ({min(d['eager_ms']):.3f}-{max(d['eager_ms']):.3f})"
            cg = f"{med(d['graph_ms']):.3f} ({min(d['graph_ms']):.3f}-{max(d['graph_ms']):.3f})"
            print(f"{name:12s} {label:28s} {ce:>18s} {cg:>18s}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
