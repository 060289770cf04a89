#!/usr/bin/env python3
"""Series-sharded TimesNet forward against the batch-sharded and the unsharded model, eager and HIP-graph replay
(DESIGN §6).

    python tools/series_shard_time.py [--out profiles/series_shard_time.json] [--iters 30] [--repeats 5]

Starts two fresh rank processes that share GPU 0, each under its own ``timeout -k``.  Every rank times, on the same
global batch, ``SeriesShardedTimesNet`` (its slice of the series, IPC row exchanges and the capturable ``[F]``
exchange) and ``ShardedTimesNet`` (its B/2 rows of all series), each called eagerly and replayed through
``graph.GraphedForward`` (gather=False).  A third fresh process times the unsharded model on the whole batch.  Each
number is device events around a window of ``--iters`` forwards that starts after a device synchronise (and, for the
ranks, a barrier), ``--repeats`` windows per mode; the JSON keeps every window, the table prints the median and the
min-max spread.

Two processes on one GPU share its HBM and CUs and move no byte over xGMI: these numbers show the cost of the extra
kernels and launches of the series-sharded path, not multi-GPU scaling or xGMI bandwidth."""
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
SHAPES = (("bench_model", 64, 336, 96, 512, 64), ("c3_small_batch", 16, 720, 96, 4096, 128))
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
        model(x[:2])                                            # lazy build with all N series, on the device
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


def _time_runner(pkg, runner, x, iters, repeats, barrier):
    import torch

    with torch.inference_mode():
        eager = _windows(lambda: runner(x, gather=False), iters, repeats, barrier)
    g = pkg.graph.GraphedForward(runner, x, gather=False)
    graph = _windows(lambda: g(g.inputs[0], gather=False), iters, repeats, barrier)
    del g
    return eager, graph


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
            n = N // WORLD
            xs = x[..., rank * n:(rank + 1) * n].contiguous()
            xb = x.chunk(WORLD, dim=0)[rank].contiguous()
            xch = pkg.dist.IpcExchange(None, dev, f_cap=L // 2 + 1, capturable=True)
            rx = pkg.dist.series_row_exchanges(model, B, device=dev)
            series = pkg.dist.SeriesShardedTimesNet(model, N, exchange=xch, row_exchange=rx)
            s_eager, s_graph = _time_runner(pkg, series, xs, iters, repeats, dist.barrier)
            batch = pkg.dist.ShardedTimesNet(model, exchange=xch)
            b_eager, b_graph = _time_runner(pkg, batch, xb, iters, repeats, dist.barrier)
            for e in (xch, *rx):
                e.check()
            res[name] = {"series_local": n, "rows_per_rank": B // WORLD,
                         "series_sharded": {"eager_ms": s_eager, "graph_ms": s_graph, "row_exchanges": rx[0].calls()},
                         "batch_sharded": {"eager_ms": b_eager, "graph_ms": b_graph}}
            for e in (xch, *rx):
                e.close()
            del series, batch, model, x, xs, xb
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
        model, x = _model(pkg, dev, B, L, H, N, D)
        with torch.inference_mode():
            eager = _windows(lambda: model(x), iters, repeats)
        g = pkg.graph.GraphedForward(model, x)
        graph = _windows(lambda: g(g.inputs[0]), iters, repeats)
        res[name] = {"rows": B, "eager_ms": eager, "graph_ms": graph}
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "series_shard_time.json"))
    ap.add_argument("--iters", type=int, default=30)
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
    result = {"tool": "tools/series_shard_time.py", "device": torch.cuda.get_device_name(0) if torch.cuda.is_available()
              else None, "world": WORLD, "placement": "two rank processes sharing GPU 0 (no xGMI traffic)",
              "iters": a.iters, "repeats": a.repeats, "shapes": {}}
    print(f"{'shape':15s} {'run':30s} {'eager ms':>20s} {'graph ms':>20s}")
    for name, B, L, H, N, D in SHAPES:
        entry = {"config": f"TimesNet B={B} L={L}->H={H} N={N} (= {WORLD} x {N // WORLD}) d_model={D} d_ff={4 * D} "
                           f"layers=3 k=5 context_rank=16", "ranks": [r[name] for r in ranks], "single": single[name]}
        result["shapes"][name] = entry
        rows = []
        for r in range(WORLD):
            rows.append((f"series-sharded rank {r}", ranks[r][name]["series_sharded"]))
            rows.append((f"batch-sharded rank {r}", ranks[r][name]["batch_sharded"]))
        rows.append((f"unsharded B={B}", single[name]))
        for label, d in rows:
            ce = f"{med(d['eager_ms']):.3f} ({min(d['eager_ms']):.3f}-{max(d['eager_ms']):.3f})"
            cg = f"{med(d['graph_ms']):.3f} ({min(d['graph_ms']):.3f}-{max(d['graph_ms']):.3f})"
            print(f"{name:15s} {label:30s} {ce:>20s} {cg:>20s}")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
