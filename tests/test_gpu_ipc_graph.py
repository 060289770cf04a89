"""Batch-sharded forwards captured as one HIP graph over the capturable IPC exchange (dist.IpcExchange(capturable=True),
FtnExchange.mode 1 in include/flowtimes.h): the call counter lives in the exchange buffer, so graph replays and eager
calls can be mixed on one exchange and every result is bit-equal to the eager sharded call.  Capturing what cannot be
captured - a mode-0 exchange, the torch.distributed exchange, an output all-gather - raises."""
import os
import socket
import sys
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu
KS = [(3, 3), (5, 5), (7, 7)]
B, L, C, K = 8, 96, 64, 3
INPUTS = ((5, (24, 12, 8)), (6, (16, 6, 32)), (7, (48, 4, 12)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _block(ftn, dev):
    T = ftn.models.timesnet
    blk = T.TimesBlock(C, KS, 0.0, "gelu", d_ff=4 * C, bottleneck_ratio=4.0)
    sd = ftn.synth.make_inception_params(C, 4 * C, KS, 4.0, 3)
    blk.inception.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    blk.period_selector = T.FFTPeriodSelector(K, L)
    return blk.eval().to(dev)


class _WorldOfOne:
    """A one-rank gloo group in this process; FTN_BENCH_FORCE_DIST=1 makes it take the sharded path."""

    def __enter__(self):
        import torch.distributed as dist

        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
        dist.init_process_group("gloo", rank=0, world_size=1, timeout=timedelta(seconds=120))
        os.environ["FTN_BENCH_FORCE_DIST"] = "1"
        return self

    def __exit__(self, *exc):
        import torch.distributed as dist

        os.environ.pop("FTN_BENCH_FORCE_DIST", None)
        dist.destroy_process_group()
        return False


def test_capturable_exchange_world_of_one_graph_and_eager(ftn):
    """Eager calls and replays interleaved on one exchange, three inputs, both buffer halves, the parity flipping
    between eager calls and replays: every output is the unsharded block's, and the device counter counts them all."""
    dev = torch.device("cuda:0")
    blk = _block(ftn, dev)
    xs = [torch.from_numpy(ftn.synth.make_input(B, L, C, seed=s, planted=p)).to(dev) for s, p in INPUTS]
    with torch.inference_mode():
        want = [blk(x).clone() for x in xs]
    with _WorldOfOne():
        xch = ftn.dist.IpcExchange(None, dev, f_cap=64, capturable=True)
        runner = ftn.dist.ShardedTimesBlock(blk, exchange=xch)
        g = ftn.graph.GraphedForward(runner, xs[0], gather=False)    # two eager warm-up calls, then the capture
        assert xch.calls() == 2 and int(xch.x.seq) == 0               # the host never counts in mode 1
        n = 2
        for how, i in (("eager", 0), ("graph", 1), ("graph", 2), ("eager", 1), ("graph", 0)):
            if how == "eager":
                with torch.inference_mode():
                    got = runner(xs[i], gather=False).clone()
            else:
                got = g(xs[i], gather=False).clone()
            n += 1
            assert torch.equal(got, want[i]), f"{how} call on input {i} differs from the unsharded block"
        assert xch.calls() == n == 7
        xch.check()
        del g
        xch.close()


def test_capture_refuses_what_cannot_be_captured(ftn):
    """A mode-0 exchange (the captured sequence number would be reused: a silent race), the torch.distributed exchange
    and gather=True (collectives) are refused at capture time; the same calls still run eagerly."""
    dev = torch.device("cuda:0")
    blk = _block(ftn, dev)
    x = torch.from_numpy(ftn.synth.make_input(B, L, C, seed=5, planted=(24, 12, 8))).to(dev)
    with _WorldOfOne():
        x0 = ftn.dist.IpcExchange(None, dev, f_cap=64)
        x1 = ftn.dist.IpcExchange(None, dev, f_cap=64, capturable=True)
        cases = ((ftn.dist.ShardedTimesBlock(blk, exchange=x0), False, "capturable"),
                 (ftn.dist.ShardedTimesBlock(blk), False, "exchange=None"),
                 (ftn.dist.ShardedTimesBlock(blk, exchange=x1), True, "gather"))
        for runner, gather, what in cases:
            with pytest.raises(RuntimeError, match=what):
                ftn.graph.GraphedForward(runner, x, gather=gather)
            with torch.inference_mode():                               # uncaptured: as before
                y = runner(x, gather=gather)
            assert y.shape == x.shape
        torch.cuda.synchronize(dev)
        x0.check()
        x1.check()
        x0.close()
        x1.close()


# ---- two ranks, two processes on the one GPU: the whole model captured -------------------------------------------
MB, ML, MH, MN, MD = 64, 336, 24, 64, 64


def _model(pkg, dev):
    cfg = dict(input_len=ML, pred_len=MH, d_model=MD, d_ff=4 * MD, n_layers=3, k_periods=5, kernel_set=KS,
               dropout=0.0, activation="gelu", mode="direct", bottleneck_ratio=4.0, id_embed_dim=32,
               use_zero_mean_context=True, context_rank=16)
    torch.manual_seed(0)
    model = pkg.models.TimesNet(**cfg).eval().to(dev)
    xs = []
    for s in (3, 4, 5):
        xh = torch.from_numpy(pkg.synth.make_input(MB, ML, MN, seed=s))
        xs.append((xh.abs() + 0.5).to(dev))                        # count-like, keeps softplus in its usual range
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        model(xs[0][:2])                                           # lazy build, on the device
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:                        # zero-initialised heads / context: randomise
                p.copy_(0.05 * torch.randn(p.shape, generator=g).to(p.device))
    return model, xs


def _model_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist

    import __graft_entry__ as ge
    pkg = ge.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        dev = torch.device("cuda:0")                              # both ranks on the one GPU of the box
        model, xs = _model(pkg, dev)
        with torch.inference_mode():                              # the single-process full-batch forward
            full = [tuple(t.clone() for t in model(x)) for x in xs]
        full_p = model.period_selector.last_selected_periods.tolist()
        shards = [x.chunk(world, dim=0)[rank].contiguous() for x in xs]
        xch = pkg.dist.IpcExchange(None, dev, f_cap=ML // 2 + 1, capturable=True)
        runner = pkg.dist.ShardedTimesNet(model, exchange=xch)
        g = pkg.graph.GraphedForward(runner, shards[0], gather=False)
        calls = 2 * 3                                             # two warm-up forwards, three blocks each
        eager = []
        with torch.inference_mode():
            for x in shards:
                eager.append(tuple(t.clone() for t in runner(x, gather=False)))
                calls += 3
        eager_p = model.period_selector.last_selected_periods.tolist()
        for rep in range(2):                                      # 6 replays, 18 exchanges
            for i, x in enumerate(shards):
                rate, disp = g(x, gather=False)
                calls += 3
                assert torch.equal(rate, eager[i][0]) and torch.equal(disp, eager[i][1]), \
                    f"replay {rep}/{i}: graph differs from the eager sharded call"
                if rep == 1:
                    rate_all = pkg.dist.gather_batch(rate.clone())
                    disp_all = pkg.dist.gather_batch(disp.clone())
                    np.save(os.path.join(out_dir, f"rate{i}_{rank}.npy"), rate_all.cpu().numpy())
                    np.save(os.path.join(out_dir, f"disp{i}_{rank}.npy"), disp_all.cpu().numpy())
                    if rank == 0:
                        np.save(os.path.join(out_dir, f"want_rate{i}.npy"), full[i][0].cpu().numpy())
                        np.save(os.path.join(out_dir, f"want_disp{i}.npy"), full[i][1].cpu().numpy())
        assert eager_p == full_p, (eager_p, full_p)
        n = xch.calls()
        assert n == calls, (n, calls)
        np.save(os.path.join(out_dir, f"calls_{rank}.npy"), np.asarray([n]))
        np.save(os.path.join(out_dir, f"per_{rank}.npy"), np.asarray(eager_p))
        xch.check()
        del g
        xch.close()
    finally:
        dist.destroy_process_group()


def test_sharded_model_graph_two_ranks_on_one_gpu(tmp_path):
    world = 2
    mp.spawn(_model_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert np.load(tmp_path / "calls_0.npy").tolist() == np.load(tmp_path / "calls_1.npy").tolist() == [33]
    assert np.load(tmp_path / "per_0.npy").tolist() == np.load(tmp_path / "per_1.npy").tolist()
    for i in range(3):
        for name in ("rate", "disp"):
            got0, got1 = np.load(tmp_path / f"{name}{i}_0.npy"), np.load(tmp_path / f"{name}{i}_1.npy")
            assert np.array_equal(got0, got1)
            np.testing.assert_allclose(got0, np.load(tmp_path / f"want_{name}{i}.npy"), rtol=1e-4, atol=2e-5)


# ---- f16x2 range repair with only rank 0's rows out of range -------------------------------------------------------
def _range_worker(rank, world, port, out_dir):
    import warnings

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist

    import __graft_entry__ as ge
    pkg = ge.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        dev = torch.device("cuda:0")
        xch = pkg.dist.IpcExchange(None, dev, f_cap=ML // 2 + 1, capturable=True)
        # the bare block: rank 0 repairs its rows on its own, on the selection of the full batch
        blk = _block(pkg, dev)
        x = torch.from_numpy(np.load(os.path.join(out_dir, "x.npy"))).chunk(world, dim=0)[rank].to(dev)
        runner = pkg.dist.ShardedTimesBlock(blk, exchange=xch)
        with torch.inference_mode(), warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            y = runner(x, gather=False)
            blk.check_range()
        assert sum("fp16 range" in str(w.message) for w in seen) == (1 if rank == 0 else 0)
        np.save(os.path.join(out_dir, f"y_{rank}.npy"), y.cpu().numpy())
        np.save(os.path.join(out_dir, f"p_{rank}.npy"), np.asarray(blk.period_selector.last_selected_periods.tolist()))
        block_calls = xch.calls()
        # the whole model: every rank repeats the forward when one rank trips
        model, xs = _model(pkg, dev)
        xm = xs[0].clone()
        xm[:MB // world] *= 1e6                                    # rank 0's rows
        runner = pkg.dist.ShardedTimesNet(model, exchange=xch)
        with torch.inference_mode(), warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            rate, disp = runner(xm.chunk(world, dim=0)[rank].contiguous(), gather=False)
        assert sum("fp16 range" in str(w.message) for w in seen) == 1, [str(w.message) for w in seen]
        assert all(b.engine == "bf16x3" for b in model.blocks)
        with torch.inference_mode():
            want = model(xm)                                       # unsharded, on bf16x3 now
        for got, w in ((rate, want[0]), (disp, want[1])):
            torch.testing.assert_close(got, w.chunk(world, dim=0)[rank], rtol=1e-4, atol=2e-5)
        np.save(os.path.join(out_dir, f"calls_{rank}.npy"), np.asarray([block_calls, xch.calls()]))
        xch.check()
        xch.close()
    finally:
        dist.destroy_process_group()


def test_range_repair_two_ranks_on_one_gpu(ftn, tmp_path):
    """Only rank 0's rows leave the fp16 range.  ShardedTimesBlock: check_range() repairs rank 0's rows without a second
    exchange (the exchange counts stay equal), both ranks keep the full batch's periods, and the rows are the
    reference's.  ShardedTimesNet: both ranks warn and run the forward twice, and match the unsharded bf16x3 model."""
    from oracle import timesblock_oracle as orc
    from test_gpu_range import _close

    world = 2
    x = ftn.synth.make_input(B, L, C, seed=6, planted=(24, 12, 8))
    x = (x / np.abs(x).max()).astype(np.float32)
    x[:B // world] *= np.float32(1e5)
    np.save(tmp_path / "x.npy", x)
    mp.spawn(_range_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    c0, c1 = np.load(tmp_path / "calls_0.npy").tolist(), np.load(tmp_path / "calls_1.npy").tolist()
    assert c0 == c1 == [1, 1 + 2 * 3], (c0, c1)                   # one block call; two forwards of three blocks
    sd = ftn.synth.make_inception_params(C, 4 * C, KS, 4.0, 3)
    y_ref, aux = orc.timesblock_forward(torch.from_numpy(x), {k: torch.from_numpy(v) for k, v in sd.items()}, KS,
                                        "gelu", K, L)
    for r in range(world):
        assert np.load(tmp_path / f"p_{r}.npy").tolist() == aux.sel.periods
        rows = slice(r * B // world, (r + 1) * B // world)
        y = np.load(tmp_path / f"y_{r}.npy")
        assert np.isfinite(y).all()
        err, tol = _close(y, y_ref.numpy()[rows], x[rows])
        assert err <= tol, (r, err, tol)
