"""Series-sharded (channel-sharded) TimesNet forwards over the IPC row exchange (dist.SeriesShardedTimesNet,
FtnRowExchange in include/flowtimes.h): a world of one against the unsharded model with eager calls and graph replays
interleaved; two ranks sharing the one GPU with even and uneven series splits at d_model 64 and 128; the collective
f16x2 range repair; and the capture refusals."""
import os
import socket
import sys
import warnings
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu
KS = [(3, 3), (5, 5), (7, 7)]
RTOL, ATOL = 1e-4, 2e-5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _model(pkg, dev, L, H, D, N, B, n_layers=2):
    """A TimesNet with every lazily built layer randomised (zero-initialised heads / context maps would hide a wrong
    series slice), identical on every rank (same seeds)."""
    cfg = dict(input_len=L, pred_len=H, d_model=D, d_ff=4 * D, n_layers=n_layers, k_periods=5, kernel_set=KS,
               dropout=0.0, activation="gelu", mode="direct", bottleneck_ratio=4.0, id_embed_dim=8,
               use_zero_mean_context=True, context_rank=4, use_constant_context_bias=True)
    torch.manual_seed(0)
    model = pkg.models.TimesNet(**cfg).eval().to(dev)
    xs = []
    for s in (3, 4):
        xh = torch.from_numpy(pkg.synth.make_input(B, L, N, seed=s))
        xs.append((xh.abs() + 0.5).to(dev))                        # count-like, keeps softplus in its usual range
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        model(xs[0][:2])                                           # lazy build with all N series, on the device
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.05 * torch.randn(p.shape, generator=g).to(p.device))
    return model, xs


def _clone(t):
    return tuple(v.clone() for v in t)


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


def test_world_of_one_eager_and_graph(ftn):
    dev = torch.device("cuda:0")
    model, xs = _model(ftn, dev, 336, 24, 64, 64, 4)
    with torch.inference_mode():
        want = [_clone(model(x)) for x in xs]
    want_p = model.period_selector.last_selected_periods.tolist()
    with _WorldOfOne():
        xch = ftn.dist.IpcExchange(None, dev, f_cap=336 // 2 + 1, capturable=True)
        rx = ftn.dist.series_row_exchanges(model, 4, device=dev)
        runner = ftn.dist.SeriesShardedTimesNet(model, 64, exchange=xch, row_exchange=rx)
        with torch.inference_mode():
            eager = [_clone(runner(x)) for x in xs]
        assert model.period_selector.last_selected_periods.tolist() == want_p
        for (r, d), (wr, wd) in zip(eager, want):
            torch.testing.assert_close(r, wr, rtol=RTOL, atol=ATOL)
            torch.testing.assert_close(d, wd, rtol=RTOL, atol=ATOL)
        g = ftn.graph.GraphedForward(runner, xs[0], gather=False)  # two eager warm-up calls, then the capture
        n = 2 + 2
        for how, i in (("graph", 1), ("eager", 0), ("graph", 0), ("graph", 1), ("eager", 1)):
            if how == "graph":
                got = _clone(g(xs[i], gather=False))
            else:
                with torch.inference_mode():
                    got = _clone(runner(xs[i]))
            n += 1
            assert torch.equal(got[0], eager[i][0]) and torch.equal(got[1], eager[i][1]), f"{how} call {i}"
        assert rx[0].calls() == rx[1].calls() == n == 9
        assert xch.calls() == 2 * n
        for x in (xch, *rx):
            x.check()
        del g
        for x in (xch, *rx):
            x.close()


def test_capture_refusals(ftn):
    dev = torch.device("cuda:0")
    model, xs = _model(ftn, dev, 336, 24, 64, 64, 4)
    with _WorldOfOne():
        xch = ftn.dist.IpcExchange(None, dev, f_cap=336 // 2 + 1, capturable=True)
        rx = ftn.dist.series_row_exchanges(model, 4, device=dev)
        cases = ((ftn.dist.SeriesShardedTimesNet(model, 64, exchange=xch), False, "row_exchange=None"),
                 (ftn.dist.SeriesShardedTimesNet(model, 64, row_exchange=rx), False, "exchange=None"),
                 (ftn.dist.SeriesShardedTimesNet(model, 64, exchange=xch, row_exchange=rx), True, "gather"))
        for runner, gather, what in cases:
            with pytest.raises(RuntimeError, match=what):
                ftn.graph.GraphedForward(runner, xs[0], gather=gather)
            with torch.inference_mode():                          # uncaptured: runs
                r, d = runner(xs[0], gather=gather)
            assert r.shape == d.shape == (4, 24, 64)
        torch.cuda.synchronize(dev)
        for x in (xch, *rx):
            x.check()
            x.close()


# ---- two ranks, two processes on the one GPU ---------------------------------------------------------------------
CASES = (("d64_even", 336, 24, 64, 64, 4, (32, 32)), ("d64_uneven", 336, 24, 64, 64, 4, (37, 27)),
         ("d128_even", 720, 96, 128, 64, 2, (32, 32)), ("d128_uneven", 720, 96, 128, 64, 2, (37, 27)))


def _two_rank_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist

    import __graft_entry__ as ge
    pkg = ge.load_package()
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        dev = torch.device("cuda:0")
        for name, L, H, D, N, B, split in CASES:
            model, xs = _model(pkg, dev, L, H, D, N, B)
            with torch.inference_mode():
                full = [_clone(model(x)) for x in xs]
            full_p = model.period_selector.last_selected_periods.tolist()
            off, n = sum(split[:rank]), split[rank]
            loc = [x[..., off:off + n].contiguous() for x in xs]
            xch = pkg.dist.IpcExchange(None, dev, f_cap=L // 2 + 1, capturable=True)
            rx = pkg.dist.series_row_exchanges(model, B, device=dev)
            runner = pkg.dist.SeriesShardedTimesNet(model, N, exchange=xch, row_exchange=rx)
            with torch.inference_mode():
                eager = [_clone(runner(x)) for x in loc]
                per = model.period_selector.last_selected_periods.tolist()
                gathered = [tuple(runner.gather_series(t) for t in e) for e in eager]
            g = pkg.graph.GraphedForward(runner, loc[0], gather=False)
            for i in (1, 0, 1):
                got = g(loc[i], gather=False)
                assert torch.equal(got[0], eager[i][0]) and torch.equal(got[1], eager[i][1]), (name, i)
            del g
            plain = pkg.dist.SeriesShardedTimesNet(model, N)       # torch.distributed (gloo) for both exchanges
            with torch.inference_mode():
                via_gloo = [_clone(plain(x)) for x in loc]
            calls = [xch.calls(), rx[0].calls(), rx[1].calls()]
            for x in (xch, *rx):
                x.check()
                x.close()
            for i in range(len(xs)):
                for k, what in enumerate(("rate", "disp")):
                    np.save(os.path.join(out_dir, f"{name}_{what}{i}_{rank}.npy"), gathered[i][k].cpu().numpy())
                    np.save(os.path.join(out_dir, f"{name}_want_{what}{i}_{rank}.npy"), full[i][k].cpu().numpy())
                    torch.testing.assert_close(via_gloo[i][k], eager[i][k], rtol=RTOL, atol=ATOL)
            np.save(os.path.join(out_dir, f"{name}_calls_{rank}.npy"), np.asarray(calls))
            np.save(os.path.join(out_dir, f"{name}_per_{rank}.npy"), np.asarray([per, full_p]))
        _range_repair(pkg, dev, rank, out_dir)
    finally:
        dist.destroy_process_group()


def _range_repair(pkg, dev, rank, out_dir):
    """Batch row 0 (blocks on rank 0) scaled out of the fp16 range, rank 1's rows clean: both ranks repeat together."""
    L, H, D, N, B, split = 336, 24, 64, 64, 4, (37, 27)
    model, xs = _model(pkg, dev, L, H, D, N, B)
    x = xs[0].clone()
    x[0] *= 1e6
    off, n = sum(split[:rank]), split[rank]
    xch = pkg.dist.IpcExchange(None, dev, f_cap=L // 2 + 1, capturable=True)
    rx = pkg.dist.series_row_exchanges(model, B, device=dev)
    runner = pkg.dist.SeriesShardedTimesNet(model, N, exchange=xch, row_exchange=rx)
    with torch.inference_mode(), warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        rate, disp = runner(x[..., off:off + n].contiguous())
        rate_all, disp_all = runner.gather_series(rate), runner.gather_series(disp)
    assert any("repeats the forward" in str(w.message) for w in seen), [str(w.message) for w in seen]
    assert all(b.engine == "bf16x3" for b in model.blocks)
    with torch.inference_mode():
        want = model(x)                                            # unsharded, on bf16x3 now
    calls = [xch.calls(), rx[0].calls(), rx[1].calls()]
    for e in (xch, *rx):
        e.check()
        e.close()
    np.save(os.path.join(out_dir, f"range_calls_{rank}.npy"), np.asarray(calls))
    for what, got, w in (("rate", rate_all, want[0]), ("disp", disp_all, want[1])):
        np.save(os.path.join(out_dir, f"range_{what}_{rank}.npy"), got.cpu().numpy())
        np.save(os.path.join(out_dir, f"range_want_{what}_{rank}.npy"), w.cpu().numpy())


def test_two_ranks_on_one_gpu(tmp_path):
    world = 2
    mp.spawn(_two_rank_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for name, *_ in CASES:
        c0, c1 = np.load(tmp_path / f"{name}_calls_0.npy"), np.load(tmp_path / f"{name}_calls_1.npy")
        assert c0.tolist() == c1.tolist() == [2 * (2 + 2 + 3), 2 + 2 + 3, 2 + 2 + 3], (name, c0, c1)
        p0, p1 = np.load(tmp_path / f"{name}_per_0.npy"), np.load(tmp_path / f"{name}_per_1.npy")
        assert p0[0].tolist() == p0[1].tolist() == p1[0].tolist(), name
        for i in range(2):
            for what in ("rate", "disp"):
                g0, g1 = np.load(tmp_path / f"{name}_{what}{i}_0.npy"), np.load(tmp_path / f"{name}_{what}{i}_1.npy")
                assert np.array_equal(g0, g1), (name, what, i)
                np.testing.assert_allclose(g0, np.load(tmp_path / f"{name}_want_{what}{i}_0.npy"), rtol=RTOL,
                                           atol=ATOL, err_msg=f"{name} {what} {i}")
    r0, r1 = np.load(tmp_path / "range_calls_0.npy"), np.load(tmp_path / "range_calls_1.npy")
    assert r0.tolist() == r1.tolist() == [2 * 2, 2, 2]              # the forward ran twice on both ranks
    for what in ("rate", "disp"):
        g0, g1 = np.load(tmp_path / f"range_{what}_0.npy"), np.load(tmp_path / f"range_{what}_1.npy")
        assert np.array_equal(g0, g1) and np.isfinite(g0).all()
        np.testing.assert_allclose(g0, np.load(tmp_path / f"range_want_{what}_0.npy"), rtol=RTOL, atol=ATOL)
