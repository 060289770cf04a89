"""world_size-2 gloo test (CPU) of the series-sharded model (dist.SeriesShardedTimesNet): each rank holds a contiguous
slice of the series, the partial value embeddings are reduce-scattered along B and summed in rank order, the blocks
run batch-sharded, the hidden rows are all-gathered and the heads run on each rank's own series.  The outputs
gathered along N must equal the single-process forward."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN, ROOT

WORLD = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _fixture_model(pkg, name):
    """The golden model fixture with its weights; m_context gets a fourth batch row so B splits over two ranks."""
    man = json.loads((GOLDEN / "manifest.json").read_text())
    cfg = dict(man["cases"][name]["cfg"])
    cfg["kernel_set"] = [tuple(k) for k in cfg["kernel_set"]]
    with np.load(GOLDEN / f"{name}.npz") as z:
        g = {k: z[k] for k in z.files}
    kw = {k: torch.from_numpy(g[k]) for k in ("x_mark", "series_static", "series_ids") if k in g}
    x = torch.from_numpy(g["x"])
    if x.size(0) % WORLD:
        x = torch.cat([x, torch.roll(x[:1], 5, dims=1) * 0.7 + 0.3], dim=0)
    model = pkg.models.TimesNet(**cfg).eval()
    with torch.no_grad():
        model(x, **kw)
    sd = {k[4:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd::")}
    d_ff = cfg["d_ff"] if cfg.get("d_ff") else cfg["d_model"]
    for li in range(cfg["n_layers"]):
        prm = pkg.synth.make_inception_params(cfg["d_model"], d_ff, cfg["kernel_set"],
                                              cfg.get("bottleneck_ratio", 1.0), seed=100 + li)
        for k, v in prm.items():
            sd[f"blocks.{li}.inception.{k}"] = torch.from_numpy(v)
    model.load_state_dict(sd, strict=True)
    return model, x, kw, g


def _split(n, world):
    """Contiguous slices in rank order, the first ranks one larger (N=5 -> 3/2)."""
    base, extra = divmod(n, world)
    sizes = [base + (r < extra) for r in range(world)]
    return [sum(sizes[:r]) for r in range(world)], sizes


def _local_kwargs(kw, off, n):
    out = {}
    if "x_mark" in kw:
        out["x_mark"] = kw["x_mark"]                               # per (b, t): every rank gets all B rows
    if "series_static" in kw:
        out["series_static"] = kw["series_static"][..., off:off + n, :]
    if "series_ids" in kw:
        out["series_ids"] = kw["series_ids"][..., off:off + n]
    return out


def _worker(rank, world, port, name, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    pkg = ge.load_package()
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        model, x, kw, _ = _fixture_model(pkg, name)
        N = x.size(-1)
        offs, sizes = _split(N, world)
        off, n = offs[rank], sizes[rank]
        runner = pkg.dist.SeriesShardedTimesNet(model, N)
        x_local = x[..., off:off + n].contiguous()
        lkw = _local_kwargs(kw, off, n)
        with torch.no_grad():
            rate, disp = runner(x_local, gather=True, **lkw)
            rate_l, disp_l = runner(x_local, **lkw)
            per = model.period_selector.last_selected_periods.numpy()
            assert model.period_selector.shard_group is None          # restored after the call
            assert torch.equal(rate[..., off:off + n], rate_l) and torch.equal(disp[..., off:off + n], disp_l)
            if "series_ids" in lkw:
                # ids left out: the global arange(offset, offset + n), not arange(n)
                lkw_none = dict(lkw, series_ids=None)
                lkw_arange = dict(lkw, series_ids=torch.arange(off, off + n))
                r_none, _ = runner(x_local, **lkw_none)
                r_arange, _ = runner(x_local, **lkw_arange)
                assert torch.equal(r_none, r_arange)
                np.save(os.path.join(out_dir, f"ids_none{rank}.npy"), runner.gather_series(r_none).numpy())
            with pytest.raises(ValueError, match="multiple of the world size"):
                runner(x_local[:3], **{k: (v[:3] if k == "x_mark" else v) for k, v in lkw.items()})
        np.save(os.path.join(out_dir, f"rate{rank}.npy"), rate.numpy())
        np.save(os.path.join(out_dir, f"disp{rank}.npy"), disp.numpy())
        np.save(os.path.join(out_dir, f"per{rank}.npy"), per)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name", ["m_context", "m_pipeline"])
def test_series_sharded_equals_single_process(name, tmp_path, ftn):
    model, x, kw, g = _fixture_model(ftn, name)
    with torch.no_grad():
        want_r, want_d = model(x, **kw)
    want_p = model.period_selector.last_selected_periods.tolist()
    mp.spawn(_worker, args=(WORLD, _free_port(), name, str(tmp_path)), nprocs=WORLD, join=True)
    r0, r1 = np.load(tmp_path / "rate0.npy"), np.load(tmp_path / "rate1.npy")
    d0, d1 = np.load(tmp_path / "disp0.npy"), np.load(tmp_path / "disp1.npy")
    assert np.array_equal(r0, r1) and np.array_equal(d0, d1)     # every rank gathers the same [B, H, N]
    assert np.load(tmp_path / "per0.npy").tolist() == want_p == np.load(tmp_path / "per1.npy").tolist()
    np.testing.assert_allclose(r0, want_r.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(d0, want_d.numpy(), rtol=1e-5, atol=1e-6)
    nref = g["rate"].shape[0]                                    # the fixture's own rows against the reference
    np.testing.assert_allclose(r0[:nref], g["rate"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(d0[:nref], g["dispersion"], rtol=1e-4, atol=1e-4)
    if "series_ids" in kw:
        with torch.no_grad():
            want_ids, _ = model(x, **dict(kw, series_ids=torch.arange(x.size(-1))))
        np.testing.assert_allclose(np.load(tmp_path / "ids_none0.npy"), want_ids.numpy(), rtol=1e-5, atol=1e-6)


def _refusal_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    pkg = ge.load_package()
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        model, x, kw, _ = _fixture_model(pkg, "m_context")
        N = x.size(-1)
        with pytest.raises(ValueError, match="not built for n_series"):
            pkg.dist.SeriesShardedTimesNet(model, N + 1)
        fresh = pkg.models.TimesNet(**{**json.loads((GOLDEN / "manifest.json").read_text())["cases"]["m_context"]["cfg"],
                                       "kernel_set": [(3, 3), (5, 5)]})
        with pytest.raises(ValueError, match="not built for n_series"):
            pkg.dist.SeriesShardedTimesNet(fresh, N)                # no lazily built, rank-local random weights
        runner = pkg.dist.SeriesShardedTimesNet(model, N)
        offs, sizes = _split(N, world)
        x_local = x[..., offs[rank]:offs[rank] + sizes[rank]].contiguous()
        lkw = _local_kwargs(kw, offs[rank], sizes[rank])
        with pytest.raises(ValueError, match="multiple of the world size"):
            with torch.no_grad():
                runner(x_local[:3], **lkw)
        with pytest.raises(RuntimeError, match="inference only"):
            runner(x_local, **lkw)                                  # autograd on
        model.train()
        with pytest.raises(RuntimeError, match="inference only"), torch.no_grad():
            runner(x_local, **lkw)
        model.eval()
        os.environ["TIMES_PERIOD_MAX_UNIQ"] = "2"
        try:
            with pytest.raises(NotImplementedError), torch.no_grad():
                runner(x_local, **lkw)
        finally:
            del os.environ["TIMES_PERIOD_MAX_UNIQ"]
        open(os.path.join(out_dir, f"ok{rank}"), "w").close()
    finally:
        dist.destroy_process_group()


def test_series_sharded_refusals(tmp_path):
    mp.spawn(_refusal_worker, args=(WORLD, _free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    assert (tmp_path / "ok0").exists() and (tmp_path / "ok1").exists()
