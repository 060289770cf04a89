"""Path summaries on the MI355X (``ftn_path_summary`` behind ``score.path_summary``): every padded size of the sort
network in both kernel forms against the numpy oracle of tests/paths_checks.py and the torch backend - bit for bit on
integer-valued samples, sorted values bit for bit and sums within one fp32 ulp on real-valued ones - special values,
strided and misaligned views, guard words around every output, independence of the grid, more ranks than one launch
takes, the sampled recursive forecast end to end, and a captured call."""
import numpy as np
import pytest
import torch

import paths_checks as pc
from test_gpu_recursive import _inputs, _model
from test_gpu_sample import _views

pytestmark = pytest.mark.gpu
KEYS = ("quantiles", "mean", "crps", "sorted")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _hip(ftn, x, levels, window, reduce, y=None, want_sorted=True):
    out = ftn.score.path_summary(x, levels, y, window=window, reduce=reduce, want_sorted=want_sorted)
    assert ftn.score._last_backend == "hip"
    return {k: v.cpu().numpy() for k, v in out.items()}


def _torch(ftn, x, levels, window, reduce, y):
    out = ftn.score.path_summary(torch.from_numpy(x), levels, torch.from_numpy(y), window=window, reduce=reduce,
                                 want_sorted=True, backend="torch")
    assert ftn.score._last_backend == "torch"
    return {k: v.numpy() for k, v in out.items()}


def _exact(got, want, where):
    for k in KEYS:
        assert pc.same(got[k], want[k]), (k,) + where


def _close(got, want, where):
    P = want["sorted"].shape[0]
    assert pc.same(got["sorted"], want["sorted"]) and pc.same(got["quantiles"], want["quantiles"]), where
    mean64 = want["sorted"].astype(np.float64).sum(0) / P
    err_m = np.nanmax(np.abs(got["mean"] - mean64) / np.spacing(want["mean_scale"].astype(np.float32)))
    err_c = np.nanmax(np.abs(got["crps"] - want["crps64"]) / np.spacing(want["scale"].astype(np.float32)))
    print(f"PATHS_ULP {where} mean {err_m:.3f} crps {err_c:.3f}")
    assert pc.within_ulp(got["mean"], mean64, want["mean_scale"]), where
    assert pc.within_ulp(got["crps"], want["crps64"], want["scale"]), where


@pytest.mark.parametrize("P", pc.PATHS)
def test_every_size_against_the_oracle(P, ftn, dev):
    g = np.random.default_rng(1000 + P)
    for B, H, N in pc.SHAPES:
        for window in pc.windows(H):
            w = 1 if window is None else window
            data = {"counts": (pc.counts(g, (P, B, H, N), 0.7), pc.counts(g, (B, H, N), 0.7)),
                    "big": (pc.big_counts(g, (P, B, H, N), w), pc.big_counts(g, (B, H, N), w)),
                    "real": (g.standard_normal((P, B, H, N)).astype(np.float32),
                             g.standard_normal((B, H, N)).astype(np.float32))}
            for kind, (x, y) in data.items():
                xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
                assert ftn.runtime.path_summary_form(xd, yd, w) == pc.form(P, N % 4 == 0), (P, B, H, N)
                for reduce in ("sum", "max"):
                    where = (P, (B, H, N), window, reduce, kind)
                    want = pc.summary(x, pc.LEVELS, window, reduce, y)
                    got = _hip(ftn, xd, pc.LEVELS, window, reduce, yd)
                    assert got["sorted"].shape == (P, B, H // w, N) and got["quantiles"].shape == (3, B, H // w, N)
                    if kind == "real":
                        _close(got, want, where)
                    else:
                        _exact(got, want, where)
                        _exact(got, _torch(ftn, x, pc.LEVELS, window, reduce, y), where)


@pytest.mark.parametrize("P", [9, 64, 100])
def test_special_values(P, ftn, dev):
    g = np.random.default_rng(7)
    for B, H, N in ((2, 4, 8), (2, 4, 3)):
        x, y = pc.counts(g, (P, B, H, N), 3.0), pc.counts(g, (B, H, N), 3.0)
        x[4, 0, 1, 2] = np.nan                                  # a NaN path in one column
        x[:, 1, 2, 0] = np.nan                                  # an all-NaN column
        x[2, 1, 0, 1], x[3, 0, 3, 0], x[5, 1, 1, 1], x[6, 1, 1, 1] = np.inf, -np.inf, np.inf, -np.inf
        y[0, 0, 0], y[1, 3, 2] = np.nan, np.inf
        xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        for reduce in ("sum", "max"):
            for window in (None, 2, 4):
                want = pc.summary(x, pc.LEVELS + [0.999], window, reduce, y)
                got = _hip(ftn, xd, pc.LEVELS + [0.999], window, reduce, yd)
                _exact(got, want, (P, N, reduce, window))
        s = _hip(ftn, xd, [0.999], None, "sum", yd)
        assert np.isnan(s["sorted"][-1, 0, 1, 2]) and not np.isnan(s["sorted"][-2, 0, 1, 2])
        assert np.isnan(s["sorted"][:, 1, 2, 0]).all() and np.isnan(s["mean"][0, 1, 2])
        assert s["sorted"][0, 1, 1, 1] == -np.inf and s["sorted"][-1, 1, 1, 1] == np.inf


def _sample_views(x, dev):
    """``x`` [P,B,H,N] as views: name -> (view, keeps whole 16-byte quads)."""
    P, B, H, N = x.shape
    row = H * N
    out = {}
    for name, pad in (("batch+2", 2), ("batch+4", 4)):
        wide = torch.zeros(P, B, row + pad, device=dev)
        wide[:, :, :row] = x.reshape(P, B, row)
        out[name] = (wide[:, :, :row].view(P, B, H, N), pad % 4 == 0)
        assert out[name][0].stride(1) == row + pad
    buf = torch.zeros(x.numel() + 1, device=dev)
    buf[1:] = x.reshape(-1)
    out["offset"] = (buf[1:].view(P, B, H, N), False)
    assert out["offset"][0].data_ptr() % 16 == 4
    for name, pad in (("path+3", 3), ("path+64", 64)):
        wide = torch.zeros(P, B * row + pad, device=dev)
        wide[:, :B * row] = x.reshape(P, B * row)
        out[name] = (wide[:, :B * row].view(P, B, H, N), pad % 4 == 0)
        assert out[name][0].stride(0) == B * row + pad > B * row
    return out


@pytest.mark.parametrize("P", [5, 16, 64, 100, 1024])
def test_views_reach_their_form_and_agree(P, ftn, dev):
    rt = ftn.runtime
    g = np.random.default_rng(3 + P)
    B, H, N = 2, 6, 8
    x = torch.from_numpy(g.standard_normal((P, B, H, N)).astype(np.float32)).to(dev)
    y = torch.from_numpy(g.standard_normal((B, H, N)).astype(np.float32)).to(dev)
    assert rt.path_summary_form(x, y, 2) == pc.form(P, True)
    for reduce in ("sum", "max"):
        base = ftn.score.path_summary(x, pc.LEVELS, y, window=2, reduce=reduce, want_sorted=True)
        for name, (view, quads) in _sample_views(x, dev).items():
            assert rt.path_summary_form(view, y, 2) == pc.form(P, quads), name
            got = ftn.score.path_summary(view, pc.LEVELS, y, window=2, reduce=reduce, want_sorted=True)
            assert ftn.score._last_backend == "hip"
            for k in KEYS:
                assert torch.equal(got[k], base[k]), (name, k)
        for yv, quads in zip(_views(y, dev), (False, False, True)):
            assert rt.path_summary_form(x, yv, 2) == pc.form(P, quads)
            got = ftn.score.path_summary(x, pc.LEVELS, yv, window=2, reduce=reduce, want_sorted=True)
            for k in KEYS:
                assert torch.equal(got[k], base[k]), k


@pytest.mark.parametrize("P", [5, 64, 100, 513])
def test_guard_words_around_every_output(P, ftn, dev):
    rt = ftn.runtime
    g = np.random.default_rng(5)
    sentinel = -12345.0
    for (B, H, N), window in (((1, 4, 260), 2), ((3, 7, 5), 1), ((2, 6, 8), 3)):
        x = torch.from_numpy(pc.counts(g, (P, B, H, N), 2.0)).to(dev)
        y = torch.from_numpy(pc.counts(g, (B, H, N), 2.0)).to(dev)
        Hp = H // window
        shapes = {"quantiles": (3, B, Hp, N), "mean": (B, Hp, N), "crps": (B, Hp, N), "sorted": (P, B, Hp, N)}
        want = rt.path_summary(x, pc.ranks(pc.LEVELS, P), window, "sum", y=y, want_sorted=True)
        for lead in (4, 1):                                     # 16-byte aligned outputs, and 4-byte aligned ones
            bufs, out = {}, {}
            for k, shape in shapes.items():
                n = int(np.prod(shape))
                bufs[k] = torch.full((n + 2 * lead + 3,), sentinel, device=dev)
                out[k] = bufs[k][lead:lead + n].view(shape)
            assert rt.path_summary_form(x, y, window, out.values()) == pc.form(P, N % 4 == 0 and lead == 4)
            got = rt.path_summary(x, pc.ranks(pc.LEVELS, P), window, "sum", y=y, want_sorted=True, out=out)
            for k, shape in shapes.items():
                n = int(np.prod(shape))
                assert got[k].data_ptr() == out[k].data_ptr() and torch.equal(got[k], want[k]), (k, lead)
                assert bool((bufs[k][:lead] == sentinel).all()) and bool((bufs[k][lead + n:] == sentinel).all()), k


@pytest.mark.parametrize("P", [16, 64, 257])
def test_a_column_does_not_depend_on_its_place_or_the_grid(P, ftn, dev):
    g = np.random.default_rng(17 + P)
    w = 2
    col = g.standard_normal((P, w)).astype(np.float32)          # one column: its paths and window rows
    ycol = g.standard_normal(w).astype(np.float32)
    seen = []
    for (B, H, N), places in (((1, 2, 4), [(0, 0, 1)]), ((3, 8, 8), [(0, 0, 0), (2, 3, 7), (1, 1, 5)]),
                              ((2, 4, 261), [(1, 1, 260), (0, 0, 64)]), ((5, 2, 3), [(4, 0, 2)])):
        x = g.standard_normal((P, B, H, N)).astype(np.float32)
        y = g.standard_normal((B, H, N)).astype(np.float32)
        for b, hp, n in places:
            x[:, b, hp * w:(hp + 1) * w, n] = col
            y[b, hp * w:(hp + 1) * w, n] = ycol
        for reduce in ("sum", "max"):
            got = _hip(ftn, torch.from_numpy(x).to(dev), pc.LEVELS, w, reduce, torch.from_numpy(y).to(dev))
            for b, hp, n in places:
                seen.append((reduce, tuple(got[k][..., b, hp, n].tobytes() for k in KEYS)))
    for reduce in ("sum", "max"):
        assert len({bits for r, bits in seen if r == reduce}) == 1


@pytest.mark.parametrize("P", [7, 64, 200])
def test_rank_counts_and_observations(P, ftn, dev):
    sc = ftn.score
    g = np.random.default_rng(23 + P)
    B, H, N = 2, 6, 8
    x = pc.counts(g, (P, B, H, N), 4.0)
    xd = torch.from_numpy(x).to(dev)
    only = ftn.runtime.path_summary(xd, [], 2, "sum", want_mean=True)                   # Q = 0: the mean alone
    assert only["quantiles"] is None and only["crps"] is None and only["sorted"] is None
    assert pc.same(only["mean"].cpu().numpy(), pc.summary(x, [], 2, "sum")["mean"])
    none = sc.path_summary(xd, (), window=2)
    assert sc._last_backend == "hip" and tuple(none["quantiles"].shape) == (0, B, 3, N) and "crps" not in none
    with pytest.raises(ValueError, match="no output"):
        ftn.runtime.path_summary(xd, [], 2, "sum", want_mean=False)
    for y in (x[min(2, P - 1)].copy(), np.full((B, H, N), 1e6, dtype=np.float32)):      # on a sample; far outside
        want = pc.summary(x, pc.LEVELS11, 2, "sum", y)
        got = _hip(ftn, xd, pc.LEVELS11, 2, "sum", torch.from_numpy(y).to(dev))          # 11 levels: two launches
        assert got["quantiles"].shape == (11, B, 3, N)
        _exact(got, want, (P,))
        assert float(got["crps"].min()) >= 0.0
    assert float(got["crps"].min()) > 9e5


def test_sampled_forecast_end_to_end(ftn, dev):
    fc, sc = ftn.forecast, ftn.score
    d_model, N, L, T, B, H, marks, norm, P = 64, 32, 24, 29, 1, 12, 0, "decoupled", 5
    model = _model(ftn, dev, d_model, N, L, marks, norm)
    x, kw = _inputs(dev, B, T, N, H, marks, seed=3)
    with torch.inference_mode():
        samples, rate, _ = fc.forecast_sample_paths(model, x, H, P, seed=17, **kw)
    y = torch.round(rate[0])
    for window in (None, 4, H):
        for reduce in ("sum", "max"):
            got = sc.path_summary(samples, pc.LEVELS, y, window=window, reduce=reduce)
            assert sc._last_backend == "hip"
            want = sc.path_summary(samples, pc.LEVELS, y, window=window, reduce=reduce, backend="torch")
            assert sc._last_backend == "torch"
            assert torch.equal(got["crps"], want["crps"]) and torch.equal(got["mean"], want["mean"])
            assert torch.equal(got["quantiles"], want["quantiles"])
            if reduce == "sum":
                assert torch.equal(got["quantiles"], sc.path_quantiles(samples, pc.LEVELS, window))
    m = sc.path_metrics(samples, y, pc.LEVELS, window=4, reduce="max")
    assert sc._last_backend == "hip" and int(m["count"]) == B * 3 * N and bool(torch.isfinite(m["crps"]))
    assert bool((m["coverage"][1:] >= m["coverage"][:-1]).all())


@pytest.mark.parametrize("P", [16, 100])
def test_captured_call_replays_on_new_samples(P, ftn, dev):
    sc = ftn.score
    g = torch.Generator().manual_seed(9)
    B, H, N = 2, 6, 8
    first, second = (torch.randn(P, B, H, N, generator=g).to(dev) for _ in range(2))
    y = torch.randn(B, H, N, generator=g).to(dev)
    static = first.clone()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        sc.path_summary(static, pc.LEVELS, y, window=2, want_sorted=True)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sc.path_summary(static, pc.LEVELS, y, window=2, want_sorted=True)
    assert sc._last_backend == "hip"
    for data in (second, first):
        static.copy_(data)
        graph.replay()
        eager = sc.path_summary(data, pc.LEVELS, y, window=2, want_sorted=True)
        for k in KEYS:
            assert torch.equal(out[k], eager[k]), k
