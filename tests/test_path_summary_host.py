"""Path summaries without a GPU: the torch backend of ``score.path_summary`` against the numpy oracle of
tests/paths_checks.py, ``path_metrics`` against a direct numpy computation, and every error case."""
import numpy as np
import pytest
import torch

import paths_checks as pc


def _run(ftn, x, levels, window, reduce, y=None):
    out = ftn.score.path_summary(torch.from_numpy(x), levels, None if y is None else torch.from_numpy(y),
                                 window=window, reduce=reduce, want_sorted=True)
    assert ftn.score._last_backend == "torch"
    return {k: v.numpy() for k, v in out.items()}


def _check(got, want, exact):
    P = want["sorted"].shape[0]
    assert got["quantiles"].dtype == np.float32 and got["mean"].dtype == np.float32
    assert pc.same(got["sorted"], want["sorted"]) and pc.same(got["quantiles"], want["quantiles"])
    if exact:
        assert pc.same(got["mean"], want["mean"]) and pc.same(got["crps"], want["crps"])
    else:
        assert pc.within_ulp(got["mean"], want["sorted"].astype(np.float64).sum(0) / P, want["mean_scale"])
        assert pc.within_ulp(got["crps"], want["crps64"], want["scale"])


@pytest.mark.parametrize("reduce", ["sum", "max"])
@pytest.mark.parametrize("P", [1, 2, 5, 13, 64, 100])
def test_torch_backend_against_numpy(P, reduce, ftn):
    g = np.random.default_rng(100 + P)
    B, H, N = 2, 6, 5
    for window in (None, 1, 2, H):
        w = 1 if window is None else window
        for kind in ("counts", "big", "real"):
            if kind == "counts":
                x, y = pc.counts(g, (P, B, H, N), 1.5), pc.counts(g, (B, H, N), 1.5)
            elif kind == "big":
                x, y = pc.big_counts(g, (P, B, H, N), w), pc.big_counts(g, (B, H, N), w)
            else:
                x = g.standard_normal((P, B, H, N)).astype(np.float32)
                y = g.standard_normal((B, H, N)).astype(np.float32)
            want = pc.summary(x, pc.LEVELS, window, reduce, y)
            got = _run(ftn, x, pc.LEVELS, window, reduce, y)
            assert got["quantiles"].shape == (3, B, H // w, N) and got["sorted"].shape == (P, B, H // w, N)
            _check(got, want, exact=kind != "real")
            if kind == "counts":
                assert float(np.abs(want["crps"]).max()) > 0.0 or P == 1


def test_special_values(ftn):
    g = np.random.default_rng(7)
    P, B, H, N = 9, 2, 4, 3
    x = pc.counts(g, (P, B, H, N), 3.0)
    y = pc.counts(g, (B, H, N), 3.0)
    x[4, 0, 1, 2] = np.nan                                      # a NaN path in one column
    x[:, 1, 2, 0] = np.nan                                      # an all-NaN column
    x[2, 1, 0, 1] = np.inf
    x[3, 0, 3, 0] = -np.inf
    y[0, 0, 0] = np.nan
    for reduce in ("sum", "max"):
        for window in (None, 2, 4):
            want = pc.summary(x, pc.LEVELS, window, reduce, y)
            got = _run(ftn, x, pc.LEVELS, window, reduce, y)
            _check(got, want, exact=True)
    s = _run(ftn, x, [0.999], None, "sum", y)
    assert np.isnan(s["sorted"][-1, 0, 1, 2]) and not np.isnan(s["sorted"][-2, 0, 1, 2])      # NaN sorts last
    assert np.isnan(s["quantiles"][0, 0, 1, 2]) and np.isnan(s["mean"][0, 1, 2]) and np.isnan(s["crps"][0, 1, 2])
    assert np.isnan(s["sorted"][:, 1, 2, 0]).all()
    assert np.isinf(s["sorted"][-1, 1, 0, 1]) and np.isinf(s["sorted"][0, 0, 3, 0])
    assert np.isnan(s["crps"][0, 0, 0]) and not np.isnan(s["mean"][0, 0, 0])                   # y NaN: the CRPS alone


def test_crps_known_values(ftn):
    x = np.array([1.0, 3.0, 2.0, 6.0], dtype=np.float32).reshape(4, 1, 1, 1)
    for yv, want in ((2.0, 0.5), (100.0, 96.0)):
        # (1/P) sum |x - y| - (1/(2 P^2)) sum sum |x - x'|, the double sum 2 (2 + 1 + 5 + 1 + 3 + 4) / 32 = 1
        s = _run(ftn, x, [], None, "sum", np.full((1, 1, 1), yv, dtype=np.float32))
        direct = np.abs(x - yv).mean() - np.abs(x[:, None] - x[None]).sum() / 32.0
        assert float(s["crps"][0, 0, 0]) == np.float32(direct) == np.float32(want)
        assert s["quantiles"].shape == (0, 1, 1, 1) and float(s["mean"][0, 0, 0]) == 3.0
    one = _run(ftn, x[:1], [0.3], None, "max", np.ones((1, 1, 1), dtype=np.float32))           # P = 1, y on it
    assert float(one["crps"][0, 0, 0]) == 0.0 and float(one["quantiles"][0, 0, 0, 0]) == 1.0


def test_quantiles_are_path_quantiles(ftn):
    g = np.random.default_rng(11)
    x = torch.from_numpy(pc.counts(g, (13, 2, 6, 3), 4.0))
    for window in (None, 2, 3, 6):
        q = ftn.score.path_summary(x, pc.LEVELS11, window=window)["quantiles"]
        assert torch.equal(q, ftn.score.path_quantiles(x, pc.LEVELS11, window))
    half = ftn.score.path_summary(x.double(), [0.5], window=2)                                 # another dtype: torch
    assert ftn.score._last_backend == "torch" and half["quantiles"].dtype == torch.float32
    assert torch.equal(half["quantiles"], ftn.score.path_quantiles(x, [0.5], 2))
    assert "crps" not in half and "sorted" not in half


def _metrics_numpy(x, y, levels, window, reduce, mask):
    s = pc.summary(x, levels, window, reduce, y)
    w = 1 if window is None else window
    B, H, N = y.shape
    valid = np.isfinite(s["yw"]) & np.isfinite(s["quantiles"]).all(0) & np.isfinite(s["crps"])
    if mask is not None:
        valid &= mask.reshape(B, H // w, w, N).all(2)
    n = max(int(valid.sum()), 1)
    cov, pin = [], []
    for i, q in enumerate(levels):
        d = (s["yw"] - s["quantiles"][i])[valid].astype(np.float64)
        cov.append((d <= 0).sum() / n)
        pin.append(np.maximum(q * d, (q - 1.0) * d).sum() / n)
    return np.array(cov), np.array(pin), s["crps"][valid].astype(np.float64).sum() / n, int(valid.sum())


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_path_metrics_against_numpy(reduce, ftn):
    g = np.random.default_rng(21)
    P, B, H, N = 24, 3, 6, 4
    x, y = pc.counts(g, (P, B, H, N), 5.0), pc.counts(g, (B, H, N), 5.0)
    x[3, 1, 2, 1] = np.nan
    y[2, 5, 3] = np.inf
    mask = g.random((B, H, N)) > 0.2
    for window in (None, 3):
        for m in (None, mask):
            cov, pin, crps, count = _metrics_numpy(x, y, pc.LEVELS, window, reduce, m)
            got = ftn.score.path_metrics(torch.from_numpy(x), torch.from_numpy(y), pc.LEVELS, window, reduce,
                                         None if m is None else torch.from_numpy(m))
            assert int(got["count"]) == count and 0 < count < B * H * N
            np.testing.assert_allclose(got["coverage"].numpy(), cov, rtol=1e-6)
            np.testing.assert_allclose(got["pinball"].numpy(), pin, rtol=1e-5)
            np.testing.assert_allclose(float(got["crps"]), crps, rtol=1e-5)


def test_errors(ftn):
    sc = ftn.score
    x, y = torch.ones(4, 2, 6, 3), torch.ones(2, 6, 3)
    for bad in ([0.0], [1.0], [0.5, 1.5]):
        with pytest.raises(ValueError, match="level"):
            sc.path_summary(x, bad)
    with pytest.raises(ValueError, match="window"):
        sc.path_summary(x, [0.5], window=4)
    with pytest.raises(ValueError, match="window"):
        sc.path_summary(x, [0.5], window=0)
    with pytest.raises(ValueError, match="y must be"):
        sc.path_summary(x, [0.5], y[:, :, :2])
    with pytest.raises(ValueError, match="hip"):
        sc.path_summary(x, [0.5], backend="hip")
    with pytest.raises(ValueError, match="backend"):
        sc.path_summary(x, [0.5], backend="numpy")
    with pytest.raises(ValueError, match="reduce"):
        sc.path_summary(x, [0.5], reduce="mean")
    with pytest.raises(ValueError, match="samples"):
        sc.path_summary(x[0], [0.5])
    with pytest.raises(ValueError, match="no levels"):
        sc.path_metrics(x, y, [])
    with pytest.raises(ValueError, match="mask"):
        sc.path_metrics(x, y, [0.5], mask=torch.ones(2, 6))
    assert sc.PATHS_MAX == ftn.lib.FTN_PATHS_MAX == 1024
