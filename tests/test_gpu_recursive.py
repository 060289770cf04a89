"""Device-side recursive forecasting (flow-timesnet_amd/forecast.py) on the MI355X: the two ring kernels
(``ftn_embed_rows_strided``, ``ftn_embed_ring``) against the one-pass ``ftn_embed_forward``, and the eager device path
and the HIP-graph replay against the reference's host loop over the same GPU model - bit for bit - plus the reference
fixtures, the f16x2 range repair and the finite-positive check across a whole forecast."""
import warnings

import pytest
import torch

from test_recursive_forecast import CASES, load_case

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-4, 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------- ring kernels
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("N", [64, 37])
@pytest.mark.parametrize("mode", ["none", "decoupled", "layer"])
def test_ring_equals_one_pass_embedding_of_the_rolled_window(mode, N, D, ftn, dev):
    """Fill V from a window, append k rows one at a time (the ring wraps), rebuild with head k % L: the result is
    ftn_embed_forward of the window k rows later.  N % 4 selects the kernel form (16-byte rows or not)."""
    rt = ftn.runtime
    B, L, k = 3, 24, 30
    g = torch.Generator().manual_seed(N + D)
    x = (torch.randn(B, L + k, N, generator=g) * 3.0).to(dev)
    w = (torch.randn(D, N, generator=g) / N ** 0.5).to(dev)
    add = torch.randn(B if mode == "decoupled" else 1, L, D, generator=g).to(dev).contiguous()
    ln = None
    if mode == "layer":
        ln = ((1.0 + 0.1 * torch.randn(D, generator=g)).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev), 1e-5)
    with torch.inference_mode():
        V = torch.empty(B, L, D, device=dev)
        rt.embed_rows_strided(x[:, :L], w, V, 0)
        assert torch.equal(V, rt.embed_forward(x[:, :L], w, None))
        for i in range(k):
            rt.embed_rows_strided(x[:, L + i:L + i + 1], w, V, i % L)
        got = rt.embed_ring(V, k % L, add, ln)
        want = rt.embed_forward(x[:, k:k + L], w, add, ln)
        # a 5-row append into the middle of the ring, then the full-window rebuild at head 0
        rt.embed_rows_strided(x[:, :5], w, V, 7)
        part = rt.embed_ring(V, 0, None)
    torch.cuda.synchronize()
    if mode == "layer" and N % 4 and D > 64:
        # k_embed_in<8, false> contracts its LayerNorm into FMAs differently from k_embed_ring: equal up to rounding
        # only, which is why forecast.py keeps this form on the reference loop
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
    else:
        assert torch.equal(got, want)
    assert torch.equal(part[:, 7:12], rt.embed_forward(x[:, :5], w, None))


def test_ring_entry_points_reject_bad_arguments(ftn, dev):
    rt = ftn.runtime
    V = torch.zeros(2, 8, 16, device=dev)
    with pytest.raises(ValueError, match="head"):
        rt.check(rt._lib.load().ftn_embed_ring(V.data_ptr(), 2, 8, 16, 8, None, 0, None, None, 0.0, V.data_ptr(), None),
                 "ftn_embed_ring")
    with pytest.raises(ValueError):
        rt.embed_rows_strided(torch.zeros(2, 1, 4, device=dev), torch.zeros(16, 4, device=dev), V, 8)


# ------------------------------------------------------------------------------------------- forecasts against the loop
def _model(ftn, dev, d_model, N, L, marks, norm, seed=0, **extra):
    cfg = dict(input_len=L, pred_len=4, d_model=d_model, d_ff=2 * d_model, n_layers=2, k_periods=3,
               kernel_set=[(3, 3), (5, 5)], dropout=0.0, activation="gelu", mode="recursive", use_checkpoint=False,
               embed_norm_mode=norm, id_embed_dim=4, use_zero_mean_context=True, context_rank=4)
    cfg.update(extra)
    torch.manual_seed(seed)
    m = ftn.models.TimesNet(**cfg).eval().to(dev)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(2, L, N, generator=g).to(dev) + 1.0
    kw = {"x_mark": torch.randn(2, L, marks, generator=g).to(dev)} if marks else {}
    with torch.no_grad():
        m(x, series_ids=torch.arange(N, device=dev), series_static=torch.randn(N, 3, generator=g).to(dev), **kw)
        for p in m.parameters():                                   # wake the zero-initialised heads / context maps
            if float(p.detach().abs().sum()) == 0.0:
                p.copy_((0.1 * torch.randn(p.shape, generator=g)).to(dev))
    return m


def _inputs(dev, B, T, N, H, marks, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float32).view(1, T, 1)
    x = (torch.rand(B, T, N, generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 6.0)).to(dev)
    kw = {"series_ids": torch.arange(N, device=dev), "series_static": torch.randn(N, 3, generator=g).to(dev)}
    if marks:
        kw["x_mark"] = torch.randn(B, T, marks, generator=g).to(dev)
        kw["y_mark"] = torch.randn(B, H + 2, marks, generator=g).to(dev)
    return x, kw


def _loop(model, x, H, x_mark=None, y_mark=None, **kw):
    """The reference's forecast_recursive_batch (predict.py:307-342) written out."""
    rates, disps, seq, mark = [], [], x, x_mark
    for s in range(H):
        extra = {} if mark is None else {"x_mark": mark}
        r, d = model(seq, **extra, **kw)
        rates.append(r)
        disps.append(d)
        seq = torch.cat([seq[:, 1:, :], r], dim=1)
        if mark is not None:
            mark = torch.cat([mark[:, 1:, :], y_mark[:, s:s + 1, :]], dim=1)
    return torch.cat(rates, 1), torch.cat(disps, 1)


FORECASTS = {   # name: d_model, N, L, T, B, H, marks, embed_norm_mode
    "d64_plain_b1": (64, 32, 24, 29, 1, 53, 0, "decoupled"),
    "d128_marks_b3": (128, 40, 24, 24, 3, 30, 3, "decoupled"),
    "d64_marks_layer_b5_n37": (64, 37, 20, 26, 5, 45, 2, "layer"),
    "d128_none_b3": (128, 16, 16, 20, 3, 20, 0, "none"),
}


@pytest.mark.parametrize("name", list(FORECASTS))
def test_device_path_and_replay_equal_the_loop(name, ftn, dev):
    d_model, N, L, T, B, H, marks, norm = FORECASTS[name]
    F = ftn.forecast
    model = _model(ftn, dev, d_model, N, L, marks, norm)
    x, kw = _inputs(dev, B, T, N, H, marks, seed=5)
    x2, kw2 = _inputs(dev, B, T, N, H, marks, seed=6)
    with torch.inference_mode():
        want_r, want_d = _loop(model, x, H, **kw)
        want_p = model.period_selector.last_selected_periods.tolist()
        got_r, got_d = F.forecast_recursive_batch(model, x, H, **kw)
        got_p = model.period_selector.last_selected_periods.tolist()
        assert model._last_embed_backend == "hip" and model._last_head_backend == "hip"
        assert all(b._last_backend == "hip" for b in model.blocks)
        fc = F.RecursiveForecaster(model, x, H, **kw)
        marks_kw = {k: kw[k] for k in ("x_mark", "y_mark") if k in kw}
        rep_r, rep_d = fc(x, **marks_kw)
        rep_r, rep_d = rep_r.clone(), rep_d.clone()
        rep_p = model.period_selector.last_selected_periods.tolist()
        want2_r, want2_d = _loop(model, x2, H, **{**kw2, "series_ids": kw["series_ids"],
                                                  "series_static": kw["series_static"]})
        want2_p = model.period_selector.last_selected_periods.tolist()
        marks_kw2 = {k: kw2[k] for k in ("x_mark", "y_mark") if k in kw2}
        rep2_r, rep2_d = fc(x2, **marks_kw2)
        rep2_p = model.period_selector.last_selected_periods.tolist()
    torch.cuda.synchronize()
    assert got_r.shape == (B, H, N)
    assert torch.equal(got_r, want_r) and torch.equal(got_d, want_d)
    assert torch.equal(rep_r, want_r) and torch.equal(rep_d, want_d)
    assert torch.equal(rep2_r, want2_r) and torch.equal(rep2_d, want2_d)
    assert got_p == want_p and rep_p == want_p and rep2_p == want2_p
    assert fc.inputs[0].data_ptr() != x2.data_ptr()


def test_layer_mode_fp32_embedding_form_takes_the_loop(ftn, dev, monkeypatch):
    F = ftn.forecast
    model = _model(ftn, dev, 128, 37, 16, 0, "layer")
    x, kw = _inputs(dev, 3, 20, 37, 6, 0, seed=5)
    calls = []
    loop = F.forecast_recursive_batch_loop
    monkeypatch.setattr(F, "forecast_recursive_batch_loop", lambda *a, **k: calls.append(1) or loop(*a, **k))
    with torch.inference_mode():
        got_r, _ = F.forecast_recursive_batch(model, x, 6, **kw)
        want_r, _ = _loop(model, x, 6, **kw)
    assert calls == [1] and torch.equal(got_r, want_r)


@pytest.mark.parametrize("name", list(CASES))
def test_reference_fixtures_on_the_device(name, ftn, dev):
    model, x, kw, H, z = load_case(ftn, name, dev)
    with torch.inference_mode():
        rate, disp = ftn.forecast.forecast_recursive_batch(model, x, H, **kw)
        periods = model.period_selector.last_selected_periods.tolist()
    assert model._last_embed_backend == "hip" and model._last_head_backend == "hip"
    torch.testing.assert_close(rate.cpu(), torch.from_numpy(z["rate"]), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(disp.cpu(), torch.from_numpy(z["disp"]), rtol=RTOL, atol=ATOL)
    assert periods == z["periods"].tolist()


# --------------------------------------------------------------------------------------------------------- the checks
@pytest.mark.parametrize("graphed", [False, True])
def test_out_of_fp16_range_forecast_is_repeated_on_bf16x3(graphed, ftn, dev):
    """Hidden values past the fp16 range (the first 1x1 of every branch of block 0 scaled, as in test_gpu_range.py)
    trip the f16x2 guard inside the forecast: the caller gets the forecast of a model whose blocks all run bf16x3 (and
    a RuntimeWarning), never the unrepaired one."""
    F = ftn.forecast
    model = _model(ftn, dev, 64, 32, 24, 0, "decoupled", seed=3, d_ff=256, bottleneck_ratio=4.0)
    safe = _model(ftn, dev, 64, 32, 24, 0, "decoupled", seed=3, d_ff=256, bottleneck_ratio=4.0)
    with torch.no_grad():
        for m in (model, safe):
            for name, p in m.named_parameters():
                if name.startswith("blocks.0.inception.0.paths.") and name.endswith("branch.0.weight"):
                    p.mul_(3e5)
    for b in safe.blocks:
        b.engine = "bf16x3"
    x, kw = _inputs(dev, 3, 24, 32, 30, 0, seed=9)
    with torch.inference_mode():
        want_r, want_d = _loop(safe, x, 30, **kw)
        with pytest.warns(RuntimeWarning, match="fp16 range"):
            if graphed:
                got_r, got_d = F.RecursiveForecaster(model, x, 30, **kw)(x)
            else:
                got_r, got_d = F.forecast_recursive_batch(model, x, 30, **kw)
    torch.cuda.synchronize()
    assert all(b.engine == "bf16x3" for b in model.blocks)
    assert all(not b.range_flag_on_device for b in model.blocks) and not model._defer_checks
    assert torch.equal(got_r, want_r) and torch.equal(got_d, want_d)


@pytest.mark.parametrize("graphed", [False, True])
def test_non_finite_forecast_raises_the_reference_error(graphed, ftn, dev):
    F = ftn.forecast
    model = _model(ftn, dev, 64, 32, 24, 0, "decoupled", seed=4)
    x, kw = _inputs(dev, 2, 24, 32, 12, 0, seed=10)
    bad = x.clone()
    bad[1, -3, 5] = float("inf")
    with torch.inference_mode(), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        if graphed:
            fc = F.RecursiveForecaster(model, x, 12, **kw)
            with pytest.raises(RuntimeError, match="^Predicted rate must be finite and strictly positive$"):
                fc(bad)
        else:
            with pytest.raises(RuntimeError, match="^Predicted rate must be finite and strictly positive$"):
                F.forecast_recursive_batch(model, bad, 12, **kw)
    assert not model._defer_checks and model._pending_bad is None
