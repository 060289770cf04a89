"""``forecast.forecast_recursive_batch`` against the reference's own recursive forecast, pinned by fixtures the reference
wrote (tests/golden/make_golden_recursive.py: the reference ``TimesNet(mode="recursive")`` built on each config below
with ``torch.manual_seed(0)``, its zero-initialised heads / context maps woken up, its ``state_dict``, the inputs and
what its ``predict.forecast_recursive_batch`` returned).  On CPU tensors the drop-in runs the reference's loop over the
mirror shell; the ring-buffer device path is covered by tests/test_gpu_recursive.py."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN

# case -> (TimesNet config, input options, H)
CASES = {
    # static features, ids and the low-rank temporal context; H > 2 * input_len (the ring wraps twice), T > input_len
    "context": (dict(input_len=12, pred_len=30, d_model=16, d_ff=32, n_layers=2, k_periods=3,
                     kernel_set=[(3, 3), (5, 5)], dropout=0.0, activation="gelu", mode="recursive",
                     bottleneck_ratio=2.0, use_checkpoint=False, id_embed_dim=8, static_proj_dim=8,
                     use_zero_mean_context=True, context_rank=4, context_scale=0.05),
                dict(B=3, T=16, N=5, static=True, ids=True), 30),
    # time features through x_mark / y_mark, "layer" embedding norm; N % 4 == 0
    "marks_layer": (dict(input_len=16, pred_len=20, d_model=12, d_ff=None, n_layers=2, k_periods=3,
                         kernel_set=[(3, 3), (5, 5)], dropout=0.0, activation="relu", mode="recursive",
                         embed_norm_mode="layer", id_embed_dim=4, use_checkpoint=False),
                    dict(B=2, T=16, N=8, marks=3, ids=True), 20),
}
WAKE = 0.1


def case_inputs(name):
    """``(last_seq, kwargs, H, generator)``: the inputs a case's fixture was made on, and the generator that then woke
    the reference's zero-initialised parameters."""
    _, opt, H = CASES[name]
    B, T, N = opt["B"], opt["T"], opt["N"]
    g = torch.Generator().manual_seed(11)
    t = torch.arange(T, dtype=torch.float32).view(1, T, 1)
    x = (torch.rand(B, T, N, generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 6.0)).contiguous()
    kw = {}
    if opt.get("static"):
        kw["series_static"] = torch.randn(N, 4, generator=g)
    if opt.get("ids"):
        kw["series_ids"] = torch.tensor([4, 0, 2, 7, 1, 3, 6, 5][:N])
    if opt.get("marks"):
        kw["x_mark"] = torch.randn(B, T, opt["marks"], generator=g)
        kw["y_mark"] = torch.randn(B, H, opt["marks"], generator=g)
    return x, kw, H, g


def _fixture(name):
    with np.load(GOLDEN / f"recursive_{name}.npz") as z:
        return {k: z[k] for k in z.files}


def _part(z, prefix):
    return {k[len(prefix):]: torch.from_numpy(np.array(v)) for k, v in z.items() if k.startswith(prefix)}


def load_case(ftn, name, device="cpu"):
    """The mirror shell holding the fixture's checkpoint, and the fixture's inputs / outputs."""
    cfg, _, H = CASES[name]
    z = _fixture(name)
    x, kw = torch.from_numpy(z["x"]), _part(z, "kw:")
    with torch.no_grad():
        torch.manual_seed(1)
        model = ftn.models.TimesNet(**cfg).eval()
        model(x, **{k: v for k, v in kw.items() if k != "y_mark"})       # materialise the lazy layers
        model.load_state_dict(_part(z, "sd:"), strict=True)
    model = model.to(device)
    return model, x.to(device), {k: v.to(device) for k, v in kw.items()}, H, z


@pytest.mark.parametrize("name", list(CASES))
def test_drop_in_matches_reference_recursive_forecast(name, ftn):
    model, x, kw, H, z = load_case(ftn, name)
    with torch.no_grad():
        rate, disp = ftn.forecast.forecast_recursive_batch(model, x, H, **kw)
    assert rate.shape == disp.shape == (x.size(0), H, x.size(2))
    torch.testing.assert_close(rate, torch.from_numpy(z["rate"]), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(disp, torch.from_numpy(z["disp"]), rtol=1e-5, atol=1e-5)
    assert model.period_selector.last_selected_periods.tolist() == z["periods"].tolist()
    assert all(b._last_backend == "torch" for b in model.blocks)


def test_value_errors_carry_the_reference_messages(ftn):
    model, x, kw, H, _ = load_case(ftn, "marks_layer")
    fc = ftn.forecast.forecast_recursive_batch
    with torch.no_grad():
        with pytest.raises(ValueError, match="^Temporal features provided for history but missing future marks "
                                             "during recursive forecast$"):
            fc(model, x, H, x_mark=kw["x_mark"], series_ids=kw["series_ids"])
        with pytest.raises(ValueError, match="^y_mark does not provide enough future steps for recursive "
                                             "forecasting$"):
            fc(model, x, H, x_mark=kw["x_mark"], y_mark=kw["y_mark"][:, : H - 1], series_ids=kw["series_ids"])
        # exactly H future marks are enough (the reference reads y_mark[:, H - 1] on its last step)
        fc(model, x, H, x_mark=kw["x_mark"], y_mark=kw["y_mark"][:, :H], series_ids=kw["series_ids"])


def test_cpu_and_direct_mode_take_the_reference_loop(ftn, monkeypatch):
    F = ftn.forecast
    calls = []
    loop = F.forecast_recursive_batch_loop
    monkeypatch.setattr(F, "forecast_recursive_batch_loop", lambda *a, **k: calls.append(1) or loop(*a, **k))
    model, x, kw, H, _ = load_case(ftn, "context")
    with torch.no_grad():
        F.forecast_recursive_batch(model, x, 3, **kw)                   # CPU tensors
    assert calls == [1]
    cfg = dict(CASES["context"][0], mode="direct", pred_len=3)
    with torch.no_grad():
        torch.manual_seed(0)
        direct = ftn.models.TimesNet(**cfg).eval()
        rate, disp = F.forecast_recursive_batch(direct, x, 2, **kw)
    assert calls == [1, 1]
    # a direct-mode model returns pred_len steps per call: the loop concatenates them, as the reference's does
    assert rate.shape == (x.size(0), 2 * 3, x.size(2))


def test_loop_is_the_reference_loop(ftn):
    """The fallback concatenates the same rows the reference does: check it against a loop written out here."""
    model, x, kw, H, _ = load_case(ftn, "marks_layer")
    H = 5
    with torch.no_grad():
        rate, disp = ftn.forecast.forecast_recursive_batch_loop(model, x, H, **kw)
        seq, mark, rates = x, kw["x_mark"], []
        for s in range(H):
            r, _ = model(seq, x_mark=mark, series_ids=kw["series_ids"])
            rates.append(r)
            seq = torch.cat([seq[:, 1:], r], 1)
            mark = torch.cat([mark[:, 1:], kw["y_mark"][:, s:s + 1]], 1)
    assert torch.equal(rate, torch.cat(rates, 1))
