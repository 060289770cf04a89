"""The late-bias refit end to end on the MI355X, on the tiny model with ids and statics of
tests/test_late_fit_host.py in both window layouts (N = 1: the series layout, the series rows per item; N = 5: the wide
layout, one block of rows for the batch): ``fit.output_nll`` with ``late=fit.late_bias(...)`` against fp64 autograd
within the composed bound, ``fit.GraphedCachedStep(..., late_bias=True)`` against the eager backward bit for bit,
``fit.refit_output_cached(..., late_bias=True)`` against the eager loop with the same ``fit.DeviceAdamWList``, a row
list outside the cache, the launch list of the step with ``late_bias=False``, and the forecast after the refit."""
import copy

import pytest
import torch

import late_fit_oracle
import output_fit_oracle
from test_late_fit_host import late_model, late_params

pytestmark = pytest.mark.gpu

L, H, BATCH = 24, 4, 4
SETTINGS = dict(weight_decay=0.01, grad_clip=0.05, use_loss_mask=True)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _windows(ftn, N, dev, T=39, **kw):
    """12 items in batches of 4.  N = 1: the series layout; N = 5: the wide layout; statics [N, 3] and ids [N]."""
    g = torch.Generator().manual_seed(31 + N)
    t = torch.arange(T, dtype=torch.float32).view(T, 1)
    table = torch.poisson(2.0 + torch.sin(2 * torch.pi * t / 6.0) + torch.rand(T, N, generator=g), generator=g)
    valid = (torch.rand(T, N, generator=g) >= 0.2).float()
    return ftn.windows.DeviceWindows(table.to(dev), L, H, valid_mask=valid.to(dev), batch_size=BATCH,
                                     layout="series" if N == 1 else "wide",
                                     series_static=torch.randn(N, 3, generator=g), series_ids=torch.arange(N), **kw)


def _model(ftn, N, dev, win):
    model = late_model(ftn, N, dev)[0]
    xb, _, _, x_mark, _, static, ids = ftn.score._unpack_batch(win.batch(0))
    model.output_inputs(xb, x_mark, static, ids)
    return model


def _eleven(ftn, model):
    return ftn.fit._refit_params(model) + late_params(model)


def _clones(ftn, model):
    return [p.detach().clone() for p in _eleven(ftn, model)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("N", [1, 5])
def test_output_nll_gives_all_eleven_gradients(N, ftn, dev):
    """The six of the output side inside the bound of tests/output_fit_oracle.py (the late bias enters it as the
    fp32 values the kernel made), the five of the head inside the bound of tests/late_fit_oracle.py with d_pre charged
    the forward's roundings E = 64 (D + 8 + L + 8) and its own three products."""
    fit = ftn.fit
    win = _windows(ftn, N, dev)
    model = _model(ftn, N, dev, win)
    xb, yb, mask, x_mark, _, static, ids = ftn.score._unpack_batch(win.batch(1))
    seq, tail, hist, late0, floor = model.output_inputs(xb, x_mark, static, ids)
    rows = model.late_rows(xb, x_mark, static, ids)
    assert rows.shape[0] == (BATCH if N == 1 else 1) and rows.shape[1] == N
    six, five = fit._refit_params(model), late_params(model)
    for p in six + five:
        p.requires_grad_(True)
        p.grad = None
    proj = model.forecast_time_proj
    eps = model.late_bias_norm.eps
    assert eps == late_fit_oracle.EPS
    late = fit.late_bias(rows, *five, eps)
    assert fit._last_late_backend == "hip" and torch.equal(late.detach(), late0)
    base = mask[:, :H, :] > 0.0
    loss, bad = fit.output_nll(seq, proj.weight[-H:], proj.bias[-H:], *six[:4], tail, hist, yb[:, :H, :], base, late,
                               floor, model.min_sigma)
    assert fit._last_head_backend == "hip" and fit._last_timeproj_backend == "hip"
    loss.backward()
    assert int(bad) == 0
    cpu = lambda t: None if t is None else t.detach().cpu()
    order6 = [proj.weight[-H:], proj.bias[-H:]] + six[:4]
    got6 = [proj.weight.grad[-H:], proj.bias.grad[-H:]] + [p.grad for p in six[:4]]
    valid = cpu(base).double()
    args = (fit, cpu(seq), [cpu(p) for p in order6], cpu(tail), hist, cpu(yb[:, :H, :]), valid)
    _, want6, bounds6 = output_fit_oracle.grads_and_bounds(*args, cpu(late), cpu(floor), model.min_sigma)
    f6 = output_fit_oracle.fraction(got6, want6, bounds6)
    # the five: fp64 autograd through the whole composition, d_pre = dloss / dlate in fp64
    p64 = [cpu(p).double() for p in order6]
    l64 = late_fit_oracle.late64(cpu(rows), [cpu(p).double() for p in five]).requires_grad_()
    loss64 = output_fit_oracle.loss64(fit, cpu(seq), p64, cpu(tail), hist, cpu(yb[:, :H, :]), valid, l64, cpu(floor),
                                      model.min_sigma)[0]
    d_pre = torch.autograd.grad(loss64, l64)[0]                   # [1, S, N] where one block serves the batch: its sum
    D = seq.shape[2]
    E = 64 * (D + 8 + L + 8) + 3
    # (+ BATCH: the additions of that batch sum, which the oracle cannot see in a d_pre of one row)
    want5, bounds5 = late_fit_oracle.grads_and_bounds(cpu(rows), [cpu(p) for p in five], d_pre, extra=E + BATCH)
    f5 = late_fit_oracle.fraction([p.grad for p in five], want5, bounds5)
    print(f"LATEFIT_ERR end to end N={N}: fraction of the bound: six {f6:.4f} five {f5:.4f}")
    assert f6 <= 1.0 and f5 <= 1.0


@pytest.mark.parametrize("N", [1, 5])
def test_graphed_step_has_the_bits_of_the_eager_backward(N, ftn, dev):
    fit = ftn.fit
    win = _windows(ftn, N, dev)
    model = _model(ftn, N, dev, win)
    cache = fit.OutputCache(model, win, use_loss_mask=True, late_bias=True)
    assert cache.late is None and cache.late_per_item == (N == 1)
    assert cache.rows.shape == ((12, 12) if N == 1 else (1, 5, 12))
    assert fit.OutputCache.bytes_needed(model, win, True, late_bias=True) == cache.nbytes
    params = _eleven(ftn, model)
    opt = fit.DeviceAdamWList(params, lr=0.0, max_norm=0.05)    # lr 0, no decay: the parameters stay
    step = fit.GraphedCachedStep(cache, model, opt, BATCH, late_bias=True)
    rows = torch.tensor([7, 2, 7, 11], device=dev)
    step.step(rows)
    torch.cuda.synchronize()
    got = [g.clone() for g in step.grads]
    assert len(got) == 11
    for p in params:
        p.requires_grad_(True)
        p.grad = None
    tail, y, mask, _ = cache.select(rows)
    proj = model.forecast_time_proj
    loss, _ = fit.output_nll(cache.seq, proj.weight[-H:], proj.bias[-H:], *params[:4], tail, cache.hist, y, mask,
                             cache.late_of(model, rows), cache.floor, cache.min_sigma, rows=rows)
    loss.backward()
    assert torch.equal(loss.detach().reshape(1), step.loss)
    for k, (p, g) in enumerate(zip(params, got)):
        assert torch.equal(p.grad, g), k
    for p in params:
        p.requires_grad_(False)


@pytest.mark.parametrize("N", [1, 5])
def test_cached_refit_ends_on_the_bits_of_the_eager_loop(N, ftn, dev):
    fit = ftn.fit
    win = _windows(ftn, N, dev)
    model = _model(ftn, N, dev, win)
    twin, before = copy.deepcopy(model), _clones(ftn, model)
    got = fit.refit_output_cached(model, win, epochs=2, lr=[1e-2, 5e-3], late_bias=True, **SETTINGS)
    assert fit._last_optim_backend == "hip" and got.shape == (6,)
    want = fit.refit_output_cached(twin, win, epochs=2, lr=[1e-2, 5e-3], late_bias=True, graphed=False, **SETTINGS)
    assert torch.equal(got, want) and _same(_clones(ftn, model), _clones(ftn, twin))
    assert not any(torch.equal(a, b) for a, b in zip(before, _clones(ftn, model)))   # all eleven moved
    moved = {id(p) for p in _eleven(ftn, model)}
    for (name, p), q in zip(model.named_parameters(), twin.parameters()):
        assert torch.equal(p, q), name
    base = late_model(ftn, N, dev)[0]
    for (name, p), q in zip(model.named_parameters(), base.parameters()):
        assert torch.equal(p, q) == (id(p) not in moved), name
    # after the refit the model's own forward uses the moved head: its late bias is that of the cached rows
    xb, _, _, x_mark, _, static, ids = ftn.score._unpack_batch(win.batch(0))
    hidden, tail, hist, late, floor = model.head_inputs(xb, x_mark, static, ids)
    again = fit.late_bias(model.late_rows(xb, x_mark, static, ids), *late_params(model), model.late_bias_norm.eps)
    assert torch.equal(late, again.detach())
    assert not torch.equal(late, base.head_inputs(xb, x_mark, static, ids)[3])
    with torch.inference_mode():
        rate, disp = model(xb, x_mark, static, ids)[:2]
    w_mu, b_mu, w_sg, b_sg = (p.detach() for p in fit._refit_params(model)[:4])
    rate2, disp2, _ = ftn.runtime.head_forward(hidden, w_mu, b_mu, w_sg, b_sg, tail.contiguous(), hist, again.detach(),
                                               floor, model.min_sigma)
    assert torch.equal(rate, rate2) and torch.equal(disp, disp2)


def test_a_row_outside_the_cache_skips_the_step(ftn, dev, monkeypatch):
    fit = ftn.fit
    win = _windows(ftn, 1, dev)
    model = _model(ftn, 1, dev, win)
    real = fit.GraphedCachedStep.step

    def bent(self, rows):
        rows = rows.clone()
        rows[1] = 10 ** 6
        return real(self, rows)

    monkeypatch.setattr(fit.GraphedCachedStep, "step", bent)
    before = _clones(ftn, model)
    with pytest.raises(IndexError, match="outside the cache"):
        fit.refit_output_cached(model, win, epochs=1, lr=1e-2, late_bias=True, **SETTINGS)
    assert _same(before, _clones(ftn, model))


def test_errors_and_the_unchanged_step_without_the_flag(ftn, dev, monkeypatch):
    """A model without the head; a cache and a step that disagree on the flag; and with ``late_bias=False`` the
    captured step makes the launches it made before, in their order, on six tensors."""
    fit, rt = ftn.fit, ftn.runtime
    win = _windows(ftn, 5, dev)
    plain = late_model(ftn, 5, dev, head=False)[0]
    xb, _, _, x_mark, _, static, ids = ftn.score._unpack_batch(win.batch(0))
    plain.output_inputs(xb, x_mark, static, ids)
    with pytest.raises(ValueError, match="no late-bias head"):
        fit.refit_output_cached(plain, win, late_bias=True)
    with pytest.raises(ValueError, match="no late-bias head"):
        fit.OutputCache(plain, win, late_bias=True)
    model = _model(ftn, 5, dev, win)
    cache = fit.OutputCache(model, win)
    with pytest.raises(ValueError, match="late_bias must be that of the cache"):
        fit.GraphedCachedStep(cache, model, fit.DeviceAdamWList(_eleven(ftn, model)), BATCH, late_bias=True)
    with pytest.raises(ValueError, match="late_bias must be that of the cache"):
        fit.refit_output_cached(model, win, cache=cache, late_bias=True)
    calls = []
    names = ("refit_rows_gather", "timeproj_forward", "head_fit_forward", "nb_nll_grad", "head_backward",
             "timeproj_backward", "refit_update", "refit_update_list", "late_fit_forward", "late_backward")
    for name in names:
        def spy(*a, _f=getattr(rt, name), _n=name, **kw):
            calls.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(rt, name, spy)
    opt = fit.DeviceAdamW(fit._refit_params(model), lr=1e-2)
    fit.GraphedCachedStep(cache, model, opt, BATCH, warmup=1)
    assert calls == list(names[:7]) * 2                          # the warm-up, then the capture
    assert cache.late is not None and cache.rows is None and not cache.late_bias
