"""The cached refit on the device: ``fit.OutputCache``, ``fit.GraphedCachedStep`` and ``fit.refit_output_cached`` on
the tiny model of ``test_gpu_fit.py``.  Both sides of every comparison are the same launches on the same operands, or
differ in addressing only, so every comparison is ``torch.equal``."""
import copy

import pytest
import torch

from test_gpu_fit import _tiny_model

pytestmark = pytest.mark.gpu

L, H, BATCH = 24, 4, 4
SETTINGS = dict(weight_decay=0.01, grad_clip=0.05, use_loss_mask=True)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _windows(ftn, N, dev, T=40, **kw):
    """N = 1: the series layout with statics and ids (the late bias is per item); N = 5: the wide layout.  T = 40:
    13 items, the last batch is short; T = 39: 12 items."""
    g = torch.Generator().manual_seed(21 + N)
    t = torch.arange(T, dtype=torch.float32).view(T, 1)
    table = torch.poisson(2.0 + torch.sin(2 * torch.pi * t / 6.0) + torch.rand(T, N, generator=g), generator=g)
    valid = (torch.rand(T, N, generator=g) >= 0.2).float()
    extra = dict(layout="series", series_static=torch.tensor([[0.5, -1.0]]),
                 series_ids=torch.zeros(1, dtype=torch.int64)) if N == 1 else dict(layout="wide")
    return ftn.windows.DeviceWindows(table.to(dev), L, H, valid_mask=valid.to(dev), batch_size=BATCH, **extra, **kw)


def _model(ftn, N, dev, win):
    model = _tiny_model(ftn, N, dev)[0]
    xb, _, _, x_mark, _, static, ids = ftn.score._unpack_batch(win.batch(0))
    model.output_inputs(xb, x_mark, static, ids)               # the lazy layers as these windows need them
    return model


def _six(ftn, model):
    return [p.detach().clone() for p in ftn.fit._refit_params(model)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _block_calls(model):
    return [b._hip_calls for b in model.blocks]


@pytest.mark.parametrize("N", [1, 5])
def test_fill_is_the_canonical_batches(N, ftn, dev):
    fit, _unpack_batch = ftn.fit, ftn.score._unpack_batch
    win = _windows(ftn, N, dev)
    model = _model(ftn, N, dev, win)
    assert win.n_items == 13 and len(win) == 4
    cache = fit.OutputCache(model, win, use_loss_mask=True)
    assert all(b._last_backend == "hip" for b in model.blocks)
    assert cache.late is not None and cache.late_per_item == (N == 1)
    assert cache.late.shape == ((13, H, 1) if N == 1 else (1, H, 5))
    assert fit.OutputCache.bytes_needed(model, win, True) == cache.nbytes
    for i in range(len(win)):
        k0, k1 = i * BATCH, min(i * BATCH + BATCH, 13)
        xb, yb, mask, x_mark, _, static, ids = _unpack_batch(win.batch(i))
        seq, tail, hist, late, floor = model.output_inputs(xb, x_mark, static, ids)
        assert hist == cache.hist == H and cache.steps == H
        assert torch.equal(cache.seq[k0:k1], seq) and torch.equal(cache.tail[k0:k1], tail)
        assert torch.equal(cache.y[k0:k1], yb) and torch.equal(cache.mask[k0:k1], (mask > 0).float())
        assert torch.equal(cache.late[k0:k1] if N == 1 else cache.late, late.expand(k1 - k0 if N == 1 else 1, -1, -1))
        assert (floor is None) == (cache.floor is None)
    # a training loader fills through gather(arange): the same stores
    shuf = _windows(ftn, N, dev, shuffle=True, drop_last=True, seed=5)
    again = fit.OutputCache(model, shuf, use_loss_mask=True)
    assert _same((cache.seq, cache.tail, cache.y, cache.mask, cache.late),
                 (again.seq, again.tail, again.y, again.mask, again.late))


@pytest.mark.parametrize("N,T", [(5, 39), (5, 40), (1, 39), (1, 40)])
def test_unshuffled_cached_refit_has_the_bits_of_the_graphed_refit(N, T, ftn, dev):
    """``shuffle=False``: an epoch's batches are the canonical ones, so the cached loop repeats
    ``refit_output_graphed``'s operands - with 13 items the short last batch takes the eager step on both sides."""
    fit = ftn.fit
    win = _windows(ftn, N, dev, T=T)
    model = _model(ftn, N, dev, win)
    twin, before = copy.deepcopy(model), _six(ftn, model)
    assert win.n_items == (12 if T == 39 else 13)
    got = fit.refit_output_cached(model, win, epochs=2, lr=[1e-2, 5e-3], **SETTINGS)
    assert fit._last_optim_backend == "hip"
    want = fit.refit_output_graphed(twin, win, epochs=2, lr=[1e-2, 5e-3], **SETTINGS)
    assert got.shape == (2 * len(win),) and torch.equal(got, want)
    assert _same(_six(ftn, model), _six(ftn, twin))
    assert not any(torch.equal(a, b) for a, b in zip(before, _six(ftn, model)))      # and all six moved


@pytest.mark.parametrize("N", [1, 5])
def test_shuffled_cached_refit_is_the_eager_loop_on_the_cache(N, ftn, dev):
    fit = ftn.fit
    win = _windows(ftn, N, dev, shuffle=True, drop_last=True, seed=7)
    model = _model(ftn, N, dev, win)
    twin = copy.deepcopy(model)
    cache = fit.OutputCache(model, win, use_loss_mask=True)
    calls = _block_calls(model)
    got = fit.refit_output_cached(model, win, epochs=3, lr=[1e-2, 5e-3, 2e-3], cache=cache, **SETTINGS)
    assert _block_calls(model) == calls and win.epoch == 3     # no block ran after the fill
    assert got.shape == (9,)
    params = fit._refit_params(twin)
    for p in params:
        p.requires_grad_(True)
    opt = fit.DeviceAdamW(params, weight_decay=0.01, max_norm=0.05)
    proj, want = twin.forecast_time_proj, []
    orders = []
    for e, lr in enumerate((1e-2, 5e-3, 2e-3)):
        opt.set_lr(lr)
        order = win.order(e)
        orders.append(order)
        for i in range(len(win)):
            rows = order[i * BATCH:(i + 1) * BATCH]
            pick = lambda t: t.index_select(0, rows)
            opt.zero_grad(set_to_none=True)
            loss, bad = fit.output_nll(pick(cache.seq), proj.weight[-H:], proj.bias[-H:], *params[:4], pick(cache.tail),
                                       cache.hist, pick(cache.y), pick(cache.mask) > 0,
                                       pick(cache.late) if cache.late_per_item else cache.late, cache.floor,
                                       twin.min_sigma)
            loss.backward()
            opt.step(loss=loss.detach(), skip=[bad])
            want.append(loss.detach().reshape(1))
    assert not torch.equal(orders[0], orders[1]) and not torch.equal(orders[0], torch.arange(13, device=dev))
    assert torch.equal(got, torch.cat(want).cpu())
    assert _same(_six(ftn, model), _six(ftn, twin))


@pytest.mark.parametrize("N", [1, 5])
def test_captured_gradients_are_the_eager_ones(N, ftn, dev):
    fit = ftn.fit
    win = _windows(ftn, N, dev)
    model = _model(ftn, N, dev, win)
    cache = fit.OutputCache(model, win, use_loss_mask=True)
    params = fit._refit_params(model)
    before = _six(ftn, model)
    step = fit.GraphedCachedStep(cache, model, fit.DeviceAdamW(params, lr=0.0), BATCH)
    assert _same(before, _six(ftn, model))                     # the warm-up moved nothing
    rows = torch.tensor([12, 0, 7, 7], device=dev)
    loss = step.step(rows).clone()
    assert torch.equal(step.rows, rows) and int(step.status) == 0
    for p in params:
        p.requires_grad_(True)
    tail, y, mask, late = cache.select(rows)
    want, bad = fit.output_nll(cache.seq, model.forecast_time_proj.weight[-H:], model.forecast_time_proj.bias[-H:],
                               *params[:4], tail, cache.hist, y, mask, late, cache.floor, model.min_sigma, rows=rows)
    assert fit._last_timeproj_backend == "hip" and fit._last_head_backend == "hip" and int(bad) == 0
    want.backward()
    assert torch.equal(loss.reshape(()), want.detach())
    assert _same(step.grads, [p.grad for p in params])
    for p in params:
        p.requires_grad_(False)
        p.grad = None


def test_a_reused_cache_runs_no_block_and_notices_a_changed_backbone(ftn, dev):
    fit = ftn.fit
    win = _windows(ftn, 5, dev, shuffle=True, seed=2)
    model = _model(ftn, 5, dev, win)
    cache = fit.OutputCache(model, win)
    calls = _block_calls(model)
    a = fit.refit_output_cached(model, win, epochs=1, lr=1e-2, cache=cache)
    b = fit.refit_output_cached(model, win, epochs=1, lr=1e-3, cache=cache)
    assert _block_calls(model) == calls and a.shape == b.shape == (4,) and win.epoch == 2
    cache.check(model)                                          # eight steps of the six tensors later
    with torch.no_grad():
        next(model.blocks[0].inception.parameters()).mul_(1.0)
    with pytest.raises(ValueError, match="the backbone changed since the cache was filled"):
        fit.refit_output_cached(model, win, cache=cache)


def test_a_row_outside_the_cache_skips_the_step(ftn, dev):
    fit = ftn.fit
    win = _windows(ftn, 5, dev)
    model = _model(ftn, 5, dev, win)
    cache = fit.OutputCache(model, win, use_loss_mask=True)
    params = fit._refit_params(model)
    opt = fit.DeviceAdamW(params, lr=1e-2)
    step = fit.GraphedCachedStep(cache, model, opt, BATCH)
    step.step(torch.tensor([1, 2, 3, 4], device=dev))
    state = [t.clone() for t in _six(ftn, model) + opt.exp_avg + opt.exp_avg_sq] + [opt._state.clone()]
    assert int(opt._state[0]) == 1
    step.rows.copy_(torch.tensor([1, 2, cache.n_items, 4], device=dev))
    loss = step.replay().clone()
    assert int(step.status) == 4 and bool(torch.isfinite(loss).all())
    now = _six(ftn, model) + opt.exp_avg + opt.exp_avg_sq
    assert _same(state[:-1], now) and int(opt._state[0]) == 1 and int(opt._state[1]) == 2
    log = opt.history()
    assert log[:, 3].tolist() == [0.0, 8.0]
    step.step(torch.tensor([1, 2, 3, 4], device=dev))           # the word is rewritten: the next step counts again
    assert int(step.status) == 0 and int(opt._state[0]) == 2


def test_refit_output_cached_raises_index_error_for_a_logged_status(ftn, dev, monkeypatch):
    """The loop's own orders are always inside the cache, so the row list is bent on its way into the step."""
    fit = ftn.fit
    win = _windows(ftn, 5, dev, T=39)
    model = _model(ftn, 5, dev, win)
    real = fit.GraphedCachedStep.step

    def bent(self, rows):
        rows = rows.clone()
        rows[1] = -1
        return real(self, rows)

    monkeypatch.setattr(fit.GraphedCachedStep, "step", bent)
    before = _six(ftn, model)
    with pytest.raises(IndexError, match="outside the cache"):
        fit.refit_output_cached(model, win, epochs=1)
    assert _same(before, _six(ftn, model))
