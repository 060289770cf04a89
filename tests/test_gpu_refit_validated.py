"""``fit.refit_output_validated`` on the device: the loop whose epochs end in ``ftn_refit_epoch_end`` against the
host-driven loop ``refit_epoch_oracle.HostDriven`` built from the same launches, on the tiny model and the windows of
``test_gpu_refit_cache.py`` (train table T = 40: 13 items, a short last batch; held-out table T = 33: 6 items, one
full and one short batch).  Every comparison is ``torch.equal`` or a comparison of fp64 bit patterns."""
import copy

import pytest
import torch

from refit_epoch_oracle import HostDriven, bits
from test_gpu_refit_cache import BATCH, H, L, SETTINGS, _model, _same, _six, _windows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _held_out(ftn, N, dev, T=33):
    """Held-out windows in the layout of ``_windows`` from another seed."""
    g = torch.Generator().manual_seed(121 + N)
    t = torch.arange(T, dtype=torch.float32).view(T, 1)
    table = torch.poisson(2.0 + torch.sin(2 * torch.pi * t / 6.0) + torch.rand(T, N, generator=g), generator=g)
    valid = (torch.rand(T, N, generator=g) >= 0.2).float()
    extra = dict(layout="series", series_static=torch.tensor([[0.5, -1.0]]),
                 series_ids=torch.zeros(1, dtype=torch.int64)) if N == 1 else dict(layout="wide")
    return ftn.windows.DeviceWindows(table.to(dev), L, H, valid_mask=valid.to(dev), batch_size=BATCH, **extra)


def _pair(ftn, N, dev, **kw):
    win, val = _windows(ftn, N, dev, **kw), _held_out(ftn, N, dev)
    assert win.n_items == 13 and len(win) == 4 and val.n_items == 6 and len(val) == 2
    model = _model(ftn, N, dev, win)
    return model, copy.deepcopy(model), win, val


def _compare(ftn, got, want, model, twin):
    assert torch.equal(got.losses, want.losses)
    assert bits(got.val_nll.tolist()) == bits(want.val_nll) and bits(got.val_smape.tolist()) == bits(want.val_smape)
    assert bits(got.lr.tolist()) == bits(want.lr)
    assert got.best_epoch == want.best_epoch and got.stopped_epoch == want.stopped_epoch
    assert bits([got.best_nll, got.best_smape]) == bits([want.best_nll, want.best_smape])
    assert _same(_six(ftn, model), _six(ftn, twin))
    a, b = got.optimizer, want.optimizer
    assert _same(a.exp_avg + a.exp_avg_sq, b.exp_avg + b.exp_avg_sq) and int(a._state[0]) == int(b._state[0])


PLATEAU = (0.5, 0, 1e-4, 1e-4)


@pytest.mark.parametrize("N,kw", [
    (5, dict(epochs=3, lr=2e-2, patience=None, plateau=PLATEAU)),
    (1, dict(epochs=3, lr=[1e-2, 5e-3, 2e-3], patience=2, plateau=None)),
])
def test_device_loop_is_the_host_driven_loop(N, kw, ftn, dev):
    """And for the direct model the validation sums of the first two epochs are those of full ``model(...)``
    forwards on the held-out batches."""
    fit = ftn.fit
    model, twin, win, val = _pair(ftn, N, dev, **(dict(shuffle=True, seed=7) if N == 5 else {}))
    got = fit.refit_output_validated(model, win, val, **kw, **SETTINGS)
    assert fit._last_epoch_backend == "hip" and fit._last_optim_backend == "hip" and win.epoch == (3 if N == 5 else 0)
    win.epoch = 0
    want = HostDriven(ftn, twin, win, val, **kw, inference_epochs=2, **SETTINGS)
    print("val_nll", want.val_nll, "lr", want.lr, "best", want.best_epoch)
    _compare(ftn, got, want, model, twin)
    assert got.val_nll.shape == (3,) and got.epochs_enqueued == 3
    assert len(want.acc_cache) == 2
    for a, b in zip(want.acc_cache, want.acc_model):
        assert torch.equal(a, b)


STOPPING = dict(epochs=6, lr=0.3, patience=0, plateau=(0.5, 1, 1e-4, 1e-3))


def test_the_loop_stops_and_restores_an_earlier_epoch(ftn, dev):
    """The scenario of the host test, on the device's own oracle: the oracle stops before the last epoch and restores
    an earlier one, ``sync_every=None`` enqueues all six epochs and ``sync_every=1`` only those that ran."""
    fit = ftn.fit
    model, twin, win, val = _pair(ftn, 5, dev)
    twin2 = copy.deepcopy(model)
    want = HostDriven(ftn, twin, win, val, **STOPPING, **SETTINGS)
    print("val_nll", want.val_nll, "lr", want.lr, "best", want.best_epoch, "stopped", want.stopped_epoch)
    assert want.stopped_epoch is not None and want.stopped_epoch < STOPPING["epochs"]
    assert 0 < want.best_epoch < want.stopped_epoch
    got = fit.refit_output_validated(model, win, val, **STOPPING, **SETTINGS)
    assert got.epochs_enqueued == 6 and got.losses.shape == (want.stopped_epoch * len(win),)
    _compare(ftn, got, want, model, twin)
    again = fit.refit_output_validated(twin2, win, val, **STOPPING, **SETTINGS, sync_every=1)
    assert again.epochs_enqueued == want.stopped_epoch < got.epochs_enqueued
    _compare(ftn, again, want, twin2, twin)


def test_replays_after_the_stop_keep_every_bit(ftn, dev):
    fit = ftn.fit
    model, _, win, val = _pair(ftn, 5, dev)
    cache = fit.OutputCache(model, win, use_loss_mask=True)
    vcache = fit.OutputCache(model, val, use_loss_mask=True)
    params = fit._refit_params(model)
    opt = fit.DeviceAdamW(params, lr=1e-2)
    end = fit.EpochEnd(params, 5, 8, 1e-2, patience=0)
    step = fit.GraphedCachedStep(cache, model, opt, BATCH, extra_skip=[end.stop])
    evaluator = fit.GraphedCachedEval(vcache, model, end.accumulators, BATCH)
    rows, vrows = torch.tensor([3, 0, 12, 7], device=dev), torch.arange(6, device=dev)

    def validate():
        evaluator.run(vrows[:4])
        evaluator.run(vrows[4:])
        end.end_epoch(opt)

    step.step(rows)
    validate()                                                      # epoch 1: better than +inf
    validate()                                                      # epoch 2: the same NLL is not better -> stop
    assert int(end.stop) == 16 and int(end.improved) == 0 and int(opt._state[0]) == 1
    assert _same(end.best, _six(ftn, model))
    before = [t.clone() for t in _six(ftn, model) + opt.exp_avg + opt.exp_avg_sq + [opt._state[:1], end.state[:56]]]
    for _ in range(2):
        step.step(rows)
        step.step(torch.tensor([1, 2, 5, 9], device=dev))
        validate()
    now = _six(ftn, model) + opt.exp_avg + opt.exp_avg_sq + [opt._state[:1], end.state[:56]]
    assert _same(before, now) and int(opt._state[1]) == 5
    assert opt.history()[:, 3].tolist() == [0.0, 8.0, 8.0, 8.0, 8.0]
    hist = end.history()
    assert hist["stopped_epoch"] == 2 and hist["best_epoch"] == 1 and hist["epoch"] == 2
    assert hist["rows"][:, 3].tolist() == [0.0, 0.0, 16.0, 16.0] and hist["rows"][:, 4].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert bits(hist["rows"][0, :2].tolist()) == bits(hist["rows"][1, :2].tolist())
    assert not bool(end.accumulators._acc.any())
    assert int(evaluator.bad_seen) == 0 and int(evaluator.rows_seen) == 0


def test_a_row_outside_the_validation_cache_is_clamped_and_reported(ftn, dev, monkeypatch):
    fit = ftn.fit
    model, _, win, val = _pair(ftn, 5, dev)
    vcache = fit.OutputCache(model, val, use_loss_mask=True)
    params = fit._refit_params(model)
    end = fit.EpochEnd(params, 5, 2, 1e-2)
    evaluator = fit.GraphedCachedEval(vcache, model, end.accumulators, BATCH)
    evaluator.run(torch.tensor([0, 1, 2, 5], device=dev))
    inside = end.accumulators._acc.clone()
    assert int(evaluator.status) == 0 and int(evaluator.rows_seen) == 0
    end.accumulators.reset()
    evaluator.run(torch.tensor([0, 1, 2, vcache.n_items + 3], device=dev))      # clamped to item 5
    assert int(evaluator.status) == 4 and int(evaluator.rows_seen) == 4
    assert torch.equal(end.accumulators._acc, inside)
    evaluator.run(torch.tensor([4, -1], device=dev))                # the eager short batch reports as well
    evaluator.run(torch.tensor([0, 1, 2, 3], device=dev))
    assert int(evaluator.status) == 0 and int(evaluator.rows_seen) == 4           # the report is sticky
    real = fit.GraphedCachedEval.run

    def bent(self, rows):
        rows = rows.clone()
        rows[0] = 99
        return real(self, rows)

    monkeypatch.setattr(fit.GraphedCachedEval, "run", bent)
    with pytest.raises(IndexError, match="outside the validation cache"):
        fit.refit_output_validated(model, win, val, 1, **SETTINGS)
