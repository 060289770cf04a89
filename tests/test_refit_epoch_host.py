"""The validated refit on the host (no GPU): the rule of ``fit.EpochEnd(backend="torch")`` against the plain-Python
``refit_epoch_oracle.EpochOracle`` and a real ``ReduceLROnPlateau``, ``fit.refit_output_validated`` on the CPU tiny
model against the host-driven loop ``refit_epoch_oracle.HostDriven``, that the feature is additive, the pinned copy
forms of ``ftn_refit_epoch_form``, and the argument checks (nothing here reaches a launch)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from refit_epoch_oracle import SEQUENCES, EpochOracle, HostDriven, bits, validation_means
from test_output_fit_host import H, L, _tiny
from test_refit_cache_host import _six_state, _windows

SETTINGS = dict(weight_decay=0.01, grad_clip=0.05, use_loss_mask=True)


def _load(ftn, acc, nll_sum, nll_cnt, smape_sum, smape_cnt, den_extra=0.0):
    sums, counts = ftn.score._part_views(acc._acc)
    sums[:, 0] = torch.tensor(nll_sum, dtype=torch.float64)
    sums[:, 1] = torch.tensor(smape_sum, dtype=torch.float64)
    counts[:, 0] = torch.tensor(nll_cnt, dtype=torch.int32)
    counts[:, 1] = torch.tensor(smape_cnt, dtype=torch.int32)
    acc._den_extra.fill_(den_extra)
    acc._count_seen.fill_(int(sum(nll_cnt)))


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_rule_on_the_torch_backend(name, ftn):
    values, lr, patience, plateau = SEQUENCES[name]
    fit = ftn.fit
    S = 3
    params = [torch.zeros(5), torch.zeros(2, 3)]
    opt = fit.DeviceAdamW(params, lr=lr, backend="torch")
    end = fit.EpochEnd(params, S, len(values), lr, patience, plateau, backend="torch")
    oracle = EpochOracle(lr, patience, plateau)
    knob = torch.nn.Parameter(torch.zeros(1))
    sched = None
    if plateau is not None:
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(
            torch.optim.SGD([knob], lr=lr), mode="min", factor=plateau[0], patience=plateau[1], threshold=plateau[2],
            threshold_mode="rel", cooldown=0, min_lr=plateau[3], eps=1e-8)
    stopped = False
    for e, v in enumerate(values):
        with torch.no_grad():
            for p in params:
                p.fill_(float(e + 1))
        _load(ftn, end.accumulators, [0.0, 0.0, v], [0, 0, 1], [0.25 * (e + 1), 0.0, 0.0], [2, 0, 0])
        end.end_epoch(opt)
        assert fit._last_epoch_backend == "torch"
        row = oracle.end(v, 0.125 * (e + 1), lr_word=float(np.float32(lr)))
        assert bits(end.log[e].tolist()) == bits(row), (name, e)
        assert end._i32[8:15].tolist() == oracle.words(), (name, e)
        assert bits(end._f64[:4].tolist()) == bits(oracle.doubles()), (name, e)
        assert float(opt._lr) == float(np.float32(oracle.lr))
        if sched is not None and not stopped:
            sched.step(v)
            assert float(opt._lr) == float(np.float32(sched.optimizer.param_groups[0]["lr"])), (name, e)
        stopped = bool(oracle.stop)
        assert int(end.stop) == oracle.stop and int(end.improved) == oracle.improved
        assert not end.accumulators._acc.any() and float(end.accumulators._den_extra) == 0.0
        assert int(end.accumulators._count_seen) == 0
        want = float(oracle.best_epoch)
        assert all(bool((b == want).all()) for b in end.best) or oracle.best_epoch == 0
    hist = end.history()
    assert hist["best_epoch"] == oracle.best_epoch and hist["stopped_epoch"] == oracle.stopped_epoch
    assert hist["rows"].shape == (len(values), 5)
    if oracle.stop:
        assert oracle.calls > oracle.epoch and hist["rows"][oracle.epoch:, 3].tolist() == [16.0] * (oracle.calls - oracle.epoch)
    before = [p.clone() for p in params]
    end.restore()
    for p, b, old in zip(params, end.best, before):
        assert torch.equal(p, b if oracle.best_epoch > 0 else old)


def test_the_sequences_cover_what_they_claim():
    """Stops with calls after them, a run without a stop, a rate held by eps, and both sides of the threshold."""
    ran = {}
    for name, (values, lr, patience, plateau) in SEQUENCES.items():
        o = EpochOracle(lr, patience, plateau)
        for v in values:
            o.end(v, 0.0)
        ran[name] = o
    assert ran["equal to the best"].stopped_epoch == 3 and ran["equal to the best"].best_epoch == 1
    assert ran["nan and inf epochs"].stopped_epoch == 8 and ran["nan and inf epochs"].best_epoch == 4
    assert ran["first epoch nan"].best_epoch == 3 and ran["first epoch nan"].rows[0][4] == 0.0
    assert ran["patience 0"].stopped_epoch == 3 and ran["patience None"].stopped_epoch is None
    assert ran["patience None"].best_epoch == 6
    assert ran["min_lr reached"].lr == 5e-5 and ran["min_lr within eps"].lr == 1e-3
    assert ran["at the threshold"].rows[1][2] == ran["one spacing above the threshold"].rows[1][2] == 5e-3
    assert ran["one spacing below the threshold"].rows[1][2] == 1e-2


def test_validation_means_are_the_scorers(ftn):
    """The torch backend's sums on real accumulator contents: ``result()`` of a ``ForecastScorer`` fed the same
    batches, a batch without one valid element included."""
    fit, score = ftn.fit, ftn.score
    g = torch.Generator().manual_seed(3)
    params = [torch.zeros(3)]
    end = fit.EpochEnd(params, 7, 2, 1e-3, backend="torch")
    opt = fit.DeviceAdamW(params, lr=1e-3, backend="torch")
    plain = score.ForecastScorer(7, "cpu")
    for k in range(3):
        y = torch.poisson(torch.full((3, 4, 7), 2.0), generator=g)
        rate, disp = torch.rand(3, 4, 7, generator=g) + 0.5, torch.rand(3, 4, 7, generator=g) + 0.1
        mask = torch.rand(3, 4, 7, generator=g) > (1.0 if k == 1 else 0.3)       # batch 1: nothing valid
        end.accumulators.update(y, rate, disp, mask)
        plain.update(y, rate, disp, mask)
    assert torch.equal(end.accumulators._acc, plain._acc) and float(plain._den_extra) == 84.0
    got, want = end.accumulators.result(), plain.result()
    assert got["nll"] == want["nll"] and got["smape"] == want["smape"]
    end.end_epoch(opt)
    assert bits(end.log[0, :2].tolist()) == bits([want["nll"], want["smape"]])
    sums, counts = score._part_views(plain._acc)
    assert bits(validation_means(sums[:, 0].tolist(), counts[:, 0].tolist(), sums[:, 1].tolist(),
                                 counts[:, 1].tolist(), 84.0)) == bits([want["nll"], want["smape"]])
    end.accumulators.update(y, rate, disp, mask)                        # the cleared buffers start a fresh scorer
    fresh = score.ForecastScorer(7, "cpu")
    fresh.update(y, rate, disp, mask)
    assert torch.equal(end.accumulators._acc, fresh._acc) and torch.equal(end.accumulators._den_extra, fresh._den_extra)


def _val_windows(ftn, N, layout, T=33):
    """Held-out windows of the same series count from another seed: 6 items, one full and one short batch."""
    g = torch.Generator().manual_seed(101 + N)
    t = torch.arange(T, dtype=torch.float32).view(T, 1)
    table = torch.poisson(2.0 + torch.sin(2 * torch.pi * t / 6.0) + torch.rand(T, N, generator=g), generator=g)
    valid = (torch.rand(T, N, generator=g) >= 0.2).float()
    return ftn.windows.DeviceWindows(table, L, H, valid_mask=valid, batch_size=4, layout=layout, device="cpu")


def _compare(ftn, got, want, model, twin):
    assert torch.equal(got.losses, want.losses)
    assert bits(got.val_nll.tolist()) == bits(want.val_nll) and bits(got.val_smape.tolist()) == bits(want.val_smape)
    assert bits(got.lr.tolist()) == bits(want.lr)
    assert got.best_epoch == want.best_epoch and got.stopped_epoch == want.stopped_epoch
    assert bits([got.best_nll, got.best_smape]) == bits([want.best_nll, want.best_smape])
    a, b = _six_state(model), _six_state(twin)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("N,layout,kw", [
    (5, "wide", dict(epochs=4, lr=2e-2, patience=None, plateau=dict(factor=0.5, patience=0))),
    (1, "series", dict(epochs=3, lr=[1e-2, 5e-3, 2e-3], patience=2, plateau=None)),
])
def test_validated_refit_is_the_host_driven_loop_on_the_cpu(N, layout, kw, ftn):
    fit = ftn.fit
    model, _ = _tiny(ftn, N)
    win, val = _windows(ftn, N, layout, T=40), _val_windows(ftn, N, layout)
    assert win.n_items % 4 != 0 and val.n_items == 6 and len(val) == 2
    model.output_inputs(win.batch(0)[0])
    twin = copy.deepcopy(model)
    flags = [p.requires_grad for p in model.parameters()]
    got = fit.refit_output_validated(model, win, val, **kw, **SETTINGS)
    assert fit._last_epoch_backend == "torch" and fit._last_optim_backend == "torch"
    assert [p.requires_grad for p in model.parameters()] == flags and not model.training
    rule = fit._epoch_rule("test", kw["patience"], kw["plateau"])[1]
    want = HostDriven(ftn, twin, win, val, kw["epochs"], kw["lr"], patience=kw["patience"], plateau=rule,
                      inference_epochs=2 if layout == "wide" else 0, **SETTINGS)
    _compare(ftn, got, want, model, twin)
    assert got.val_nll.shape == (kw["epochs"],) and got.epochs_enqueued == kw["epochs"]
    for a, b in zip(want.acc_cache, want.acc_model):                 # the cache scores what the model forecasts
        assert torch.equal(a, b)


STOPPING = dict(epochs=6, lr=0.3, patience=1, plateau=dict(factor=0.5, patience=1, threshold=1e-4, min_lr=1e-3),
                weight_decay=0.01, grad_clip=None, use_loss_mask=True)


def test_the_loop_stops_and_restores_an_earlier_epoch(ftn):
    """A rate far too high: the held-out NLL turns up after a few epochs.  The oracle stops before the last epoch and
    restores an earlier one; the device-side rule must do both to agree with it."""
    fit = ftn.fit
    model, _ = _tiny(ftn, 5)
    win, val = _windows(ftn, 5, "wide", T=40), _val_windows(ftn, 5, "wide")
    model.output_inputs(win.batch(0)[0])
    twin, twin2 = copy.deepcopy(model), copy.deepcopy(model)
    kw = {**STOPPING, "plateau": fit._epoch_rule("test", 1, STOPPING["plateau"])[1]}
    want = HostDriven(ftn, twin, win, val, **kw)
    print("val_nll", want.val_nll, "lr", want.lr, "best", want.best_epoch, "stopped", want.stopped_epoch)
    assert want.stopped_epoch is not None and want.stopped_epoch < STOPPING["epochs"]
    assert 0 < want.best_epoch < want.stopped_epoch
    got = fit.refit_output_validated(model, win, val, **STOPPING)
    assert got.epochs_enqueued == STOPPING["epochs"] and got.losses.shape == (want.stopped_epoch * len(win),)
    _compare(ftn, got, want, model, twin)
    # reading the stop word every epoch ends the loop early with the same result
    again = fit.refit_output_validated(twin2, win, val, **STOPPING, sync_every=1)
    assert again.epochs_enqueued == want.stopped_epoch
    _compare(ftn, again, want, twin2, twin)


def test_the_feature_is_additive(ftn):
    """No patience, no schedule, no restore: the six tensors and the losses of ``refit_output_cached``."""
    fit = ftn.fit
    model, _ = _tiny(ftn, 5)
    win, val = _windows(ftn, 5, "wide", T=40), _val_windows(ftn, 5, "wide")
    model.output_inputs(win.batch(0)[0])
    twin = copy.deepcopy(model)
    got = fit.refit_output_validated(model, win, val, 3, lr=[1e-2, 5e-3, 2e-3], patience=None, plateau=None,
                                     restore_best=False, **SETTINGS)
    want = fit.refit_output_cached(twin, win, epochs=3, lr=[1e-2, 5e-3, 2e-3], graphed=False, **SETTINGS)
    assert torch.equal(got.losses, want) and got.stopped_epoch is None
    a, b = _six_state(model), _six_state(twin)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert got.lr.tolist() == [float(np.float32(v)) for v in (1e-2, 5e-3, 2e-3)]


K = 4096                                                            # elements of a chunk: 1024 units of 4
FORMS = [
    ([1], None, ("vec", 0, 1)),
    ([3], None, ("vec", 0, 1)),
    ([4 * 7 + 1], None, ("vec", 0, 1)),
    ([K], None, ("vec", 0, 1)),
    ([K + 1], None, ("vec", 0, 2)),
    ([K - 3, 5], None, ("vec", 0, 2)),                              # the second tensor's units straddle the boundary
    ([5, 80, 16, 5, 64, 4, 96, 4], None, ("vec", 0, 1)),
    ([5, 80, 16, 5, 64, 4, 96, 4], [0, 4, 0, 0, 8, 0, 0, 12], ("mixed", 0b10010010, 1)),
    ([17], [4], ("mixed", 1, 1)),
    ([K * 1024], None, ("vec", 0, 1024)),
    ([K * 1024 + 1], None, ("vec", 0, 820)),                        # beyond 1024 chunks: 1280 units a chunk
    ([K * 2048], None, ("vec", 0, 1024)),
]


@pytest.mark.parametrize("counts,misalign,want", FORMS)
def test_epoch_copy_forms_are_pinned(counts, misalign, want, ftn):
    assert ftn.runtime.refit_epoch_form_of(counts, misalign) == want


def test_epoch_form_rejects_bad_lists(ftn):
    rt = ftn.runtime
    for counts, mis in (([], None), ([1] * 9, None), ([0], None), ([4, -1], None), ([4], [2]), ([4], [16]),
                        ([2 ** 31], None)):
        with pytest.raises(ValueError, match="ftn_refit_epoch_form"):
            rt.refit_epoch_form_of(counts, mis)
    with pytest.raises(ValueError, match="2 misalign values for 1 tensors"):
        rt.refit_epoch_form_of([4], [0, 0])


A, M = 0x10000, 0x10004          # stand-ins for device addresses: 16-byte aligned / 4 bytes past a boundary


def _end_args(ftn, **over):
    a = ftn.lib.FtnEpochArgs()
    a.acc, a.n_slots, a.max_epochs, a.err, a.den_extra, a.count_seen = A, 3, 4, A, A, None
    a.state, a.lr, a.log, a.plateau_patience, a.patience_limit = A, A, A, -1, -1
    a.n_tensors = 1
    a.src[0], a.dst[0], a.n[0] = A, A + 0x1000, 16
    for k, v in over.items():
        if k in ("src", "dst", "n"):
            getattr(a, k)[0] = v
        else:
            setattr(a, k, v)
    return a


END_BAD = {"null acc": dict(acc=None), "acc off by 4": dict(acc=M), "no slots": dict(n_slots=0),
           "no log rows": dict(max_epochs=0), "null log": dict(log=None), "null err": dict(err=None),
           "lr off by 2": dict(lr=A + 2), "null state": dict(state=None), "den_extra off by 4": dict(den_extra=M),
           "count_seen off by 4": dict(count_seen=M), "plateau factor 1": dict(plateau_patience=0, factor=1.0),
           "plateau min_lr < 0": dict(plateau_patience=0, factor=0.5, min_lr=-1.0), "9 tensors": dict(n_tensors=9),
           "empty tensor": dict(n=0), "null src": dict(src=None), "dst off by 2": dict(dst=A + 0x1002),
           "overlap": dict(dst=A + 32)}


@pytest.mark.parametrize("name", list(END_BAD))
def test_epoch_end_rejects_bad_arguments_before_any_launch(name, ftn):
    lib = ftn.lib.load()
    assert lib.ftn_timeproj_form(24, 4, 64, 0) > 0                      # leaves an earlier message out of the way
    rc = lib.ftn_refit_epoch_end(C.byref(_end_args(ftn, **END_BAD[name])), None)
    assert rc != 0 and lib.ftn_last_error().decode().startswith("ftn_refit_epoch_end"), lib.ftn_last_error()
    with pytest.raises(ValueError, match="ftn_refit_epoch_end"):
        ftn.lib.check(rc, "ftn_refit_epoch_end")


def test_epoch_restore_rejects_bad_arguments_before_any_launch(ftn):
    lib = ftn.lib.load()
    one = lambda v: (C.c_void_p * 1)(v)
    n = (C.c_longlong * 1)(16)
    for state, src, dst, cnt, k in ((None, one(A), one(A + 0x1000), n, 1), (M, one(A), one(A + 0x1000), n, 1),
                                    (A, one(A), one(A + 0x1000), n, 0), (A, one(None), one(A + 0x1000), n, 1),
                                    (A, one(A), one(A + 16), n, 1), (A, one(A), one(A + 0x1000), (C.c_longlong * 1)(0), 1)):
        assert lib.ftn_timeproj_form(24, 4, 64, 0) > 0
        rc = lib.ftn_refit_epoch_restore(state, k, src, dst, cnt, None)
        assert rc != 0 and lib.ftn_last_error().decode().startswith("ftn_refit_epoch_restore"), lib.ftn_last_error()


def test_exports_abi_and_record_sizes(ftn):
    assert {"ftn_refit_epoch_form", "ftn_refit_epoch_end", "ftn_refit_epoch_restore"} <= set(ftn.lib.EXPORTS)
    assert ftn.lib.load().ftn_abi_version() == 14
    assert C.sizeof(ftn.lib.FtnEpochState) == ftn.fit._STATE_BYTES == ftn.runtime.EPOCH_STATE_BYTES == 64
    assert ftn.lib.FtnEpochState.stop.offset == 4 * ftn.fit._I_STOP
    assert ftn.lib.FtnEpochState.calls.offset == 4 * ftn.fit._I_CALLS


def test_argument_errors_come_before_any_work(ftn):
    fit = ftn.fit
    model, _ = _tiny(ftn, 5)
    win, val = _windows(ftn, 5, "wide"), _val_windows(ftn, 5, "wide")
    run = lambda **kw: fit.refit_output_validated(model, win, kw.pop("val", val), kw.pop("epochs", 2), **kw)
    with pytest.raises(ValueError, match="exclude each other"):
        run(lr=[1e-3, 1e-3], plateau=dict(factor=0.5))
    with pytest.raises(ValueError, match="1 learning rates for 2 epochs"):
        run(lr=[1e-3])
    with pytest.raises(ValueError, match="epochs=0"):
        run(epochs=0)
    with pytest.raises(ValueError, match="patience=-1"):
        run(patience=-1)
    with pytest.raises(ValueError, match="plateau factor=1.0"):
        run(plateau=dict(factor=1.0))
    with pytest.raises(ValueError, match="unknown keys"):
        run(plateau=dict(cooldown=2))
    with pytest.raises(ValueError, match="sync_every=0"):
        run(sync_every=0)
    with pytest.raises(ValueError, match="must be a default loader"):
        run(val=_windows(ftn, 5, "wide", shuffle=True))
    with pytest.raises(ValueError, match="are the training windows"):
        run(val=win)
    with pytest.raises(ValueError, match="filled from other windows"):
        run(val_cache=fit.OutputCache(model, win))
    params = [torch.zeros(3)]
    for kw in (dict(n_slots=0, max_epochs=1), dict(n_slots=1, max_epochs=0), dict(n_slots=1, max_epochs=1, lr=-1.0),
               dict(n_slots=1, max_epochs=1, backend="cuda")):
        with pytest.raises(ValueError, match="EpochEnd"):
            fit.EpochEnd(params, **{"lr": 1e-3, **kw})
    with pytest.raises(ValueError, match="parameter tensors"):
        fit.EpochEnd([], 1, 1, 1e-3)
    with pytest.raises(ValueError, match="its lr word"):
        fit.EpochEnd(params, 1, 1, 1e-3, backend="torch").end_epoch(object())
    with pytest.raises(ValueError, match="needs fit.ValidationAccumulators"):
        fit.GraphedCachedEval(fit.OutputCache(model, val), model, ftn.score.ForecastScorer(5, "cpu"), 4)
