"""The rule of ``fit.EpochEnd`` / ``ftn_refit_epoch_end`` restated in plain Python, for the host and the GPU tests:
the reference's validation bookkeeping (train.py:1536-1572) with torch's ``ReduceLROnPlateau(mode="min",
threshold_mode="rel", cooldown=0, eps=1e-8)``.  Python floats are fp64, so every value here is the one the kernel
must produce to the bit.  Also the synthetic validation sequences both tests run."""
import math
import struct

INF, NAN = float("inf"), float("nan")


def validation_means(nll_sum, nll_cnt, smape_sum, smape_cnt, den_extra=0.0):
    """``(val_nll, val_smape)`` from per-slot sums as ``ForecastScorer.result()`` takes them: slots ascending."""
    num = sm = 0.0
    for v in nll_sum:
        num += float(v)
    for v in smape_sum:
        sm += float(v)
    den = float(sum(int(c) for c in nll_cnt)) + float(den_extra)
    n_sm = sum(int(c) for c in smape_cnt)
    return (num / den if den > 0 else 0.0), (sm / n_sm if n_sm > 0 else 0.0)


class EpochOracle:
    def __init__(self, lr, patience=None, plateau=None):
        self.best_nll = self.best_smape = self.plateau_best = INF
        self.lr = float(lr)
        self.epoch = self.best_epoch = self.patience = self.num_bad = self.stop = self.improved = self.calls = 0
        self.limit, self.plateau = patience, plateau            # plateau: (factor, patience, threshold, min_lr)
        self.rows = []

    def end(self, val_nll, val_smape, err=0, lr_word=None):
        """One call; returns the log row.  ``lr_word``: without a plateau schedule, the optimizer's rate."""
        self.calls += 1
        if self.plateau is None and lr_word is not None:
            lr_now = float(lr_word)
        else:
            lr_now = self.lr
        if self.stop:
            row = (NAN, NAN, lr_now, 16.0, 0.0)
            self.rows.append(row)
            return row
        self.epoch += 1
        self.lr = lr_now
        if self.plateau is not None:
            factor, p_pat, threshold, min_lr = self.plateau
            if val_nll < self.plateau_best * (1.0 - threshold):
                self.plateau_best, self.num_bad = val_nll, 0
            else:
                self.num_bad += 1
            if self.num_bad > p_pat:
                new = max(self.lr * factor, min_lr)
                if self.lr - new > 1e-8:
                    self.lr = new
                self.num_bad = 0
        if val_nll < self.best_nll:
            self.best_nll, self.best_smape, self.best_epoch = val_nll, val_smape, self.epoch
            self.patience, self.improved = 0, 1
        else:
            self.improved = 0
            self.patience += 1
            if self.limit is not None and self.patience > self.limit:
                self.stop = 16
        row = (val_nll, val_smape, self.lr, 32.0 if err else 0.0, float(self.improved))
        self.rows.append(row)
        return row

    @property
    def stopped_epoch(self):
        return self.epoch if self.stop else None

    def words(self):
        """The int32 words of the state record from ``epoch`` on."""
        return [self.epoch, self.best_epoch, self.patience, self.num_bad, self.stop, self.improved, self.calls]

    def doubles(self):
        return [self.best_nll, self.best_smape, self.plateau_best, self.lr]


class HostDriven:
    """``fit.refit_output_validated`` the way a host drives it: ``OutputCache``s, the eager cached step with one
    ``DeviceAdamW``, a fresh ``ForecastScorer`` per epoch read on the host, ``EpochOracle``'s Python comparisons,
    ``set_lr`` and ``load``-style copies of the six tensors.  ``inference_epochs``: for that many epochs the held-out
    batches are also scored from full ``model(...)`` forwards; ``acc_cache`` / ``acc_model`` keep both scorers' bytes."""

    def __init__(self, ftn, model, win, val, epochs, lr=1e-3, weight_decay=0.0, grad_clip=None, use_loss_mask=False,
                 patience=None, plateau=None, restore_best=True, inference_epochs=0):
        import torch

        fit, score = ftn.fit, ftn.score
        rates = [float(lr)] * epochs if isinstance(lr, (int, float)) else [float(v) for v in lr]
        cache = fit.OutputCache(model, win, use_loss_mask=use_loss_mask)
        vcache = fit.OutputCache(model, val, use_loss_mask=use_loss_mask)
        params = fit._refit_params(model)
        dev = params[0].device
        flags = [p.requires_grad for p in model.parameters()]
        for p in model.parameters():
            p.requires_grad_(False)
        for p in params:
            p.requires_grad_(True)
        was_training = model.training
        model.eval()
        opt = self.optimizer = fit.DeviceAdamW(params, lr=rates[0], weight_decay=weight_decay, max_norm=grad_clip)
        rule = self.rule = EpochOracle(rates[0], patience, plateau)
        proj, steps, B = model.forecast_time_proj, cache.steps, win.batch_size
        losses, best = [], None
        self.acc_cache, self.acc_model = [], []
        for e in range(epochs):
            if plateau is None:
                opt.set_lr(rates[e])
            order = win.order(win.epoch).to(dev)
            if not win._default:
                win.epoch += 1
            for i in range(len(win)):
                rows = order[i * B:(i + 1) * B]
                tail, y, mask, late = cache.select(rows)
                opt.zero_grad(set_to_none=True)
                with torch.enable_grad():
                    loss, bad = fit.output_nll(cache.seq, proj.weight[-steps:], proj.bias[-steps:], *params[:4], tail,
                                               cache.hist, y, mask, late, cache.floor, cache.min_sigma, rows=rows)
                loss.backward()
                opt.step(loss=loss.detach(), skip=[bad])
                opt.zero_grad(set_to_none=True)
                losses.append(loss.detach().reshape(1))
            scorer = score.ForecastScorer(vcache.y.shape[2], dev)
            for k0 in range(0, val.n_items, val.batch_size):
                rows = torch.arange(k0, min(k0 + val.batch_size, val.n_items), dtype=torch.int64, device=dev)
                y, mask, rate, disp, bad, status = fit._cached_forecast(vcache, model, rows)
                assert int(bad) == 0 and int(status) == 0
                scorer.update(y, rate, disp, mask)
            if e < inference_epochs:
                full = score.ForecastScorer(vcache.y.shape[2], dev)
                with torch.no_grad():
                    for i in range(len(val)):
                        xb, yb, mk, x_mark, _, static, ids = score._unpack_batch(val.batch(i))
                        rate, disp = model(xb, x_mark, static, ids)
                        full.update(yb[:, :steps, :], rate, disp, (mk[:, :steps, :] > 0) if use_loss_mask else None)
                self.acc_cache.append(scorer._acc.clone())
                self.acc_model.append(full._acc.clone())
            r = scorer.result()
            rule.end(r["nll"], r["smape"], lr_word=float(opt._lr))
            if plateau is not None:
                opt.set_lr(rule.lr)
            if rule.improved:
                best = [p.detach().clone() for p in params]
            if rule.stop:
                break
        if restore_best and best is not None:
            with torch.no_grad():
                for p, b in zip(params, best):
                    p.copy_(b)
        for p, flag in zip(model.parameters(), flags):
            p.requires_grad_(flag)
        model.train(was_training)
        self.losses = torch.cat(losses).cpu()
        self.val_nll = [r[0] for r in rule.rows]
        self.val_smape = [r[1] for r in rule.rows]
        self.lr = [r[2] for r in rule.rows]
        self.best_epoch, self.stopped_epoch = rule.best_epoch, rule.stopped_epoch
        self.best_nll, self.best_smape = rule.best_nll, rule.best_smape


def bits(values):
    """fp64 values as their bit patterns (a NaN compares equal to itself here)."""
    return [struct.unpack("<q", struct.pack("<d", float(v)))[0] for v in values]


_EDGE = 2.0 * (1.0 - 1e-4)                                      # plateau_best * (1 - threshold) after an epoch at 2.0
_TIGHT = (0.5, 0, 1e-4, 0.0)                                    # every epoch that is not better cuts the rate

# name -> (val_nll sequence, lr, patience, plateau)
SEQUENCES = {
    "strictly falling": ([5.0, 4.0, 3.0, 2.5, 1.0], 1e-2, 1, (0.1, 1, 1e-4, 0.0)),
    "equal to the best": ([3.0, 3.0, 3.0, 2.0, 2.0, 2.0, 2.0], 1e-2, 1, (0.5, 0, 1e-4, 0.0)),
    "at the threshold": ([2.0, _EDGE, 1.5, 1.5], 1e-2, None, _TIGHT),
    "one spacing below the threshold": ([2.0, math.nextafter(_EDGE, -INF), 1.5, 1.5], 1e-2, None, _TIGHT),
    "one spacing above the threshold": ([2.0, math.nextafter(_EDGE, INF), 1.5, 1.5], 1e-2, None, _TIGHT),
    "nan and inf epochs": ([3.0, NAN, INF, 2.0, NAN, NAN, NAN, NAN, 1.0], 1e-2, 3, (0.5, 1, 1e-4, 0.0)),
    "first epoch nan": ([NAN, 3.0, 2.0, NAN, 4.0], 1e-2, 5, (0.5, 0, 1e-4, 0.0)),
    "first epoch inf": ([INF, INF, 2.0, 2.0], 1e-2, 1, (0.5, 0, 1e-4, 0.0)),
    "min_lr reached": ([1.0, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0], 1e-3, None, (0.1, 0, 1e-4, 5e-5)),
    "min_lr within eps": ([1.0, 2.0, 2.0, 2.0], 1e-3, None, (0.5, 0, 1e-4, 1e-3 - 5e-9)),
    "patience 0": ([2.0, 1.0, 1.0, 0.5, 0.25], 1e-2, 0, (0.5, 1, 1e-4, 0.0)),
    "patience None": ([1.0, 2.0, 3.0, 4.0, 5.0, 0.5], 1e-2, None, None),
    "no plateau, patience 1": ([1.0, 2.0, 0.5, 3.0, 4.0, 5.0, 0.1], 1e-2, 1, None),
    "negative values": ([-1.0, -1.0, -2.0, -1.9999, -3.0], 1e-2, 1, (0.5, 0, 1e-4, 0.0)),
}
