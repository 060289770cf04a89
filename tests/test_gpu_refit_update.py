"""``ftn_refit_update`` behind ``runtime.refit_update`` on the MI355X.  The shape table of tests/refit_oracle.py - tensors
of 1 to 4097 elements in sets of 1, 2, 6 and 8, totals across unit tails, tensor boundaries, workgroup boundaries and the
form threshold - against the fp64 restatement after 1 and after 5 calls, within 4 times what torch's fp32
``clip_grad_norm_`` + ``AdamW(foreach=False)`` shows against the same restatement over the same table.  Then the bits:
an idle clip against no clip, run to run, form against form, a NaN-poisoned workspace between guards and the bytes
around every output, a view one float off the 16-byte grid, a skipped call.

Every accuracy case prints ``REFIT_ERR`` with its figures."""
import numpy as np
import pytest
import torch

import refit_oracle as oracle
import ws_poison

pytestmark = pytest.mark.gpu

ONE, GRID = "k_refit_one", "k_refit_norm+k_refit_apply"
PAD = 32                                                        # floats around an output: keeps the 16-byte grid


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


class Run:
    """The operands of a case on the device, every one a view ``PAD + off`` floats into a NaN buffer of its own."""

    def __init__(self, ftn, dev, i, counts, max_norm, wd, off=None, log_steps=8):
        self.rt, self.dev, self.counts, self.max_norm, self.wd = ftn.runtime, dev, counts, max_norm, wd
        ps, self.gs = oracle.case(i, counts)
        off = off or {}
        self.bufs, self.snaps = [], []

        def inside(values, shift=0, dtype=torch.float32):
            values = torch.as_tensor(values, dtype=dtype).reshape(-1)
            fill = float("nan") if dtype == torch.float32 else -7
            buf = torch.full((values.numel() + 2 * PAD + 4,), fill, dtype=dtype, device=dev)
            view = buf[PAD + shift:PAD + shift + values.numel()]
            view.copy_(values)
            self.bufs.append((buf, PAD + shift, values.numel()))
            return view

        self.p = [inside(p, off.get(("p", k), 0)) for k, p in enumerate(ps)]
        self.m = [inside(np.zeros_like(p), off.get(("m", k), 0)) for k, p in enumerate(ps)]
        self.v = [inside(np.zeros_like(p), off.get(("v", k), 0)) for k, p in enumerate(ps)]
        self.goff = {k: off.get(("g", k), 0) for k in range(len(ps))}
        self.lr = torch.full((1,), oracle.LR, device=dev)
        self.state = inside([0, 0], dtype=torch.int32)
        self.log = inside(np.zeros(log_steps * 4)).view(log_steps, 4)

    def grads(self, s):
        out = []
        for k, g in enumerate(self.gs[s]):
            buf = torch.zeros(g.size + 8, device=self.dev)
            view = buf[4 + self.goff[k]:4 + self.goff[k] + g.size]
            view.copy_(torch.from_numpy(g))
            out.append(view)
        return out

    def misalign(self):
        return [(p.data_ptr() | m.data_ptr() | v.data_ptr() | g.data_ptr()) & 15
                for p, m, v, g in zip(self.p, self.m, self.v, self.grads(0))]

    def form(self):
        return self.rt.refit_update_form_of(self.counts, self.misalign())

    def call(self, s, grads=None, **kw):
        self.rt.refit_update(self.p, self.grads(s) if grads is None else grads, self.m, self.v, self.lr, self.state,
                             oracle.BETAS, oracle.EPS, self.wd, self.max_norm, log=self.log, **kw)

    def snapshot(self):
        self.snaps = [buf.clone() for buf, _, _ in self.bufs]

    def around_is_untouched(self):
        for (buf, start, n), snap in zip(self.bufs, self.snaps):
            a, b = buf.view(torch.int32), snap.view(torch.int32)
            assert torch.equal(a[:start], b[:start]) and torch.equal(a[start + n:], b[start + n:])

    def host(self):
        return tuple([t.cpu().numpy() for t in group] for group in (self.p, self.m, self.v))

    def bits(self):
        return [t.clone().view(torch.int32) for t in self.p + self.m + self.v]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


_forms_seen = set()


@pytest.mark.parametrize("i,counts,max_norm,wd", oracle.cases())
def test_shape_table_against_the_fp64_restatement(i, counts, max_norm, wd, ftn, dev):
    ref = oracle.reference_errors()                             # torch's own error: computed once for the module
    want = oracle.want64(i, counts, max_norm, wd)
    run = Run(ftn, dev, i, counts, max_norm, wd)
    name, mask, chunks = run.form()
    assert (name, mask, chunks) == (oracle.form_name(counts), 0, oracle.chunks(counts))
    _forms_seen.add(name)
    run.snapshot()
    for s in range(oracle.STEPS):
        run.call(s)
        if s + 1 in want:
            err = oracle.errors(run.host(), want[s + 1])
            print(f"REFIT_ERR case {i} {counts} {name} after {s + 1}: |p| |m| |v| {err}, torch's own {ref[s + 1]}")
            assert all(e <= 4.0 * r for e, r in zip(err, ref[s + 1]))
    run.around_is_untouched()
    assert run.state.tolist() == [oracle.STEPS, oracle.STEPS]
    log = run.log.cpu()
    norms = [np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in run.gs[s])) for s in range(oracle.STEPS)]
    np.testing.assert_allclose(log[:oracle.STEPS, 1].numpy(), norms, rtol=1e-6)
    assert log[:oracle.STEPS, 2].tolist() == [oracle.LR] * oracle.STEPS and not log[:oracle.STEPS, 3].any()
    assert not log[oracle.STEPS:].any()                         # rows no call reached


def test_every_form_of_the_table_ran(ftn):
    assert _forms_seen == {ONE, GRID} == {oracle.form_name(c) for c in oracle.TABLE}


@pytest.mark.parametrize("i,counts", [(3, (5,)), (19, (193, 255, 256, 257, 1023, 4097)),
                                      (24, (4097, 4097, 4097, 4097, 4097, 7, 193, 1023))])
def test_an_idle_clip_has_the_bits_of_no_clip_and_runs_repeat(i, counts, ftn, dev):
    runs = []
    for max_norm in (None, 1e9, 1e9):
        run = Run(ftn, dev, i, counts, max_norm, 0.01)
        for s in range(3):
            run.call(s)
        runs.append(run.bits())
    assert _same(runs[0], runs[1]) and _same(runs[1], runs[2])
    again = []
    for _ in range(2):                                          # an active clip: run to run
        run = Run(ftn, dev, i, counts, 0.05, 0.01)
        for s in range(3):
            run.call(s)
        again.append(run.bits() + [run.log.clone().view(torch.int32)])
    assert _same(again[0], again[1]) and not _same(again[0][:len(counts)], runs[0][:len(counts)])


@pytest.mark.parametrize("i,counts", [(5, (64,)), (17, (4097, 4097)), (20, (4097, 4097, 4097, 4097, 1, 3)),
                                      (23, (256, 257, 1023, 4097, 1, 3, 4, 5))])
def test_the_two_forms_agree_bit_for_bit(i, counts, ftn, dev):
    """A total both forms accept, under an active clip: the partial sums are added in one order."""
    runs = []
    for force in ("one", "grid", None):
        run = Run(ftn, dev, i, counts, 0.05, 0.01)
        for s in range(3):
            run.call(s, force_form=force)
        runs.append(run.bits() + [run.log.clone().view(torch.int32), run.state.clone()])
    assert _same(runs[0], runs[1]) and _same(runs[1], runs[2])
    assert float(run.log[0, 1]) > 0.05                          # the clip was active


@pytest.mark.parametrize("i,counts,force", [(19, (193, 255, 256, 257, 1023, 4097), None),
                                            (19, (193, 255, 256, 257, 1023, 4097), "grid"),
                                            (25, (4097, 1, 4097, 3, 4097, 5, 4097, 4097), None)])
def test_poisoned_workspace_between_guards(i, counts, force, ftn, dev):
    rt = ftn.runtime
    base = Run(ftn, dev, i, counts, 0.05, 0.01)
    run = Run(ftn, dev, i, counts, 0.05, 0.01)
    run.snapshot()
    log = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(rt, "_workspace", ws_poison.poisoned_workspace(0xFF, log))
        for s in range(2):
            run.call(s, force_form=force)
        assert ws_poison.check_guards(log) == 2
    for s in range(2):
        base.call(s, force_form=force)
    assert _same(run.bits(), base.bits())
    assert all(bool(torch.isfinite(t).all()) for t in run.p + run.m + run.v)
    run.around_is_untouched()
    assert log[0][1] == 8 * oracle.chunks(counts) + 16


@pytest.mark.parametrize("which", ["p", "g", "m", "v"])
@pytest.mark.parametrize("i,counts", [(15, (255, 257)), (21, (4097, 1023, 7, 4097, 5, 4097)),
                                      (24, (4097, 4097, 4097, 4097, 4097, 7, 193, 1023))])
def test_a_view_one_float_off_the_grid_equals_the_aligned_result(i, counts, which, ftn, dev):
    k = len(counts) - 1 if len(counts) < 6 else 3               # which tensor's operand is off
    base = Run(ftn, dev, i, counts, 0.05, 0.01)
    run = Run(ftn, dev, i, counts, 0.05, 0.01, off={(which, k): 1})
    assert base.form()[1] == 0 and run.form() == (base.form()[0], 1 << k, base.form()[2])
    assert run.misalign()[k] == 4
    run.snapshot()
    for s in range(3):
        base.call(s)
        run.call(s)
    assert _same(run.bits(), base.bits()) and torch.equal(run.log, base.log)
    run.around_is_untouched()


@pytest.mark.parametrize("force", ["one", "grid"])
def test_a_skipped_call_keeps_every_bit(force, ftn, dev):
    """Each trigger by itself: p, m, v and t keep every bit, ``calls`` advances, the log row has the flags."""
    i, counts = 15, (255, 257)
    run = Run(ftn, dev, i, counts, 0.05, 0.01, log_steps=16)
    word = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)
    loss = lambda v: torch.tensor([v], device=dev)
    run.call(0, loss=loss(1.5), skip=[word(0), word(0)], range_mask=2, force_form=force)
    before = run.bits()
    run.snapshot()
    nan_g, inf_g = run.grads(1), run.grads(1)
    nan_g[1][200] = float("nan")
    inf_g[0][7] = float("-inf")
    triggers = [(dict(skip=[word(1), word(0)], range_mask=2), 1), (dict(skip=[word(2), word(0)], range_mask=2), 2),
                (dict(skip=[word(3)]), 3), (dict(skip=[word(0), word(1)], range_mask=2), 4),
                (dict(skip=[word(0), word(65536)], range_mask=2), 4), (dict(grads=nan_g), 8), (dict(grads=inf_g), 8),
                (dict(loss=loss(float("nan"))), 8), (dict(loss=loss(float("inf"))), 8),
                (dict(skip=[word(1), word(1)], range_mask=2, loss=loss(float("nan"))), 13)]
    for kw, _ in triggers:
        kw.setdefault("loss", loss(2.5))
        run.call(1, force_form=force, **kw)
    assert _same(run.bits(), before)
    run.around_is_untouched()
    assert run.state.tolist() == [1, 1 + len(triggers)]
    log = run.log.cpu()
    assert log[:1 + len(triggers), 3].tolist() == [0.0] + [float(f) for _, f in triggers]
    assert float(log[0, 0]) == 1.5 and float(log[1, 0]) == 2.5 and bool(torch.isnan(log[6, 1]))
    # the next good call is the second update: the one a run without the skipped calls makes
    run.call(1, force_form=force)
    twin = Run(ftn, dev, i, counts, 0.05, 0.01)
    twin.call(0, force_form=force)
    twin.call(1, force_form=force)
    assert _same(run.bits(), twin.bits()) and run.state.tolist() == [2, 2 + len(triggers)]


def test_device_adamw_takes_the_hip_backend_and_bumps_versions(ftn, dev):
    fit = ftn.fit
    _param_key = ftn.models.timesnet._param_key
    ps, gs = oracle.case(15, (255, 257))
    P = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dev)) for p in ps]
    opt = fit.DeviceAdamW(P, lr=oracle.LR, betas=oracle.BETAS, eps=oracle.EPS, weight_decay=0.01, max_norm=0.05)
    run = Run(ftn, dev, 15, (255, 257), 0.05, 0.01)
    key = _param_key(P)
    for s in range(2):
        for p, g in zip(P, gs[s]):
            p.grad = torch.from_numpy(g).to(dev)
        opt.step()
        run.call(s)
        assert fit._last_optim_backend == "hip"
    assert _param_key(P) != key
    assert all(torch.equal(a.detach(), b) for a, b in zip(P + opt.exp_avg + opt.exp_avg_sq, run.p + run.m + run.v))
    assert opt.state_dict()["t"] == 2 and opt.history().shape == (2, 4)
    opt.set_lr(0.5)
    opt.step()
    assert opt.history()[:, 2].tolist() == [0.5]
    # the torch backend on the same device, asked for by name: within the same allowance of the kernel's result
    opt_t = fit.DeviceAdamW([p.detach().clone() for p in run.p], lr=oracle.LR, weight_decay=0.01, max_norm=0.05,
                            backend="torch")
    opt_t.load_state_dict({"t": 2, "exp_avg": run.m, "exp_avg_sq": run.v})
    opt_t.step_on(run.grads(2))
    run.call(2)
    assert fit._last_optim_backend == "torch"
    ref = oracle.reference_errors()[oracle.STEPS][0]
    assert max(float((a - b).abs().max()) for a, b in zip(opt_t.params, run.p)) <= 8.0 * ref
