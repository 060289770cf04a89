"""``fit.DeviceAdamW`` without a GPU: its ``torch`` backend against the fp64 restatement of the formulas
(tests/refit_oracle.py) within 4 times what torch's own fp32 ``clip_grad_norm_`` + ``AdamW(foreach=False)`` shows
against the same restatement on the same cases, the skip rule trigger by trigger as bit-equality, the version counters
``_param_key`` goes by, ``state_dict`` and the argument errors."""
import numpy as np
import pytest
import torch

import refit_oracle as oracle

# five steps, clip on and off, weight decay 0 and 0.01, small tensors in sets of 1, 2 and 6
TABLE = ((5,), (64,), (257,), (7, 64), (255, 257), (1, 3, 4, 5, 7, 64), (193, 255, 256, 257, 1023, 4097))


def _opt(ftn, ps, max_norm=None, wd=0.0, **kw):
    return ftn.fit.DeviceAdamW(ps, lr=oracle.LR, betas=oracle.BETAS, eps=oracle.EPS, weight_decay=wd,
                               max_norm=max_norm, **kw)


def test_the_reference_side_figure_is_not_zero():
    """The allowance is 4 times torch's own error against the restatement; ``reference_errors`` asserts that every
    one of its figures is above 0 for these inputs, so no comparison below is against an allowance of 0."""
    ref = oracle.reference_errors(TABLE)
    print("REFIT_ERR host: torch AdamW against fp64, largest |p|, |m|, |v| difference:", ref)
    assert set(ref) == {1, oracle.STEPS} and all(e > 0.0 for figures in ref.values() for e in figures)
    assert {(m is not None, wd) for _, _, m, wd in oracle.cases(list(TABLE))} >= {(True, 0.0), (True, 0.01),
                                                                                 (False, 0.0), (False, 0.01)}


@pytest.mark.parametrize("i,counts,max_norm,wd", oracle.cases(list(TABLE)))
def test_torch_backend_against_the_fp64_restatement(i, counts, max_norm, wd, ftn):
    ref = oracle.reference_errors(TABLE)
    ps, gs = oracle.case(i, counts)
    want = oracle.want64(i, counts, max_norm, wd)
    P = [torch.from_numpy(p.copy()) for p in ps]
    opt = _opt(ftn, P, max_norm, wd)
    for s in range(oracle.STEPS):
        opt.step_on([torch.from_numpy(g) for g in gs[s]])
        assert ftn.fit._last_optim_backend == "torch"
        if s + 1 in want:
            got = ([p.numpy() for p in P], [m.numpy() for m in opt.exp_avg], [v.numpy() for v in opt.exp_avg_sq])
            err = oracle.errors(got, want[s + 1])
            print(f"REFIT_ERR host case {i} {counts} after {s + 1}: |p| |m| |v| {err}, torch's own {ref[s + 1]}")
            assert all(e <= 4.0 * r for e, r in zip(err, ref[s + 1]))
    assert opt.state_dict()["t"] == oracle.STEPS
    hist = opt.history()
    assert hist.shape == (oracle.STEPS, 4) and bool((hist[:, 3] == 0).all()) and bool((hist[:, 2] == oracle.LR).all())
    norms = [np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in gs[s])) for s in range(oracle.STEPS)]
    np.testing.assert_allclose(hist[:, 1].numpy(), norms, rtol=1e-6)
    assert opt.history().shape == (0, 4)


def test_an_idle_clip_has_the_bits_of_no_clip(ftn):
    ps, gs = oracle.case(3, (7, 64))
    runs = []
    for max_norm in (None, 1e9):
        P = [torch.from_numpy(p.copy()) for p in ps]
        opt = _opt(ftn, P, max_norm, 0.01)
        for s in range(3):
            opt.step_on([torch.from_numpy(g) for g in gs[s]])
        runs.append(P + opt.exp_avg + opt.exp_avg_sq)
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def _bits(opt):
    return [t.clone() for t in opt.params + opt.exp_avg + opt.exp_avg_sq] + [opt._state[0:1].clone()]


@pytest.mark.parametrize("trigger,flag", [("bad_rate", 1), ("bad_dispersion", 2), ("bad_both", 3), ("range", 4),
                                          ("nan_gradient", 8), ("inf_gradient", 8), ("nan_loss", 8), ("inf_loss", 8)])
def test_skip_rule_keeps_every_bit(trigger, flag, ftn):
    ps, gs = oracle.case(4, (255, 257))
    P = [torch.from_numpy(p.copy()) for p in ps]
    opt = _opt(ftn, P, 0.5, 0.01, log_steps=4)
    good = [torch.from_numpy(g) for g in gs[0]]
    zero = torch.zeros(1, dtype=torch.int32)
    opt.step_on(good, loss=torch.tensor(1.5), skip=[zero, (zero.clone(), "range")])
    before = _bits(opt)
    grads, loss, skip = [g.clone() for g in good], torch.tensor(2.5), [zero, (zero.clone(), "range")]
    if trigger.startswith("bad"):
        skip[0] = torch.tensor([flag], dtype=torch.int32)
    elif trigger == "range":
        skip[1] = (torch.ones(1, dtype=torch.int32), "range")
    elif trigger.endswith("gradient"):
        grads[1][200] = float("nan") if trigger.startswith("nan") else float("inf")
    else:
        loss = torch.tensor(float("nan") if trigger.startswith("nan") else float("inf"))
    opt.step_on(grads, loss=loss, skip=skip)
    after = _bits(opt)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, after))
    assert opt._state.tolist() == [1, 2]                          # t stays, calls advances
    hist = opt.history()
    assert hist[:, 3].tolist() == [0.0, float(flag)] and float(hist[0, 0]) == 1.5
    # the next good call is the second update
    opt.step_on(good, loss=torch.tensor(0.5), skip=[zero])
    assert opt._state.tolist() == [2, 3] and not torch.equal(before[0], opt.params[0])
    assert opt.history()[:, 3].tolist() == [0.0]


def test_the_log_is_a_ring(ftn):
    ps, gs = oracle.case(0, (5,))
    opt = _opt(ftn, [torch.from_numpy(ps[0].copy())], log_steps=3)
    for s in range(5):
        opt.step_on([torch.from_numpy(gs[s][0])], loss=torch.tensor(float(s)))
    assert opt.history()[:, 0].tolist() == [2.0, 3.0, 4.0]        # the last three of five


def test_param_key_changes_with_a_step_and_grad_interface(ftn):
    _param_key = ftn.models.timesnet._param_key

    lin = torch.nn.Linear(4, 3)
    ps = list(lin.parameters())
    opt = _opt(ftn, ps)
    key = _param_key(ps)
    lin(torch.ones(2, 4)).sum().backward()
    opt.step()
    assert _param_key(ps) != key and all(a[0] == b[0] for a, b in zip(key, _param_key(ps)))
    opt.zero_grad()
    assert all(p.grad is None for p in ps)
    with pytest.raises(ValueError, match="no parameter has a gradient"):
        opt.step()
    lin(torch.ones(2, 4)).sum().backward()
    opt.zero_grad(set_to_none=False)
    assert all(p.grad is not None and float(p.grad.abs().sum()) == 0.0 for p in ps)
    # set_lr is what the next update uses
    opt.set_lr(0.25)
    opt.step()
    assert opt.history()[:, 2].tolist() == [oracle.LR, 0.25]


def test_state_dict_round_trip(ftn):
    ps, gs = oracle.case(3, (7, 64))
    grads = [[torch.from_numpy(g) for g in step] for step in gs]
    a = _opt(ftn, [torch.from_numpy(p.copy()) for p in ps], 0.5, 0.01)
    for s in range(3):
        a.step_on(grads[s])
    state = a.state_dict()
    assert state["t"] == 3 and len(state["exp_avg"]) == len(state["exp_avg_sq"]) == 2
    b = _opt(ftn, [p.clone() for p in a.params], 0.5, 0.01)
    b.load_state_dict(state)
    state["exp_avg"][0].zero_()                                   # the state is a copy on both sides
    a.step_on(grads[3])
    b.step_on(grads[3])
    assert all(torch.equal(x, y) for x, y in zip(a.params + a.exp_avg + a.exp_avg_sq,
                                                 b.params + b.exp_avg + b.exp_avg_sq))
    assert b.state_dict()["t"] == 4
    with pytest.raises(ValueError, match="another number of parameters"):
        _opt(ftn, [torch.zeros(3)]).load_state_dict(state)


def test_argument_errors(ftn):
    fit = ftn.fit
    p = torch.zeros(4)
    with pytest.raises(ValueError, match=r"\(1\.\.8\)"):
        fit.DeviceAdamW([])
    with pytest.raises(ValueError, match=r"\(1\.\.8\)"):
        fit.DeviceAdamW([torch.zeros(2) for _ in range(9)])
    with pytest.raises(ValueError, match="not empty"):
        fit.DeviceAdamW([torch.zeros(0)])
    with pytest.raises(ValueError, match="floating-point"):
        fit.DeviceAdamW([torch.zeros(3, dtype=torch.int32)])
    with pytest.raises(ValueError, match="betas"):
        fit.DeviceAdamW([p], betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="must be >= 0"):
        fit.DeviceAdamW([p], weight_decay=-1.0)
    with pytest.raises(ValueError, match="log_steps"):
        fit.DeviceAdamW([p], log_steps=0)
    with pytest.raises(ValueError, match="backend"):
        fit.DeviceAdamW([p], backend="triton")
    opt = fit.DeviceAdamW([p])
    with pytest.raises(ValueError, match="2 gradients for 1 parameters"):
        opt.step_on([p, p])
    with pytest.raises(ValueError, match="shape and device"):
        opt.step_on([torch.zeros(5)])
    with pytest.raises(ValueError, match="skip word"):
        opt.step_on([p], skip=[torch.zeros(1)])
    with pytest.raises(ValueError, match="'range'"):
        opt.step_on([p], skip=[(torch.zeros(1, dtype=torch.int32), "bad")])
    with pytest.raises(ValueError, match="loss must be one"):
        opt.step_on([p], loss=torch.zeros(2))
    with pytest.raises(ValueError, match="backend 'hip' takes"):
        fit.DeviceAdamW([p], backend="hip").step_on([p])
    assert opt._state.tolist() == [0, 0]                          # nothing ran
    with pytest.raises(ValueError, match="needs a fit.DeviceAdamW"):
        fit.GraphedRefitStep(None, None, torch.optim.Adam([p.requires_grad_()]))
    with pytest.raises(ValueError, match="learning rates for 2 epochs"):
        fit.refit_output_graphed(torch.nn.Linear(1, 1), [], epochs=2, lr=[1e-3])
