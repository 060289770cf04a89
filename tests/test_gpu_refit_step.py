"""``fit.GraphedRefitStep`` and ``fit.refit_output_graphed`` on the MI355X, on the tiny model of tests/test_gpu_fit.py
with 1 and 5 series: the captured step's six gradients against the ``.grad``s of the eager ``fit.output_nll`` backward
(bits), replayed steps against the same updates made eagerly (bits), five steps against the parent's ``refit_output``
under torch's ``AdamW(foreach=False)`` with clip and weight decay, and - on the d_model 64 model of
tests/test_gpu_range.py - a batch that trips the f16x2 range word.

The five-step case prints ``REFIT_STEP`` with its two distances (tools/refit_step_time.py records them in
profiles/refit_step_error.json)."""
import copy

import pytest
import torch

from test_gpu_fit import _tiny_model

pytestmark = pytest.mark.gpu

LR, WD, CLIP = 1e-2, 0.01, 0.05


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _six(m):
    return [m.mu_head.weight, m.mu_head.bias, m.sigma_head.weight, m.sigma_head.bias, m.forecast_time_proj.weight,
            m.forecast_time_proj.bias]


def _on(dev, batches):
    return [tuple(t.to(dev) for t in b) for b in batches]


def _eager_grads(fit, model, batch):
    """The ``.grad``s ``fit.output_nll(...).backward()`` leaves in the six tensors, and the loss."""
    x, yb, mk = batch
    steps = model._out_steps
    ps = _six(model)
    for p in ps:
        p.requires_grad_(True)
        p.grad = None
    seq, tail, hist, late, floor = model.output_inputs(x)
    proj = model.forecast_time_proj
    loss, bad = fit.output_nll(seq, proj.weight[-steps:], proj.bias[-steps:], *ps[:4], tail, hist, yb[:, :steps, :],
                               mk[:, :steps, :] > 0.0, late, floor, model.min_sigma)
    loss.backward()
    assert fit._last_timeproj_backend == "hip" and fit._last_head_backend == "hip" and int(bad) == 0
    return [p.grad.clone() for p in ps], loss.detach().clone()


@pytest.mark.parametrize("N", [1, 5])
def test_captured_gradients_have_the_bits_of_the_eager_backward(N, ftn, dev):
    fit = ftn.fit
    model, batches = _tiny_model(ftn, N, dev)
    batches = _on(dev, batches)
    twin = copy.deepcopy(model)
    want, want_loss = _eager_grads(fit, twin, batches[0])
    opt = fit.DeviceAdamW(_six(model), lr=LR, weight_decay=WD, max_norm=CLIP)
    before = [p.detach().clone() for p in _six(model)]
    step = fit.GraphedRefitStep(model, batches[0], opt, use_loss_mask=True)
    assert fit._last_optim_backend == "hip"
    # warm-up and capture moved nothing
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, _six(model)))
    assert opt._state.tolist() == [0, 0] and not any(bool(m.any()) for m in opt.exp_avg + opt.exp_avg_sq)
    key = ftn.models.timesnet._param_key(_six(model))
    loss = step.step(batches[0])
    assert all(blk._last_backend == "hip" for blk in model.blocks)
    assert len(step.grads) == 6
    for name, a, b in zip(("w_mu", "b_mu", "w_sigma", "b_sigma", "w_t", "b_t"), step.grads, want):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert torch.equal(loss.reshape(()), want_loss) and int(step.bad) == 0
    assert opt._state.tolist() == [1, 1] and ftn.models.timesnet._param_key(_six(model)) != key
    assert all(not torch.equal(a, b.detach()) for a, b in zip(before, _six(model)))
    # the same update made by the eager optimizer call from those gradients
    opt2 = fit.DeviceAdamW(_six(twin), lr=LR, weight_decay=WD, max_norm=CLIP)
    opt2.step()
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(_six(model), _six(twin)))
    # what is frozen at capture
    x, yb, mk = batches[0]
    with pytest.raises(ValueError, match="x is"):
        step.step((x[:2], yb, mk))
    with pytest.raises(ValueError, match="x_mark is"):
        step.step((x, yb, mk, torch.zeros(4, 24, 2, device=dev), None))
    assert step.fits(batches[1]) and not step.fits((x[:2], yb[:2], mk[:2]))
    assert step.inputs[0].shape == x.shape and step.inputs[3] is None


@pytest.mark.parametrize("N", [1, 5])
def test_replayed_steps_have_the_bits_of_the_eager_steps(N, ftn, dev):
    """Three replays over three batches against ``refit_output`` with the same ``DeviceAdamW`` settings: the same
    launches on the same operands, once replayed and once enqueued one by one."""
    fit = ftn.fit
    model, batches = _tiny_model(ftn, N, dev)
    batches = _on(dev, batches)
    twin = copy.deepcopy(model)
    opt = fit.DeviceAdamW(_six(model), lr=LR, weight_decay=WD, max_norm=CLIP)
    step = fit.GraphedRefitStep(model, batches[0], opt, use_loss_mask=True)
    losses = torch.cat([step.step(b).clone() for b in batches]).cpu()
    eager = fit.refit_output(twin, batches, lr=LR, use_loss_mask=True,
                             optimizer=fit.DeviceAdamW(_six(twin), lr=LR, weight_decay=WD, max_norm=CLIP))
    assert torch.equal(losses, eager)
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(_six(model), _six(twin)))
    hist = opt.history()
    assert hist.shape == (3, 4) and torch.equal(hist[:, 0], losses) and not hist[:, 3].any()
    assert bool((hist[:, 1] > CLIP).all())                      # the clip was active


@pytest.mark.parametrize("N", [1, 5])
def test_five_steps_against_the_parents_loop_under_torch_adamw(N, ftn, dev):
    """``refit_output_graphed`` against an fp64-master run: parameters and moments kept in fp64 by torch's AdamW and
    rounded to fp32 only for the kernels.  ``d_ref`` is the distance of the parent's fp32 loop (``refit_output`` with
    ``AdamW(foreach=False)`` and ``grad_clip``) to that run; neither involves the code under test.  The graphed result
    must be within ``4 d_ref + 5 2^-23 max|p|`` of the fp64-master run."""
    fit = ftn.fit
    model, batches = _tiny_model(ftn, N, dev)
    batches = _on(dev, batches)
    five = [batches[i % 3] for i in range(5)]
    # the parent's fp32 loop
    parent = copy.deepcopy(model)
    fit.refit_output(parent, five, use_loss_mask=True, grad_clip=CLIP,
                     optimizer=torch.optim.AdamW(_six(parent), lr=LR, weight_decay=WD, foreach=False))
    # the fp64-master run, from the parent's gradients
    twin = copy.deepcopy(model)
    master = [p.detach().double().clone().requires_grad_() for p in _six(twin)]
    opt64 = torch.optim.AdamW(master, lr=LR, weight_decay=WD, foreach=False)
    for batch in five:
        with torch.no_grad():
            for p, q in zip(_six(twin), master):
                p.copy_(q.float())
        grads, _ = _eager_grads(fit, twin, batch)
        for q, g in zip(master, grads):
            q.grad = g.double()
        torch.nn.utils.clip_grad_norm_(master, CLIP, foreach=False)
        opt64.step()
    # the code under test
    losses = fit.refit_output_graphed(model, five, lr=LR, weight_decay=WD, grad_clip=CLIP, use_loss_mask=True)
    assert losses.shape == (5,) and bool(torch.isfinite(losses).all()) and not model.training
    dist = lambda ps: max(float((p.detach().double() - q.detach()).abs().max()) for p, q in zip(ps, master))
    d_ref, d_got = dist(_six(parent)), dist(_six(model))
    top = max(float(q.detach().abs().max()) for q in master)
    print(f"REFIT_STEP N={N}: five steps, graphed to the fp64-master run {d_got:.3e}, the parent's fp32 loop to it "
          f"{d_ref:.3e}, max|p| {top:.3e}")
    assert d_got <= 4.0 * d_ref + 5.0 * 2.0 ** -23 * top


def test_loop_invariants_rates_per_epoch_and_a_short_last_batch(ftn, dev):
    fit = ftn.fit
    model, batches = _tiny_model(ftn, 5, dev)
    batches = _on(dev, batches)
    short = tuple(t[:3] for t in batches[2])
    before = {k: v.clone() for k, v in model.state_dict().items()}
    flags = [p.requires_grad for p in model.parameters()]
    model.train()
    losses = fit.refit_output_graphed(model, batches[:2] + [short], epochs=2, lr=[1e-2, 5e-3], use_loss_mask=True)
    assert losses.shape == (6,) and losses.device.type == "cpu" and bool(torch.isfinite(losses).all())
    assert [p.requires_grad for p in model.parameters()] == flags and model.training
    for k, v in model.state_dict().items():
        changed = not torch.equal(v, before[k])
        assert changed == k.startswith(("forecast_time_proj.", "mu_head.", "sigma_head.")), k
    assert float(losses[3:].mean()) < float(losses[:3].mean())
    with pytest.raises(ValueError, match="no batches"):
        fit.refit_output_graphed(model, [], lr=1e-2)


def test_a_replay_that_trips_the_range_word_moves_nothing(ftn, dev):
    """One 1e6 value in x: its embedding row leaves the fp16 range of engine f16x2 inside the replay.  The update is
    skipped on the device, flag 4 is logged, and the loop raises.  The model is the d_model 64 one of
    tests/test_gpu_range.py: at the tiny model's d_model of 16 no input trips the word, eagerly or captured (an
    input scaled by 1e6 runs through ``output_inputs`` without the warning), so there is nothing to skip there."""
    from test_gpu_range import _model

    fit = ftn.fit
    model, x = _model(ftn, dev)
    g = torch.Generator().manual_seed(5)
    yb = torch.poisson(torch.full((4, 8, 16), 2.0), generator=g).to(dev)
    mk = (torch.rand(4, 8, 16, generator=g) >= 0.2).float().to(dev)
    batches = [(x, yb, mk), (x.flip(0), yb, mk), (x.roll(1, 0), yb, mk)]
    assert all(b._engine_name() == "f16x2" for b in model.blocks)
    opt = fit.DeviceAdamW(_six(model), lr=LR, weight_decay=WD, max_norm=CLIP)
    step = fit.GraphedRefitStep(model, batches[0], opt, use_loss_mask=True)
    assert len(step.range_words) == len(model.blocks)
    step.step(batches[0])
    six = _six(model) + opt.exp_avg + opt.exp_avg_sq
    before = [t.detach().clone() for t in six]
    hot = batches[1][0].clone()
    hot[1, 7, 2] = 1e6
    step.step((hot, yb, mk))
    words = [int(w) for w in step.range_words]
    print("REFIT_STEP range words after the hot replay:", words)
    assert any(words)
    assert all(torch.equal(a.view(torch.int32), b.detach().view(torch.int32)) for a, b in zip(before, six))
    assert opt._state.tolist() == [1, 2]
    hist = opt.history()
    assert int(hist[0, 3]) == 0 and int(hist[1, 3]) & 4
    # the words are zeroed by the replay itself: the next batch updates again
    step.step(batches[2])
    assert opt._state.tolist() == [2, 3] and int(opt.history()[0, 3]) == 0
    # the `bad` word directly through step_on
    opt.step_on([torch.zeros_like(p) for p in _six(model)],
                skip=[torch.tensor([2], dtype=torch.int32, device=dev)])
    assert opt._state.tolist() == [2, 4] and int(opt.history()[0, 3]) == 2
    fresh, _ = _model(ftn, dev)
    with pytest.raises(FloatingPointError, match="fp16 range of engine f16x2"):
        fit.refit_output_graphed(fresh, [batches[0], (hot, yb, mk)], lr=LR, use_loss_mask=True)
    assert all(b._engine_name() == "f16x2" for b in fresh.blocks) and not fresh.training
