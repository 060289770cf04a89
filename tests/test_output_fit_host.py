"""The output refit on the host (no GPU): the torch fallback of ``fit.time_projection`` / ``fit.output_nll`` against
autograd of the plain composition to the bit, ``fit.refit_output`` on a CPU model (what moves, what comes back, the
recursive model's one row, gradient clipping), and the reference anchor: the gradients the reference's own autograd
left in the six output-side tensors (tests/golden/output_grad_n<N>.npz, written by make_golden_output_grad.py) against
``fit.output_nll`` from the recorded ``seq``, within twice the composed bound of tests/output_fit_oracle.py."""
import copy
import json

import numpy as np
import pytest
import torch

import output_fit_oracle as oracle
from conftest import GOLDEN

L, H = 24, 4
OUT = ("forecast_time_proj.", "mu_head.", "sigma_head.")


def _tiny(ftn, N, mode="direct", seed=1):
    """tests/test_gpu_fit.py's ``_tiny_model`` on the CPU, in either mode."""
    cfg = dict(input_len=L, pred_len=H, d_model=16, d_ff=32, n_layers=2, k_periods=3, kernel_set=[(3, 3), (5, 5)],
               dropout=0.0, activation="gelu", mode=mode, use_checkpoint=False)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(0)
    model = ftn.models.TimesNet(**cfg).eval()
    with torch.no_grad():
        model(torch.rand(2, L, N, generator=g) + 1.0)
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    t = torch.arange(L, dtype=torch.float32).view(1, L, 1)
    batches = []
    for _ in range(3):
        x = torch.rand(4, L, N, generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 6.0)
        yb = torch.poisson(torch.full((4, H, N), 2.0), generator=g)
        batches.append((x, yb, (torch.rand(4, H, N, generator=g) >= 0.2).float()))
    return model, batches


def _six(model):
    steps = model._out_steps
    return [model.forecast_time_proj.weight[-steps:], model.forecast_time_proj.bias[-steps:], model.mu_head.weight,
            model.mu_head.bias, model.sigma_head.weight, model.sigma_head.bias]


@pytest.mark.parametrize("S", [1, 4])
def test_torch_fallback_is_the_plain_composition_to_the_bit(S, ftn):
    fit = ftn.fit
    g = torch.Generator().manual_seed(3 + S)
    B, Lx, D, N = 3, 7, 8, 2
    seq = torch.randn(B, Lx, D, generator=g)
    full_w, full_b = torch.randn(4, Lx, generator=g).requires_grad_(), torch.randn(4, generator=g).requires_grad_()
    heads = [(0.2 * torch.randn(s, generator=g)).requires_grad_() for s in ((N, D), (N,), (N, D), (N,))]
    tail = torch.rand(B, S, N, generator=g) + 0.5
    y = torch.poisson(torch.full((B, S, N), 2.0), generator=g)
    mask = torch.rand(B, S, N, generator=g) >= 0.2
    fit._last_timeproj_backend = None
    hidden = fit.time_projection(seq, full_w[-S:], full_b[-S:])
    assert fit._last_timeproj_backend == "torch" and hidden.requires_grad and hidden.shape == (B, S, D)
    plain = torch.matmul(full_w[-S:], seq) + full_b[-S:].view(1, -1, 1)
    assert torch.equal(hidden, plain)
    loss, bad = fit.output_nll(seq, full_w[-S:], full_b[-S:], *heads, tail, S, y, mask)
    assert fit._last_timeproj_backend == "torch" and fit._last_head_backend == "torch" and int(bad) == 0
    got = torch.autograd.grad(loss, [full_w, full_b] + heads)
    want_loss, _ = fit.head_nll(plain, *heads, tail, S, y, mask)
    want = torch.autograd.grad(want_loss, [full_w, full_b] + heads)
    assert torch.equal(loss, want_loss) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert not bool(got[0][:4 - S].any()) and not bool(got[1][:4 - S].any())    # the other rows: exact zeros
    assert bool(got[0][4 - S:].any()) and bool(got[1][4 - S:].any())
    with pytest.raises(ValueError, match="time_projection: seq"):
        fit.time_projection(seq, full_w[:, :3], full_b)


@pytest.mark.parametrize("mode", ["direct", "recursive"])
def test_refit_output_moves_the_output_side_alone(mode, ftn):
    fit = ftn.fit
    model, batches = _tiny(ftn, 5, mode)
    model.train()
    list(model.parameters())[0].requires_grad_(False)
    flags = [p.requires_grad for p in model.parameters()]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    seq, tail, hist, late, floor = model.output_inputs(batches[0][0])
    assert seq.shape == (4, L, 16) and seq.is_contiguous() and not seq.requires_grad
    hidden = model.head_inputs(batches[0][0])[0]
    steps = model._out_steps
    assert steps == (H if mode == "direct" else 1) and hist == steps and tail.shape == (4, steps, 5)
    with torch.no_grad():
        assert torch.equal(hidden, fit.time_projection(seq, *_six(model)[:2]))
    losses = fit.refit_output(model, batches, epochs=2, lr=1e-2, use_loss_mask=True)
    assert fit._last_timeproj_backend == "torch" and fit._last_head_backend == "torch"
    assert losses.shape == (6,) and bool(torch.isfinite(losses).all())
    assert float(losses[3:].mean()) < float(losses[:3].mean())
    assert [p.requires_grad for p in model.parameters()] == flags and model.training
    after = model.state_dict()
    for k, v in after.items():
        assert (not torch.equal(v, before[k])) == k.startswith(OUT), k
    if mode == "recursive":                                     # only the last row / entry of the projection moved
        w0, b0 = before["forecast_time_proj.weight"], before["forecast_time_proj.bias"]
        assert torch.equal(after["forecast_time_proj.weight"][:-1], w0[:-1]) and torch.equal(
            after["forecast_time_proj.bias"][:-1], b0[:-1])
        assert not torch.equal(after["forecast_time_proj.weight"][-1], w0[-1]) and \
            after["forecast_time_proj.bias"][-1] != b0[-1]
    with pytest.raises(ValueError, match="refit_output: no batches"):
        fit.refit_output(model, [])
    with pytest.raises(ValueError, match="use_loss_mask needs a mask"):
        fit.refit_output(model, [batches[0][:2] + (None,)], use_loss_mask=True)


def test_grad_clip_is_the_references_clipping(ftn):
    """One SGD step (Adam's step would hide a rescaled gradient): a threshold below the first step's gradient norm
    changes the result - it is the unclipped step scaled by threshold / norm - and a huge one changes no bit."""
    fit = ftn.fit
    model, batches = _tiny(ftn, 5)
    x, yb, mk = batches[0]
    seq, tail, hist, late, floor = model.output_inputs(x)
    ps = [p.detach().clone().requires_grad_() for p in _six(model)]
    loss, _ = fit.output_nll(seq, *ps, tail, hist, yb, mk > 0, late, floor, model.min_sigma)
    norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in torch.autograd.grad(loss, ps))))
    assert norm > 0.0

    def run(clip):
        twin = copy.deepcopy(model)
        params = [twin.mu_head.weight, twin.mu_head.bias, twin.sigma_head.weight, twin.sigma_head.bias,
                  twin.forecast_time_proj.weight, twin.forecast_time_proj.bias]
        fit.refit_output(twin, [batches[0]], use_loss_mask=True, optimizer=torch.optim.SGD(params, lr=0.5),
                         grad_clip=clip)
        return [p.detach().clone() for p in params]

    start = [model.mu_head.weight, model.mu_head.bias, model.sigma_head.weight, model.sigma_head.bias,
             model.forecast_time_proj.weight, model.forecast_time_proj.bias]
    free, huge, half = run(None), run(1e30), run(0.5 * norm)
    assert all(torch.equal(a, b) for a, b in zip(free, huge))
    assert not all(torch.equal(a, b) for a, b in zip(free, half))
    # half the step: each update rounds once at |p| < 2 (2^-23 and half of it), the factor is 0.5 norm / (norm + 1e-6)
    for p0, a, b in zip(start, free, half):
        assert float(p0.detach().abs().max()) < 2.0
        torch.testing.assert_close(b - p0.detach(), 0.5 * (a - p0.detach()), rtol=1e-4, atol=1.5 * 2.0 ** -23)


@pytest.mark.parametrize("N", [1, 5])
def test_gradients_against_the_references_autograd(N, ftn):
    """Both sides are fp32 evaluations of one function, each within one composed bound of the fp64 composition (the
    generator checked the reference's side): twice the bound between them."""
    fit = ftn.fit
    with np.load(GOLDEN / f"output_grad_n{N}.npz") as z:
        z = {k: z[k] for k in z.files}
    cfg = json.loads(str(z["config_json"]))
    cfg["kernel_set"] = [tuple(k) for k in cfg["kernel_set"]]
    x, y, mask, seq = (torch.from_numpy(z[k]) for k in ("x", "y", "mask", "seq"))
    sd = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd:")}
    with torch.no_grad():
        torch.manual_seed(1)
        mine = ftn.models.TimesNet(**cfg).eval()
        mine(x)
        assert set(mine.state_dict().keys()) == set(sd)
        mine.load_state_dict(sd, strict=True)
    _, tail, hist, late, floor = mine.head_inputs(x)
    named = dict(mine.named_parameters())
    ps = [named[k].detach().clone().requires_grad_() for k in oracle.NAMES]
    loss, bad = fit.output_nll(seq, *ps, tail, hist, y, mask > 0, late, floor, mine.min_sigma)
    assert fit._last_timeproj_backend == "torch" and int(bad) == 0
    got = torch.autograd.grad(loss, ps)
    ref = [torch.from_numpy(z[f"grad:{k}"]) for k in oracle.NAMES]
    loss64, want64, bounds = oracle.grads_and_bounds(fit, seq, ps, tail, hist, y, mask > 0, late, floor, mine.min_sigma)
    D, Lx = seq.shape[2], seq.shape[1]
    assert abs(float(loss.detach()) - float(z["loss"])) <= 2 * 64 * (D + 8 + Lx + 8) * oracle.U * abs(float(loss64))
    ours, theirs = oracle.fraction(got, want64, bounds), oracle.fraction(ref, want64, bounds)
    between = oracle.fraction(got, [r.double() for r in ref], bounds)
    print(f"OUTFIT_ERR reference anchor N={N}: fraction of the composed bound, ours against fp64 {ours:.4f}, the "
          f"reference against fp64 {theirs:.4f}, ours against the reference (allowed 2) {between:.4f}")
    assert between <= 2.0 and theirs <= 1.0
