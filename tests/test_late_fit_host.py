"""The late-bias refit without a GPU: ``fit.late_bias`` (torch backend) against fp64 autograd of the composition,
torch's own fp32 autograd inside the a-priori bounds of tests/late_fit_oracle.py (the oracle's soundness check), the
exactness lattice, ``TimesNet.late_rows``, ``fit.refit_output(..., late_bias=True)`` on a tiny model with ids and
statics, ``fit.DeviceAdamWList`` (torch backend) against the fp64 restatement of tests/refit_oracle.py and against
``fit.DeviceAdamW`` bit for bit, and the argument errors."""
import copy

import numpy as np
import pytest
import torch

import late_fit_oracle as oracle
import refit_oracle


def late_model(ftn, N=5, dev="cpu", seed=1, head=True):
    """``test_gpu_fit._tiny_model`` with ids and statics: ``(model, batches)``, the batches 7-tuples ``(x, y, mask,
    None, None, static [N, 3], ids [N])``."""
    L, H = 24, 4
    cfg = dict(input_len=L, pred_len=H, d_model=16, d_ff=32, n_layers=2, k_periods=3, kernel_set=[(3, 3), (5, 5)],
               dropout=0.0, activation="gelu", mode="direct", use_checkpoint=False, id_embed_dim=8, static_proj_dim=4,
               use_late_bias_head=head)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(0)
    model = ftn.models.TimesNet(**cfg).eval()
    static = torch.randn(N, 3, generator=g)
    ids = torch.arange(N)
    with torch.no_grad():
        model(torch.rand(2, L, N, generator=g) + 1.0, None, static, ids)
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    t = torch.arange(L, dtype=torch.float32).view(1, L, 1)
    batches = []
    for _ in range(3):
        x = torch.rand(4, L, N, generator=g) + 1.5 + torch.sin(2 * torch.pi * t / 6.0)
        yb = torch.poisson(torch.full((4, H, N), 2.0), generator=g)
        batches.append((x, yb, (torch.rand(4, H, N, generator=g) >= 0.2).float(), None, None, static, ids))
    return model.to(dev), batches


def late_params(model):
    return [model.late_bias_norm.weight, model.late_bias_norm.bias, model.late_bias_head.weight,
            model.late_bias_head.bias, model.late_bias_gate]


def test_the_grid_walks_every_axis():
    for k, axis in enumerate((oracle.CTXS, oracle.SS, oracle.RS, oracle.LAYOUTS)):
        assert {c[k] for c in oracle.GRID} == set(axis)


@pytest.mark.parametrize("i", range(len(oracle.GRID)))
def test_torch_backend_and_torch_autograd_lie_inside_the_bound(i, ftn):
    """``fit.late_bias`` on CPU tensors is the torch composition; its fp32 gradients - torch's own autograd - lie
    inside the oracle's bound, which is the check that the bound is sound for an fp32 implementation."""
    rows, params, d_pre = oracle.case(i)
    want, bounds = oracle.grads_and_bounds(rows, params, d_pre)
    ps = [p.clone().requires_grad_() for p in params]
    late = ftn.fit.late_bias(rows, *ps, oracle.EPS)
    assert ftn.fit._last_late_backend == "torch" and late.shape == (rows.shape[0], ps[2].shape[0], rows.shape[1])
    assert torch.allclose(late.double(), oracle.late64(rows, [p.double() for p in params]), rtol=1e-4, atol=1e-5)
    (late * d_pre).sum().backward()
    frac = oracle.fraction([p.grad for p in ps], want, bounds)
    print(f"LATEFIT_ERR host grid {i} {oracle.GRID[i]}: torch fp32 autograd, fraction of the bound {frac:.4f}")
    assert frac <= 1.0


def test_the_index_form_is_the_gathered_call(ftn):
    rows, params, _ = oracle.case(3)
    store = rows.reshape(-1, rows.shape[-1])
    index = torch.tensor([5, 0, 5, 200, 17])
    a = ftn.fit.late_bias(store, *params, oracle.EPS, index=index)
    b = ftn.fit.late_bias(store[index].unsqueeze(1), *params, oracle.EPS)
    assert a.shape == (5, params[2].shape[0], 1) and torch.equal(a, b)


def test_the_lattice_is_exact_in_fp32_torch():
    """The exactness case's own premise, on the CPU: the rows normalise exactly and fp32 autograd of the composition
    reproduces the int64 lattice."""
    rows, params, d_pre, want = oracle.lattice_case(oracle.CHUNK + 1)
    p = [t.clone().requires_grad_() for t in params]
    lb = torch.nn.functional.linear(torch.nn.functional.layer_norm(rows, (rows.shape[-1],), p[0], p[1], 0.0), p[2], p[3])
    ((p[4].reshape(1, -1, 1) * lb.transpose(1, 2)) * d_pre).sum().backward()
    for name, got in (("dgamma", p[0].grad), ("dbeta", p[1].grad), ("dW", p[2].grad), ("db", p[3].grad),
                      ("dgate", p[4].grad.reshape(-1))):
        assert torch.equal(got.double(), want[name].double()), name


def test_late_bias_argument_errors(ftn):
    rows, params, _ = oracle.case(1)
    fit = ftn.fit
    with pytest.raises(ValueError, match="late_bias: rows"):
        fit.late_bias(rows[0], *params, oracle.EPS)
    with pytest.raises(ValueError, match="late_bias: index"):
        fit.late_bias(rows[0], *params, oracle.EPS, index=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="do not fit"):
        fit.late_bias(rows, params[0][:-1], *params[1:], oracle.EPS)
    with pytest.raises(ValueError, match="do not fit"):
        fit.late_bias(rows, *params[:4], params[4].reshape(-1, 1), oracle.EPS)


def test_late_rows_are_the_rows_the_model_reads(ftn):
    model, batches = late_model(ftn)
    x, _, _, _, _, static, ids = batches[0]
    rows = model.late_rows(x, None, static, ids)
    assert rows.shape == (1, 5, 12) and not rows.requires_grad
    late = ftn.fit.late_bias(rows, *late_params(model), model.late_bias_norm.eps)
    assert torch.equal(late.detach(), model.output_inputs(x, None, static, ids)[3])
    plain = late_model(ftn, head=False)[0]
    assert plain.late_rows(x, None, static, ids) is None


def test_refit_output_moves_all_eleven_and_nothing_else(ftn):
    model, batches = late_model(ftn)
    model.train()
    model.mu_head.bias.requires_grad_(False)
    before = copy.deepcopy(model.state_dict())
    flags = {n: p.requires_grad for n, p in model.named_parameters()}
    losses = ftn.fit.refit_output(model, batches * 2, epochs=1, lr=2e-2, late_bias=True, grad_clip=1.0)
    assert losses.shape == (6,) and bool(torch.isfinite(losses).all())
    assert model.training and {n: p.requires_grad for n, p in model.named_parameters()} == flags
    moved = {"mu_head.weight", "mu_head.bias", "sigma_head.weight", "sigma_head.bias", "forecast_time_proj.weight",
             "forecast_time_proj.bias", "late_bias_norm.weight", "late_bias_norm.bias", "late_bias_head.weight",
             "late_bias_head.bias", "late_bias_gate"}
    after = model.state_dict()
    assert moved <= set(after)
    for name, t in after.items():
        assert torch.equal(t, before[name]) == (name not in moved), name
    # five steps on one batch: the loss comes down
    model, batches = late_model(ftn)
    losses = ftn.fit.refit_output(model, batches[:1] * 5, lr=2e-2, late_bias=True)
    assert float(losses[4]) < float(losses[0])
    # the flag off: the six tensors, the late bias a constant (the call as it was)
    model, batches = late_model(ftn)
    before = copy.deepcopy(model.state_dict())
    ftn.fit.refit_output(model, batches, lr=2e-2)
    for name in ("late_bias_norm.weight", "late_bias_head.weight", "late_bias_gate"):
        assert torch.equal(model.state_dict()[name], before[name])


def test_refit_output_without_the_head_is_a_value_error(ftn):
    model, batches = late_model(ftn, head=False)
    with pytest.raises(ValueError, match="late_bias=True: the model has no late-bias head"):
        ftn.fit.refit_output(model, batches, late_bias=True)


ELEVEN = (4097, 1, 3, 4, 5, 7, 64, 193, 4097, 255, 1023)          # a record boundary after the eighth


def _run_list(ftn, cls, counts, i, max_norm, wd):
    ps, gs = refit_oracle.case(i, counts)
    P = [torch.from_numpy(p.copy()) for p in ps]
    opt = cls(P, lr=refit_oracle.LR, betas=refit_oracle.BETAS, eps=refit_oracle.EPS, weight_decay=wd, max_norm=max_norm)
    out = {}
    for s in range(refit_oracle.STEPS):
        opt.step_on([torch.from_numpy(g) for g in gs[s]])
        assert ftn.fit._last_optim_backend == "torch"
        if s + 1 in (1, refit_oracle.STEPS):
            out[s + 1] = ([p.numpy().copy() for p in P], [m.numpy().copy() for m in opt.exp_avg],
                          [v.numpy().copy() for v in opt.exp_avg_sq])
    return out, opt


LIST_TABLE = (ELEVEN,) * len(refit_oracle.HYPERS)                # every (max_norm, weight_decay) of the oracle once


@pytest.mark.parametrize("i,counts,max_norm,wd", refit_oracle.cases(list(LIST_TABLE)))
def test_device_adamw_list_eleven_against_the_fp64_restatement(i, counts, max_norm, wd, ftn):
    """Eleven tensors, under the rule of tests/refit_oracle.py: at most 4 times what torch's own fp32 optimizer shows
    against the restatement over the same cases."""
    ref = refit_oracle.reference_errors(LIST_TABLE)
    got, opt = _run_list(ftn, ftn.fit.DeviceAdamWList, counts, i, max_norm, wd)
    want = refit_oracle.want64(i, counts, max_norm, wd)
    for k in want:
        err = refit_oracle.errors(got[k], want[k])
        print(f"REFIT_ERR host list case {i} {max_norm} {wd} after {k}: |p| |m| |v| {err}, torch's own {ref[k]}")
        assert all(e <= 4.0 * r for e, r in zip(err, ref[k]))
    assert opt.state_dict()["t"] == refit_oracle.STEPS and opt.history().shape == (refit_oracle.STEPS, 4)


@pytest.mark.parametrize("counts", [(5,), (255, 257), (1, 3, 4, 5, 7, 64, 193, 255)])
def test_device_adamw_list_up_to_eight_is_device_adamw(counts, ftn):
    a, _ = _run_list(ftn, ftn.fit.DeviceAdamWList, counts, 2, 0.5, 0.01)
    b, _ = _run_list(ftn, ftn.fit.DeviceAdamW, counts, 2, 0.5, 0.01)
    for k in a:
        for ga, gb in zip(a[k], b[k]):
            assert all(np.array_equal(x, y) for x, y in zip(ga, gb))


def test_device_adamw_list_limits(ftn):
    fit = ftn.fit
    assert issubclass(fit.DeviceAdamWList, fit.DeviceAdamW)
    fit.DeviceAdamWList([torch.zeros(2) for _ in range(32)])
    with pytest.raises(ValueError, match=r"DeviceAdamWList: 33 parameter tensors \(1..32\)"):
        fit.DeviceAdamWList([torch.zeros(2) for _ in range(33)])
    with pytest.raises(ValueError, match=r"DeviceAdamW: 9 parameter tensors \(1..8\)"):
        fit.DeviceAdamW([torch.zeros(2) for _ in range(9)])
