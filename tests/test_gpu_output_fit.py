"""The output refit on the MI355X.  ``ftn_timeproj_backward`` behind ``runtime.timeproj_backward``: a shape grid against
fp64 within the a-priori bound of any fp32 summation order, the form the query names, a NaN-poisoned workspace between
guards, run-to-run bits, untouched bytes around the outputs, exact integers, operands off the 16-byte grid.  End to
end on the tiny model of tests/test_gpu_fit.py: ``fit.output_nll`` against fp64 autograd of the torch composition
within the composed bound of tests/output_fit_oracle.py, ``fit.refit_output``'s invariants, and five Adam steps against
fp64-driven ones (tolerance: profiles/output_fit_error.json, written by tools/output_fit_error.py on the device).

Every accuracy case prints ``OUTFIT_ERR`` / ``OUTFIT_ADAM`` with its figures."""
import copy
import json
import re

import pytest
import torch

import output_fit_oracle as oracle
import ws_poison
from conftest import ROOT
from test_gpu_fit import _tiny_model

pytestmark = pytest.mark.gpu

C, U = oracle.C, oracle.U


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _off16(t):
    return torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)


def _operands(i, B, L, S, D, dev, integers=False):
    g = torch.Generator().manual_seed(300 + i)
    if integers:
        return (torch.randint(-3, 4, (B, L, D), generator=g).float().to(dev),
                torch.randint(-4, 5, (B, S, D), generator=g).float().to(dev))
    return torch.randn(B, L, D, generator=g).to(dev), torch.randn(B, S, D, generator=g).to(dev)


@pytest.mark.parametrize("i,B,L,S,D", [(i,) + c for i, c in enumerate(oracle.GRID)])
def test_timeproj_backward_shape_grid(i, B, L, S, D, ftn, dev):
    """dW_t and db_t against fp64 within ``(B D + 2) 2^-24 sum_{b,d} |dH[b,s,d] seq[b,l,d]|`` (the bias: without
    seq): the bound of B D products added in any order, plus the final rounding."""
    rt = ftn.runtime
    seq, dh = _operands(i, B, L, S, D, dev)
    assert (seq.data_ptr() | dh.data_ptr()) % 16 == 0
    assert rt.timeproj_backward_form_of(B, L, S, D, (seq.data_ptr() | dh.data_ptr()) & 15) == \
        ("k_timeproj_bwd_mfma", -(-B // C))
    dw, db = rt.timeproj_backward(seq, dh)
    assert dw.shape == (S, L) and db.shape == (S,) and dw.dtype == db.dtype == torch.float32
    s64, d64 = seq.double(), dh.double()
    want_w, mag_w = torch.einsum("bsd,bld->sl", d64, s64), torch.einsum("bsd,bld->sl", d64.abs(), s64.abs())
    want_b, mag_b = d64.sum((0, 2)), d64.abs().sum((0, 2))
    K = (B * D + 2) * U
    f_w = float(((dw.double() - want_w).abs() / (K * mag_w + 1e-300)).max())
    f_b = float(((db.double() - want_b).abs() / (K * mag_b + 1e-300)).max())
    print(f"OUTFIT_ERR grid {i} B={B} L={L} S={S} D={D}: fraction of the bound: dW_t {f_w:.4f} db_t {f_b:.4f}")
    assert f_w <= 1.0 and f_b <= 1.0
    # run to run, and from a NaN-poisoned workspace between guards
    again = rt.timeproj_backward(seq, dh)
    assert torch.equal(again[0], dw) and torch.equal(again[1], db)
    log = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(rt, "_workspace", ws_poison.poisoned_workspace(0xFF, log))
        # outputs that are views into a poisoned buffer
        buf_w = torch.full((S * L + 64,), float("nan"), device=dev)
        buf_b = torch.full((S + 64,), float("nan"), device=dev)
        snap_w, snap_b = buf_w.clone(), buf_b.clone()
        got = rt.timeproj_backward(seq, dh, dw=buf_w[32:32 + S * L].view(S, L), db=buf_b[32:32 + S])
        assert ws_poison.check_guards(log) == 1
    assert torch.equal(got[0], dw) and torch.equal(got[1], db)
    for buf, snap, n in ((buf_w, snap_w, S * L), (buf_b, snap_b, S)):
        assert torch.equal(buf[:32].view(torch.int32), snap[:32].view(torch.int32))
        assert torch.equal(buf[32 + n:].view(torch.int32), snap[32 + n:].view(torch.int32))


def test_every_form_ran(ftn):
    forms = {ftn.runtime.timeproj_backward_form_of(B, L, S, D)[0] for B, L, S, D in oracle.GRID}
    text = (ROOT / "flow-timesnet_amd" / "csrc" / "timeproj_bwd.hip").read_text()
    defined = set(re.findall(r"__global__[^\n]*\bvoid (k_\w+)\(", text)) - {"k_timeproj_bwd_reduce"}
    assert forms == defined == oracle.FORMS
    for k, axis in enumerate((oracle.BS, oracle.LS, oracle.SS, oracle.DS)):
        assert {c[k] for c in oracle.GRID} == set(axis)


@pytest.mark.parametrize("i,B,L,S,D", [(0, 3, 33, 17, 64), (1, 2 * C + 3, 28, 7, 96), (2, C + 1, 65, 33, 136),
                                       (3, C, 31, 1, 24), (4, 2 * C + 3, 1, 97, 4)])
def test_timeproj_backward_is_exact_on_small_integers(i, B, L, S, D, ftn, dev):
    """Integer seq in [-3, 3] and dH in [-4, 4]: every partial sum stays below B D 12 < 2^24 and is exact in fp32, so
    the result is the integer result, across the chunk boundary too."""
    assert B * D * 12 < 2 ** 24
    seq, dh = _operands(i, B, L, S, D, dev, integers=True)
    dw, db = ftn.runtime.timeproj_backward(seq, dh)
    assert torch.equal(dw.double(), torch.einsum("bsd,bld->sl", dh.double(), seq.double()))
    assert torch.equal(db.double(), dh.double().sum((0, 2)))


def test_operands_off_the_16_byte_grid_are_rejected_before_any_launch(ftn, dev):
    """There is no scalar-load form: a ValueError from the entry's own check, nothing is launched, and the next call
    on the grid gives the bits it gave before."""
    rt = ftn.runtime
    seq, dh = _operands(0, 3, 7, 2, 8, dev)
    base = rt.timeproj_backward(seq, dh)
    for a, b in ((_off16(seq), dh), (seq, _off16(dh))):
        assert (a.data_ptr() | b.data_ptr()) % 16 == 4
        with pytest.raises(ValueError, match="seq and d_hidden must be 16-byte aligned"):
            rt.timeproj_backward(a, b)
        with pytest.raises(ValueError, match="must be 16-byte aligned"):
            rt.timeproj_backward_form_of(3, 7, 2, 8, 4)
    again = rt.timeproj_backward(seq, dh)
    assert torch.equal(again[0], base[0]) and torch.equal(again[1], base[1])
    # the autograd function takes an off-grid seq on the torch path instead
    wt, bt = torch.randn(2, 7, device=dev).requires_grad_(), torch.randn(2, device=dev).requires_grad_()
    ftn.fit.time_projection(_off16(seq), wt, bt)
    assert ftn.fit._last_timeproj_backend == "torch"
    ftn.fit.time_projection(seq, wt, bt)
    assert ftn.fit._last_timeproj_backend == "hip"


def _six(model):
    steps = model._out_steps
    return [model.forecast_time_proj.weight[-steps:], model.forecast_time_proj.bias[-steps:], model.mu_head.weight,
            model.mu_head.bias, model.sigma_head.weight, model.sigma_head.bias]


@pytest.mark.parametrize("N", [1, 5])
def test_output_nll_end_to_end(N, ftn, dev):
    """The six gradients of ``fit.output_nll`` against fp64 autograd of the torch composition from the same ``seq``,
    within the composed bounds of ``output_fit_oracle.grads_and_bounds``; the fraction is printed."""
    fit, rt = ftn.fit, ftn.runtime
    model, batches = _tiny_model(ftn, N, dev)
    x, yb, mk = (t.to(dev) for t in batches[0])
    seq, tail, hist, late, floor = model.output_inputs(x)
    assert all(blk._last_backend == "hip" for blk in model.blocks)
    assert seq.shape == (4, 24, 16) and seq.is_contiguous() and not seq.requires_grad and hist == 4
    ps = [p.detach().clone().requires_grad_() for p in _six(model)]
    fit._last_timeproj_backend = fit._last_head_backend = None
    hidden = fit.time_projection(seq, ps[0], ps[1])
    assert fit._last_timeproj_backend == "hip" and hidden.requires_grad
    assert torch.equal(hidden.detach(), rt.timeproj_forward(seq, ps[0].detach(), ps[1].detach()))
    assert torch.equal(hidden.detach(), model.head_inputs(x)[0])
    loss, bad = fit.output_nll(seq, *ps, tail, hist, yb, mk > 0, late, floor, model.min_sigma)
    assert fit._last_timeproj_backend == "hip" and fit._last_head_backend == "hip" and int(bad) == 0
    got = torch.autograd.grad(loss, ps)
    loss64, want, bounds = oracle.grads_and_bounds(fit, seq, ps, tail, hist, yb, mk > 0, late, floor, model.min_sigma)
    assert abs(float(loss.detach()) - float(loss64)) <= 64 * (16 + 8 + 24 + 8) * U * abs(float(loss64))
    fracs = [oracle.fraction([a], [b], [c]) for a, b, c in zip(got, want, bounds)]
    print(f"OUTFIT_ERR output_nll N={N}: gradients against fp64 autograd, fraction of the composed bound: time "
          f"projection {max(fracs[:2]):.4f} heads {max(fracs[2:]):.4f}")
    assert max(fracs) <= 1.0


def test_refit_output_loop(ftn, dev):
    fit = ftn.fit
    model, batches = _tiny_model(ftn, 5, dev)
    twin = copy.deepcopy(model)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    flags = [p.requires_grad for p in model.parameters()]
    losses = fit.refit_output(model, batches, epochs=2, lr=1e-2, use_loss_mask=True)
    assert losses.shape == (6,) and losses.device.type == "cpu" and bool(torch.isfinite(losses).all())
    assert all(blk._last_backend == "hip" for blk in model.blocks)
    assert fit._last_head_backend == "hip" and fit._last_timeproj_backend == "hip"
    assert [p.requires_grad for p in model.parameters()] == flags and not model.training
    for k, v in model.state_dict().items():
        changed = not torch.equal(v, before[k])
        assert changed == k.startswith(("forecast_time_proj.", "mu_head.", "sigma_head.")), k
    assert float(losses[3:].mean()) < float(losses[:3].mean())     # the second pass over the batches starts lower
    first = fit.refit_heads(twin, batches[:1], lr=1e-2, use_loss_mask=True)
    assert float(first[0]) == float(losses[0])                     # the same forward: the same bits


@pytest.mark.parametrize("N", [1, 5])
def test_five_adam_steps_against_fp64_gradients(N, ftn, dev):
    """Five Adam steps of ``fit.refit_output`` against five steps of the same optimizer driven by the fp64 gradients
    (cast to fp32 for the step).  ``d0``: two fp64-driven runs that differ only in summation order (the batch rows
    reversed); it never involves the code under test.  The tolerance is the one measured on the MI355X and recorded in
    profiles/output_fit_error.json (``adam5``, by tools/output_fit_error.py), asserted at twice the recorded difference
    plus four times the recorded ``d0``; the figures are printed."""
    fit = ftn.fit
    model, batches = _tiny_model(ftn, N, dev)
    full = lambda m: [m.forecast_time_proj.weight, m.forecast_time_proj.bias, m.mu_head.weight, m.mu_head.bias,
                      m.sigma_head.weight, m.sigma_head.bias]
    steps = [batches[i % 3] for i in range(5)]
    runs = []
    for flip in (False, True):
        twin = copy.deepcopy(model)
        ps = full(twin)
        for p in ps:
            p.requires_grad_(True)
        opt = torch.optim.Adam(ps, lr=1e-2)
        for x, yb, mk in steps:
            seq, tail, hist, late, floor = twin.output_inputs(x.to(dev))
            yd, valid = yb.to(dev), mk.to(dev) > 0
            if flip:
                seq, tail, yd, valid = (t.flip(0) for t in (seq, tail, yd, valid))
                late = late if late is None or late.shape[0] == 1 else late.flip(0)
            grads = oracle.grads64(fit, seq, ps, tail, hist, yd, valid, late, floor, twin.min_sigma)
            opt.zero_grad(set_to_none=True)
            for p, g in zip(ps, grads):
                p.grad = g.float()
            opt.step()
        runs.append([p.detach().clone() for p in ps])
    fit.refit_output(model, steps, epochs=1, lr=1e-2, use_loss_mask=True)
    assert fit._last_head_backend == "hip" and fit._last_timeproj_backend == "hip"
    assert all(blk._last_backend == "hip" for blk in model.blocks)
    diff = max(float((a.detach() - b).abs().max()) for a, b in zip(full(model), runs[0]))
    d0 = max(float((a - b).abs().max()) for a, b in zip(runs[0], runs[1]))
    print(f"OUTFIT_ADAM N={N}: five Adam steps, largest parameter difference to the fp64-driven run {diff:.3e}, "
          f"between two fp64-driven runs {d0:.3e}")
    rec = json.loads((ROOT / "profiles" / "output_fit_error.json").read_text())["adam5"][f"N={N}"]
    assert diff <= 2 * rec["diff"] + 4 * rec["d0"]
