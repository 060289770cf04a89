"""The late-bias refit kernels on the MI355X (csrc/latefit.hip).  ``ftn_late_fit_forward`` behind
``runtime.late_fit_forward``: the bits of ``runtime.context_rows``' late output over the shape grid, a row list against
the unmapped call on ``rows[list]``, a NaN row and a bad-id row that leave every other row's bits.
``ftn_late_backward`` behind ``runtime.late_backward``: each of the five gradients against fp64 autograd of the torch
composition within the a-priori bound of tests/late_fit_oracle.py, run-to-run bits, a NaN-poisoned workspace between
guards, untouched bytes around every output, row lists with repeated and out-of-store indices, an integer lattice
across a chunk boundary, and the form the query names.  ``fit.late_bias`` as an autograd node.

Every accuracy case prints ``LATEFIT_ERR`` with its fraction of the bound."""
import re

import pytest
import torch

import late_fit_oracle as oracle
import ws_poison
from conftest import ROOT

pytestmark = pytest.mark.gpu

CHUNK = oracle.CHUNK


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _case(i, dev):
    rows, params, d_pre = oracle.case(i)
    return rows.to(dev), tuple(p.to(dev) for p in params), d_pre.to(dev)


@pytest.mark.parametrize("i", range(len(oracle.GRID)))
def test_forward_has_the_bits_of_context_rows(i, ftn, dev):
    """A table of ctx-wide embeddings through ``ftn_context_rows`` gives the rows and their late bias; the stored rows
    through ``ftn_late_fit_forward`` give that late bias again, bit for bit.  Then the row list."""
    rt = ftn.runtime
    ctx, S, R, layout = oracle.GRID[i]
    _, Bc, N = oracle.dims(R, layout)
    _, (gamma, beta, weight, bias, gate), _ = _case(i, dev)
    g = torch.Generator().manual_seed(500 + i)
    V = 37
    table = torch.randn(V, ctx, generator=g).to(dev)
    ids = torch.randint(0, V, (Bc, N), generator=g).to(dev)
    cn = (1.0 + 0.2 * torch.randn(ctx, generator=g)).to(dev), (0.2 * torch.randn(ctx, generator=g)).to(dev), 1e-5
    late_arg = ((gamma, beta, oracle.EPS), weight, bias, gate.reshape(-1))
    rows, _, _, late = rt.context_rows(Bc, N, cn, ids=ids, table=table, late=late_arg)
    got = rt.late_fit_forward(rows, gamma, beta, weight, bias, gate, oracle.EPS)
    assert got.shape == (Bc, S, N) and torch.equal(got.view(torch.int32), late.view(torch.int32))
    # the row list: repeated entries, the store read in place
    store = rows.reshape(Bc * N, ctx)
    index = torch.randint(0, Bc * N, (max(3, min(Bc * N, 70)),), generator=g).to(dev)
    mapped = rt.late_fit_forward(store, gamma, beta, weight, bias, gate, oracle.EPS, rows=index)
    plain = rt.late_fit_forward(store[index].unsqueeze(1).contiguous(), gamma, beta, weight, bias, gate, oracle.EPS)
    assert mapped.shape == (index.numel(), S, 1) and torch.equal(mapped.view(torch.int32), plain.view(torch.int32))


def test_a_nan_row_and_a_bad_id_row_leave_every_other_row(ftn, dev):
    rt = ftn.runtime
    i = 18                                                        # Bc = 3 blocks of N = 85 rows
    ctx, S, R, layout = oracle.GRID[i]
    rows, (gamma, beta, weight, bias, gate), _ = _case(i, dev)
    Bc, N = rows.shape[:2]
    base = rt.late_fit_forward(rows, gamma, beta, weight, bias, gate, oracle.EPS)
    hurt = rows.clone()
    r = (Bc * N) // 2
    hurt.reshape(Bc * N, ctx)[r, ctx // 2] = float("nan")
    got = rt.late_fit_forward(hurt, gamma, beta, weight, bias, gate, oracle.EPS)
    mask = torch.zeros(Bc, N, dtype=torch.bool, device=dev)
    mask.view(-1)[r] = True
    sel = mask.unsqueeze(1).expand(Bc, S, N)
    assert bool(torch.isnan(got[sel]).all())
    assert torch.equal(got[~sel].view(torch.int32), base[~sel].view(torch.int32))
    # a bad id: ftn_context_rows makes that row NaN, and so is its late bias here
    g = torch.Generator().manual_seed(1)
    table = torch.randn(11, ctx, generator=g).to(dev)
    ids = torch.randint(0, 11, (Bc, N), generator=g).to(dev)
    cn = torch.ones(ctx, device=dev), torch.zeros(ctx, device=dev), 1e-5
    good = rt.late_fit_forward(rt.context_rows(Bc, N, cn, ids=ids, table=table)[0], gamma, beta, weight, bias, gate,
                               oracle.EPS)
    ids.view(-1)[r] = 11
    bad_rows = rt.context_rows(Bc, N, cn, ids=ids, table=table)[0]
    assert bool(torch.isnan(bad_rows.reshape(Bc * N, ctx)[r]).all())
    got = rt.late_fit_forward(bad_rows, gamma, beta, weight, bias, gate, oracle.EPS)
    assert bool(torch.isnan(got[sel]).all())
    assert torch.equal(got[~sel].view(torch.int32), good[~sel].view(torch.int32))


@pytest.mark.parametrize("i", range(len(oracle.GRID)))
def test_backward_shape_grid(i, ftn, dev):
    """The five gradients against fp64 inside the oracle's bound; the form; run to run; a NaN-poisoned workspace
    between guards; bytes around every output."""
    rt = ftn.runtime
    ctx, S, R, layout = oracle.GRID[i]
    B, Bc, N = oracle.dims(R, layout)
    rows, params, d_pre = _case(i, dev)
    assert rt.late_backward_form_of(B, Bc, N, ctx, S) == ("k_late_bwd_mfma", -(-R // CHUNK))
    want, bounds = oracle.grads_and_bounds(*oracle.case(i))
    got = rt.late_backward(d_pre, rows, *params, oracle.EPS)
    assert [tuple(t.shape) for t in got] == [(ctx,), (ctx,), (S, ctx), (S,), (S,)]
    frac = oracle.fraction(got, want, bounds)
    print(f"LATEFIT_ERR grid {i} ctx={ctx} S={S} R={R} B={B} Bc={Bc}: fraction of the bound {frac:.4f}")
    assert frac <= 1.0
    again = rt.late_backward(d_pre, rows, *params, oracle.EPS)
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    log = []
    sizes = [ctx, ctx, S * ctx, S, S]
    bufs = [torch.full((n + 64,), float("nan"), device=dev) for n in sizes]
    snaps = [b.clone() for b in bufs]
    outs = [b[32:32 + n].view(t.shape) for b, n, t in zip(bufs, sizes, got)]
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(rt, "_workspace", ws_poison.poisoned_workspace(0xFF, log))
        poisoned = rt.late_backward(d_pre, rows, *params, oracle.EPS, out=outs)
        assert ws_poison.check_guards(log) == 1
    assert all(torch.equal(a, b) for a, b in zip(poisoned, got))
    for buf, snap, n in zip(bufs, snaps, sizes):
        assert torch.equal(buf[:32].view(torch.int32), snap[:32].view(torch.int32))
        assert torch.equal(buf[32 + n:].view(torch.int32), snap[32 + n:].view(torch.int32))


@pytest.mark.parametrize("i,B", [(3, 70), (8, CHUNK + 5), (12, 9)])
def test_backward_through_a_row_list(i, B, ftn, dev):
    """Repeated indices have the bits of the unmapped call on ``rows[list]``; an index outside the store is clamped
    into it."""
    rt = ftn.runtime
    ctx, S, R, _ = oracle.GRID[i]
    rows, params, _ = _case(i, dev)
    store = rows.reshape(R, ctx)
    g = torch.Generator().manual_seed(40 + i)
    index = torch.randint(0, R, (B,), generator=g).to(dev)
    index[B // 2] = index[0]
    d_pre = (torch.randn(B, S, 1, generator=g) / (B * S)).to(dev)
    mapped = rt.late_backward(d_pre, store, *params, oracle.EPS, rows=index)
    plain = rt.late_backward(d_pre, store[index].unsqueeze(1).contiguous(), *params, oracle.EPS)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(mapped, plain))
    wild = index.clone()
    wild[0], wild[-1] = -7, R + 1000
    clamped = index.clone()
    clamped[0], clamped[-1] = 0, R - 1
    a = rt.late_backward(d_pre, store, *params, oracle.EPS, rows=wild)
    b = rt.late_backward(d_pre, store, *params, oracle.EPS, rows=clamped)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    fa = rt.late_fit_forward(store, *params, oracle.EPS, rows=wild)
    fb = rt.late_fit_forward(store, *params, oracle.EPS, rows=clamped)
    assert torch.equal(fa.view(torch.int32), fb.view(torch.int32))


@pytest.mark.parametrize("R", [CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3])
def test_backward_is_exact_on_the_integer_lattice(R, ftn, dev):
    """gamma = 1, beta = 0, integer W, b, gate and d_pre, rows (+a, -a, 0, ...) with eps = 0: xh is (+-2, -+2, 0, ...)
    exactly and every partial sum an integer below 2^24, so the five results are the integers, across the chunk
    boundary."""
    rows, params, d_pre, want = oracle.lattice_case(R)
    assert R * 5 * 8 * 3 * 2 < 2 ** 24                            # |dz xh| <= S |du| |W| |xh| per row, the largest
    dgamma, dbeta, dw, db, dgate = ftn.runtime.late_backward(d_pre.to(dev), rows.to(dev), *(p.to(dev) for p in params),
                                                             0.0)
    for name, got in (("dgate", dgate), ("db", db), ("dW", dw), ("dbeta", dbeta), ("dgamma", dgamma)):
        assert torch.equal(got.cpu().double(), want[name].double()), name


def test_the_wide_layout_sums_the_batch_in_the_kernel(ftn, dev):
    """Bc == 1 and B > 1: the bits of the call on the batch sum formed ascending in one chain per (s, n)."""
    rt = ftn.runtime
    i = next(k for k, c in enumerate(oracle.GRID) if c[3] == ("wide", 5))
    rows, params, d_pre = _case(i, dev)
    summed = d_pre[0].clone()
    for b in range(1, d_pre.shape[0]):
        summed = summed + d_pre[b]
    a = rt.late_backward(d_pre, rows, *params, oracle.EPS)
    b = rt.late_backward(summed.unsqueeze(0).contiguous(), rows, *params, oracle.EPS)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def test_late_bias_is_an_autograd_node_over_the_kernels(ftn, dev):
    """``fit.late_bias`` on the device: the forward's bits, the five gradients those of ``runtime.late_backward`` on
    the incoming gradient, and its ``late=`` plugs into a loss."""
    fit = ftn.fit
    i = 4
    rows, params, d_pre = _case(i, dev)
    ps = [p.clone().requires_grad_() for p in params]
    late = fit.late_bias(rows, *ps, oracle.EPS)
    assert fit._last_late_backend == "hip"
    assert torch.equal(late.detach(), ftn.runtime.late_fit_forward(rows, *params, oracle.EPS))
    w = d_pre if d_pre.shape[0] == late.shape[0] else d_pre.sum(0, keepdim=True)
    (late * w).sum().backward()
    want = ftn.runtime.late_backward(w.contiguous(), rows, *params, oracle.EPS)
    for p, g in zip(ps, want):
        assert torch.equal(p.grad.reshape(-1), g.reshape(-1))
    assert ps[4].grad.shape == params[4].shape


def test_every_form_ran(ftn):
    forms = {ftn.runtime.late_backward_form_of(*oracle.dims(R, lay), ctx, S)[0] for ctx, S, R, lay in oracle.GRID}
    text = (ROOT / "flow-timesnet_amd" / "csrc" / "latefit.hip").read_text()
    defined = set(re.findall(r"__global__[^\n]*\bvoid (k_\w+)\(", text))
    assert defined == {"k_late_fit_forward", "k_late_bwd_rows", "k_late_bwd_mfma", "k_late_bwd_reduce"}
    assert forms == defined - {"k_late_fit_forward", "k_late_bwd_rows", "k_late_bwd_reduce"} == oracle.FORMS
    for k, axis in enumerate((oracle.CTXS, oracle.SS, oracle.RS, oracle.LAYOUTS)):
        assert {c[k] for c in oracle.GRID} == set(axis)
