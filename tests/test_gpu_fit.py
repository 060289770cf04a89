"""The head refit on the MI355X.  ``ftn_nb_nll_grad`` behind ``fit.nb_nll_grad`` and ``fit.negative_binomial_nll``:
every element of the lattice and of random fills against 40-digit arithmetic within the bound of tests/fit_oracle.py,
exact zeros where an element does not count, both kernel forms, a grid that walks its elements more than once,
bit-reproducibility (run to run, poisoned workspace, operands off the 16-byte grid, batch-strided operands), untouched
bytes around the outputs, and the autograd node.  ``ftn_head_fit_forward`` / ``ftn_head_backward``: a shape grid
against fp64 within the a-priori bound of an fp32 sum, exact integers, a poisoned workspace, both forms.  End to end:
``fit.head_nll`` against fp64 autograd, five Adam steps against fp64-driven ones, the loop's invariants.
``table.min_sigma`` on the device.

Every accuracy case prints ``FIT_ERR`` / ``FIT_ADAM`` with its figures (tools/head_fit_error.py records them)."""
import functools

import numpy as np
import pytest
import torch

import fit_oracle as fo
import ws_poison

pytestmark = pytest.mark.gpu

# (shape, seed): scalar and vector forms, one workgroup and several, N = 1, odd sizes
FILLS = [((1, 1, 1), 1), ((3, 7, 5), 2), ((4, 24, 37), 3), ((2, 24, 64), 4), ((5, 257, 1), 5), ((3, 2, 6), 6)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _draw(shape, seed):
    """log rate ~ U(-6, 6), y ~ Poisson(rate) with every seventh + 0.37, dispersion log-uniform in [1e-3, 100], a
    20 % mask."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = np.log(1e-3), np.log(100.0)
    disp = torch.exp(torch.rand(shape, generator=g) * (hi - lo) + lo)
    rate = torch.exp(torch.rand(shape, generator=g) * 12.0 - 6.0)
    y = torch.poisson(rate, generator=g)
    y.view(-1)[::7] += 0.37
    mask = torch.rand(shape, generator=g) >= 0.2
    return y, rate, disp, mask


@functools.lru_cache(maxsize=None)
def _truth(shape, seed):
    """The 40-digit closed forms of a fill, once for its three masks (the fills are finite everywhere)."""
    y, rate, disp, _ = _draw(shape, seed)
    return fo.closed_form(*fo.valid_of(y, rate, disp)[1:])


def _check(ftn, dev, y, rate, disp, mask, tag, truth=None):
    """hip against 40 digits: gradients within the bound times the scale, exact zeros elsewhere, the loss within its
    fp32 rounding plus the series' 1e-11 of the addends' magnitude."""
    loss, g_rate, g_disp = ftn.fit.nb_nll_grad(*(None if t is None else t.to(dev) for t in (y, rate, disp, mask)),
                                               backend="hip")
    assert ftn.fit._last_backend == "hip" and loss.dim() == 0 and g_rate.shape == y.shape
    valid, yv, mv, av = fo.valid_of(y, rate, disp, mask)
    t_rate, t_disp, ll, amp = truth if truth is not None else fo.closed_form(yv, mv, av)
    t_rate = np.where((rate < 1e-8).numpy(), 0.0, t_rate)       # the clamp is active: the value enters as eps
    t_disp = np.where((disp < 1e-8).numpy(), 0.0, t_disp)
    v = valid.numpy()
    n = max(int(v.sum()), 1)
    gr, gd = g_rate.cpu().double().numpy() * -n, g_disp.cpu().double().numpy() * -n
    assert ((gr == 0) & (gd == 0))[~v].all() and not np.isnan(gr).any() and not np.isnan(gd).any()
    f_rate = (np.abs(gr - t_rate) / fo.bound(t_rate))[v].max(initial=0.0)
    f_disp = (np.abs(gd - t_disp) / fo.bound(t_disp, amp))[v].max(initial=0.0)
    r = 1.0 / av.double()
    mag = (torch.lgamma(yv.double() + r).abs() + torch.lgamma(r).abs() + torch.lgamma(yv.double() + 1.0).abs()).numpy()
    want = -np.where(v, ll, 0.0).sum() / n
    f_loss = abs(float(loss) - want) / (2.0 ** -23 * abs(want) + 1e-11 * np.where(v, mag, 0.0).sum() / n + 1e-45)
    print(f"FIT_ERR {tag}: fraction of the bound: g_rate {f_rate:.3f} g_disp {f_disp:.3f} loss {f_loss:.3f}")
    assert f_rate <= 1.0 and f_disp <= 1.0 and f_loss <= 1.0, tag
    return loss, g_rate, g_disp


def test_lattice_against_the_differentiated_formula(ftn, dev):
    """Nothing of the lattice is left out; the truth is oracle 1 (the formula differentiated in 40 digits)."""
    y, rate, disp = fo.lattice()
    (d_rate, d_disp), _, (_, _, ll, amp) = fo.lattice_oracles()
    assert ftn.runtime.nb_nll_grad_form_of(6, 13, 8, (104,) * 3, 0)[0] == "k_nb_grad<4>"
    _check(ftn, dev, y, rate, disp, None, "lattice", truth=(d_rate, d_disp, ll, amp))
    # the same elements as [624, 1, 1] take the scalar form
    flat = [t.reshape(-1, 1, 1) for t in (y, rate, disp)]
    assert ftn.runtime.nb_nll_grad_form_of(624, 1, 1, (1,) * 3, 0) == ("k_nb_grad<1>", 3)
    _check(ftn, dev, *flat, None, "lattice as [624,1,1]",
           truth=tuple(t.reshape(-1, 1, 1) for t in (d_rate, d_disp, ll, amp)))


@pytest.mark.parametrize("shape,seed", FILLS)
@pytest.mark.parametrize("mask_kind", ["none", "bool", "float"])
def test_random_fills(shape, seed, mask_kind, ftn, dev):
    y, rate, disp, full = _draw(shape, seed)
    mask = {"none": None, "bool": full, "float": full.float() * 2.5}[mask_kind]
    _check(ftn, dev, y, rate, disp, mask, f"{shape} mask {mask_kind}", truth=_truth(shape, seed))


def test_both_forms_ran(ftn, dev):
    forms = set()
    for shape, seed in FILLS:
        y, rate, disp, _ = (t.to(dev) for t in _draw(shape, seed))
        forms.add(ftn.runtime.nb_nll_grad_form(y, rate, disp)[0])
    assert forms == {"k_nb_grad<1>", "k_nb_grad<4>"}


def test_elements_that_do_not_count_give_exact_zeros(ftn, dev):
    """NaN y, inf rate, inf and NaN dispersion, inside the mask and outside it; negative y counts as 0; a rate or
    dispersion below eps counts with a 0 derivative of its own."""
    y, rate, disp, mask = _draw((3, 7, 8), 11)
    mask[:] = True
    mask[0, 0, 0] = mask[1, 2, 3] = False
    y[0, 0, 0] = y[0, 0, 1] = float("nan")
    rate[1, 2, 3] = rate[1, 2, 4] = float("inf")
    disp[2, 0, 0], disp[2, 0, 1] = float("inf"), float("nan")
    y[2, 1, :4] = torch.tensor([-1.0, -0.5, -3.0, -float("inf")])
    rate[2, 2, 0], disp[2, 2, 1] = 1e-9, 0.0
    loss, g_rate, g_disp = _check(ftn, dev, y, rate, disp, mask, "special")
    assert bool(torch.isfinite(loss))
    assert g_rate[2, 2, 0] == 0 and g_disp[2, 2, 0] != 0 and g_disp[2, 2, 1] == 0 and g_rate[2, 2, 1] != 0
    zero = torch.zeros_like(y)
    for m in (zero.bool(), zero):
        loss, g_rate, g_disp = ftn.fit.nb_nll_grad(y.to(dev), rate.to(dev), disp.to(dev), m.to(dev))
        assert float(loss) == 0.0 and not bool(g_rate.any()) and not bool(g_disp.any())


def test_a_grid_that_walks_its_elements_more_than_once(ftn, dev):
    """[4, 301, 257] is 309428 elements (H N odd: the scalar form) for 1024 workgroups of 256: the derivatives are the bits of the same rows
    computed alone, the scale is -1 / count exactly and the loss is the fp64 mean of the per-element
    log-likelihoods ``score_columns`` writes."""
    rt = ftn.runtime
    y, rate, disp, mask = (t.to(dev) for t in _draw((4, 301, 257), 21))
    assert rt.nb_nll_grad_form(y, rate, disp, mask) == ("k_nb_grad<1>", 1024)
    words, g_rate, g_disp = rt.nb_nll_grad(y, rate, disp, mask, scaled=False)
    for b in range(4):
        _, r1, d1 = rt.nb_nll_grad(y[b:b + 1], rate[b:b + 1], disp[b:b + 1], mask[b:b + 1], scaled=False)
        assert torch.equal(r1[0], g_rate[b]) and torch.equal(d1[0], g_disp[b])
    _, ll = rt.score_columns(y, rate, disp, mask, want_ll=True)
    count = int(ftn.score.negative_binomial_mask(y, rate, disp, mask).sum())
    assert float(words[1]) == float(np.float32(-1.0 / count))
    want = -float(ll.double().sum()) / count
    assert abs(float(words[0]) - want) <= 2.0 ** -23 * abs(want)       # ll itself was rounded to fp32: 2^-24 each
    again, s_rate, s_disp = rt.nb_nll_grad(y, rate, disp, mask)
    assert torch.equal(again, words)
    assert torch.equal(s_rate, g_rate * words[1]) and torch.equal(s_disp, g_disp * words[1])


def test_poisoned_workspace_and_buffers(ftn, dev, monkeypatch):
    """The same bits from a NaN-poisoned workspace between guards, and outputs that are views into a poisoned
    buffer leave every byte around them alone."""
    rt = ftn.runtime
    for shape, seed in (((4, 24, 37), 3), ((2, 24, 64), 4)):
        y, rate, disp, mask = (t.to(dev) for t in _draw(shape, seed))
        base = rt.nb_nll_grad(y, rate, disp, mask)
        log = []
        monkeypatch.setattr(rt, "_workspace", ws_poison.poisoned_workspace(0xFF, log))
        n = y.numel()
        buf = torch.full((2, n + 64), float("nan"), device=dev)
        snapshot = buf.clone()
        outs = [buf[i, 32:32 + n].view(shape) for i in range(2)]
        got = rt.nb_nll_grad(y, rate, disp, mask, g_rate=outs[0], g_disp=outs[1])
        assert ws_poison.check_guards(log) == 1
        monkeypatch.undo()
        assert all(torch.equal(a, b) for a, b in zip(base, got))
        assert torch.equal(buf[:, :32].view(torch.int32), snapshot[:, :32].view(torch.int32))
        assert torch.equal(buf[:, 32 + n:].view(torch.int32), snapshot[:, 32 + n:].view(torch.int32))


def test_misaligned_and_strided_operands_give_the_same_bits(ftn, dev):
    """Operands one float off the 16-byte grid and a batch-strided rate take the scalar form; the bits are the vector
    form's."""
    rt = ftn.runtime
    shape = (2, 24, 64)
    y, rate, disp, mask = (t.to(dev) for t in _draw(shape, 4))
    base = rt.nb_nll_grad(y, rate, disp, mask)
    assert rt.nb_nll_grad_form(y, rate, disp, mask)[0] == "k_nb_grad<4>"
    n = y.numel()

    def off(t):
        return torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(shape)

    for which in range(3):
        ops = [y, rate, disp]
        ops[which] = off(ops[which])
        assert ops[which].data_ptr() % 16 == 4
        assert rt.nb_nll_grad_form(*ops, mask)[0] == "k_nb_grad<1>"
        assert all(torch.equal(a, b) for a, b in zip(base, rt.nb_nll_grad(*ops, mask)))
    wide = torch.zeros(2, 24 * 64 + 6, device=dev)
    wide[:, :24 * 64] = rate.view(2, -1)
    strided = wide.as_strided(shape, (24 * 64 + 6, 64, 1))
    assert strided.stride(0) % 4 == 2 and rt.nb_nll_grad_form(y, strided, disp, mask)[0] == "k_nb_grad<1>"
    assert all(torch.equal(a, b) for a, b in zip(base, rt.nb_nll_grad(y, strided, disp, mask)))
    wide4 = torch.zeros(2, 24 * 64 + 8, device=dev)
    wide4[:, :24 * 64] = rate.view(2, -1)
    strided4 = wide4.as_strided(shape, (24 * 64 + 8, 64, 1))
    assert rt.nb_nll_grad_form(y, strided4, disp, mask)[0] == "k_nb_grad<4>"
    assert all(torch.equal(a, b) for a, b in zip(base, rt.nb_nll_grad(y, strided4, disp, mask)))
    out_off = off(torch.empty(n, device=dev).view(shape))
    got = rt.nb_nll_grad(y, rate, disp, mask, g_disp=out_off)
    assert all(torch.equal(a, b) for a, b in zip(base, got))


def test_the_loss_is_an_autograd_node_on_the_device(ftn, dev):
    """``fit.negative_binomial_nll`` with operands that require grad runs the kernel (``score``'s function would go to
    torch) and ``backward`` delivers ``nb_nll_grad``'s gradients."""
    fit = ftn.fit
    y, rate, disp, mask = (t.to(dev) for t in _draw((4, 24, 37), 3))
    _, g_rate, g_disp = fit.nb_nll_grad(y, rate, disp, mask)
    rate, disp = rate.clone().requires_grad_(), disp.clone().requires_grad_()
    fit._last_backend = None
    loss = fit.negative_binomial_nll(y, rate, disp, mask)
    assert fit._last_backend == "hip" and loss.requires_grad
    (2.0 * loss).backward()
    assert torch.equal(rate.grad, 2.0 * g_rate) and torch.equal(disp.grad, 2.0 * g_disp)
    with pytest.raises(ValueError, match="nb_nll_grad: backend 'hip' takes fp32"):
        fit.nb_nll_grad(y.double(), rate.double(), disp.double(), backend="hip")
    t_loss, t_rate, t_disp = fit.nb_nll_grad(y, rate, disp, mask, backend="torch")
    assert fit._last_backend == "torch" and t_rate.device == y.device
    assert float((t_rate - g_rate).abs().max()) <= 4 * 2.0 ** -24 * float(g_rate.abs().max())


@pytest.mark.parametrize("name", ["dense", "masked", "even", "all_masked", "empty", "one_series"])
def test_min_sigma_on_the_device(name, ftn, dev):
    """``table.min_sigma`` from ``ftn_table_moments``' centred sums against the reference's recorded ``_masked_std``.
    The kernel squares differences ``fp32(v - mean)``: each is within 2^-24 relative, so each square within 2^-23,
    their fp64 sum within 2^-23 and its root within 2^-24; the reference subtracts ``mean^2`` from the mean square in
    fp64 and carries ``2^-52 mean^2 / variance`` itself, below 1e-9 on these tables (mean up to 900, std from 0.5).
    Together: rtol 2^-24 + 1e-9."""
    from test_fit_forms_table import load_case

    RTOL_STD = 2.0 ** -24 + 1e-9
    tb = ftn.table
    values, mask, want_global, want_median, want_per = load_case(name)
    v = torch.from_numpy(values).to(dev)
    m = None if mask is None else torch.from_numpy(mask).to(dev)
    std, per = tb.min_sigma(v, m)
    assert tb._last_backend == "hip" and std.is_cuda and per.is_cuda and std.dtype == per.dtype == torch.float64
    np.testing.assert_allclose(float(std), want_global, rtol=RTOL_STD, atol=0.0)
    med, per2 = tb.min_sigma(v, m, method="per_series_median")
    np.testing.assert_allclose(float(med), want_median, rtol=RTOL_STD, atol=0.0)
    np.testing.assert_allclose(per2.cpu().numpy(), want_per, rtol=RTOL_STD, atol=0.0)
    assert torch.equal(per, per2)


def _tiny_model(ftn, N, dev, seed=1):
    L, H = 24, 4
    cfg = dict(input_len=L, pred_len=H, d_model=16, d_ff=32, n_layers=2, k_periods=3, kernel_set=[(3, 3), (5, 5)],
               dropout=0.0, activation="gelu", mode="direct", use_checkpoint=False)
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
    return model.to(dev), batches


C = 256                                                         # rows of a chunk (HF_CHUNK)
RS = [1, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3]
NS = [1, 2, 4, 5, 16, 17, 32, 33, 130]
DS = [8, 24, 64, 96, 128, 136, 512]
# every R, N and D appears, rotated against each other; 0: hidden on the 16-byte grid, 4: one float off it
GRID = [(RS[i % 8], NS[i % 9], DS[i % 7], 4 if i % 5 == 4 else 0) for i in range(0, 63, 1)][:36]


def _head_case(i, R, N, D, dev, integers=False):
    """Operands of case i: B S = R with S in {1, R} or a divisor, hist < S and hist = S, late absent / [1,S,N] /
    [B,S,N], floor scalar / vector and a batch-strided tail in rotation; one pre-activation above 20."""
    g = torch.Generator().manual_seed(100 + i)
    S = next(s for s in (7, 5, 3, 1) if R % s == 0)
    B = R // S
    hist = S if i % 2 else max(1, S - 2)
    if integers:
        hidden = torch.randint(-3, 4, (B, S, D), generator=g).float()
    else:
        hidden = torch.randn(B, S, D, generator=g)
    ws = [0.2 * torch.randn(N, D, generator=g), 0.1 * torch.randn(N, generator=g),
          0.2 * torch.randn(N, D, generator=g), 0.1 * torch.randn(N, generator=g)]
    wide = torch.rand(B, hist * N + 3, generator=g) + 0.5
    late = [None, 0.1 * torch.randn(1, S, N, generator=g), 0.1 * torch.randn(B, S, N, generator=g)][i % 3]
    floor = None if i % 2 else torch.rand(N, generator=g) * 0.1 + 1e-3
    if not integers:
        wide[0, 0] = 60.0                                       # pre-activation above 20: sigma' = 1
    to = lambda t: None if t is None else t.to(dev)
    widedev = to(wide)
    tail = widedev.as_strided((B, hist, N), (hist * N + 3, N, 1)) if i % 4 < 2 else widedev[:, :hist * N].reshape(B, hist, N).contiguous()
    return to(hidden), [to(w) for w in ws], tail, hist, to(late), to(floor), B, S


def _off16(t):
    return torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)


@pytest.mark.parametrize("i,R,N,D,mis", [(i,) + c for i, c in enumerate(GRID)])
def test_head_backward_shape_grid(i, R, N, D, mis, ftn, dev):
    """dW, db and d_hidden against fp64 within the a-priori bound of any fp32 summation order,
    ``(R + 2) 2^-24 sum_r |G[r, n] hidden[r, d]|`` (d_hidden: N + N + 2 terms), with G the kernel's own operands
    promoted to fp64; the forward's rate, dispersion and sigmoids against the fp64 composition; the form the query
    names; the same bits from a NaN-poisoned workspace, whose guards stay."""
    rt = ftn.runtime
    hidden, ws, tail, hist, late, floor, B, S = _head_case(i, R, N, D, dev)
    rate, disp, sig_mu, sig_sg, bad = rt.head_fit_forward(hidden, *ws, tail, hist, late, floor, 1e-3)
    h64, (wm, bm, wsg, bs) = hidden.double(), [w.double() for w in ws]
    last = tail.double()
    if hist < S:
        last = torch.cat([last, last[:, -1:].expand(-1, S - hist, -1)], 1)
    pre = h64 @ wm.T + bm + last + (0 if late is None else late.double())
    sp = h64 @ wsg.T + bs
    soft = lambda t: torch.where(t > 20, t, torch.log1p(torch.exp(torch.clamp(t, max=20.0))))
    fl = 1e-3 if floor is None else floor.double()
    mag = (h64.abs() @ wm.abs().T + bm.abs() + last.abs() + 1.0)
    tol = (D + 8) * 2.0 ** -24 * mag                            # D + 3 roundings of the sum, softplus' few ulps
    assert bool(((rate.double() - (soft(pre) + 1e-6)).abs() <= tol).all()) and int(bad) == 0
    assert bool(((disp.double() - (soft(sp) + fl + 1e-6)).abs() <= (D + 8) * 2.0 ** -24 * (h64.abs() @ wsg.abs().T + bs.abs() + 1.0)).all())
    want_sig = torch.where(pre > 20, torch.ones_like(pre), torch.sigmoid(pre))
    assert bool(((sig_mu.double() - want_sig).abs() <= 0.25 * tol + 4 * 2.0 ** -24).all())    # sigma'' <= 1/4
    assert float(sig_mu[0, 0, 0]) == 1.0 and float(pre[0, 0, 0]) > 20

    g = torch.Generator().manual_seed(7 + i)
    g_rate, g_disp = (torch.randn(B, S, N, generator=g).to(dev) for _ in range(2))
    scale = torch.tensor([-1.0 / 37.0], device=dev)
    hid = _off16(hidden) if mis else hidden
    assert hid.data_ptr() % 16 == mis
    form = rt.head_backward_form_of(R, N, D, mis)
    assert form == ((f"k_headfit_colsum<{N}>" if N <= 4 and not mis else "k_headfit_mfma"), -(-R // C))
    base = rt.head_backward(hid, g_rate, g_disp, sig_mu, sig_sg, scale, ws[0], ws[2], want_hidden=True)
    Gm = (g_rate * sig_mu * scale).double().reshape(R, N)       # the kernel's G: three fp32 values, two roundings
    Gs = (g_disp * sig_sg * scale).double().reshape(R, N)
    H = h64.reshape(R, D)
    u = 2.0 ** -24
    for got, G in ((base[0], Gm), (base[2], Gs)):
        assert bool(((got.double() - G.T @ H).abs() <= (R + 2) * u * (G.abs().T @ H.abs())).all())
    for got, G in ((base[1], Gm), (base[3], Gs)):
        assert bool(((got.double() - G.sum(0)).abs() <= (R + 2) * u * G.abs().sum(0)).all())
    dh = Gm @ wm + Gs @ wsg
    assert bool(((base[4].double().reshape(R, D) - dh).abs() <= (2 * N + 2) * u * (Gm.abs() @ wm.abs() + Gs.abs() @ wsg.abs())).all())
    log = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(rt, "_workspace", ws_poison.poisoned_workspace(0xFF, log))
        again = rt.head_backward(hid, g_rate, g_disp, sig_mu, sig_sg, scale, ws[0], ws[2], want_hidden=True)
        assert ws_poison.check_guards(log) == 1
    assert all(torch.equal(a, b) for a, b in zip(base, again))


def test_head_backward_both_forms_ran(ftn):
    forms = {ftn.runtime.head_backward_form_of(R, N, D, mis)[0].split("<")[0] for R, N, D, mis in GRID}
    assert forms == {"k_headfit_colsum", "k_headfit_mfma"}
    assert {c[0] for c in GRID} == set(RS) and {c[1] for c in GRID} == set(NS) and {c[2] for c in GRID} == set(DS)


@pytest.mark.parametrize("i,R,N,D", [(0, 2 * C + 3, 2, 24), (1, C + 1, 4, 136), (2, 2 * C + 3, 5, 96), (3, 65, 33, 8),
                                     (4, C - 1, 130, 64)])
def test_head_backward_is_exact_on_small_integers(i, R, N, D, ftn, dev):
    """Integer G (sigma' = 1, scale = 1) and integer hidden keep every partial sum exact in fp32: the result is the
    integer result, in both forms."""
    rt = ftn.runtime
    g = torch.Generator().manual_seed(50 + i)
    hidden = torch.randint(-3, 4, (R, D), generator=g).float().to(dev)
    g_rate, g_disp = (torch.randint(-4, 5, (R, N), generator=g).float().to(dev) for _ in range(2))
    ones, scale = torch.ones(R, N, device=dev), torch.ones(1, device=dev)
    wm, wsg = (torch.randint(-2, 3, (N, D), generator=g).float().to(dev) for _ in range(2))
    out = rt.head_backward(hidden, g_rate, g_disp, ones, ones, scale, wm, wsg, want_hidden=True)
    H, Gm, Gs = hidden.double(), g_rate.double(), g_disp.double()
    want = (Gm.T @ H, Gm.sum(0), Gs.T @ H, Gs.sum(0), Gm @ wm.double() + Gs @ wsg.double())
    assert all(torch.equal(a.double(), b) for a, b in zip(out, want))


@pytest.mark.parametrize("N", [1, 5])
def test_refit_heads_end_to_end(N, ftn, dev):
    """A tiny model (d_model 16, 2 blocks, L 24, H 4).  ``head_nll``'s gradients against fp64 autograd of the torch
    composition: the summation bound ``(R + 2) 2^-24 sum |G hidden|`` plus what the forward's fp32 pre-activations
    (D + 8 roundings) move G by - G's logarithmic derivative in a pre-activation is below 1 + y <= 64 on these
    inputs - so ``(R + 2 + 64 (D + 8)) 2^-24 sum_r |G[r, n] hidden[r, d]|``; the fraction of it is printed.  Then the
    loop: the backbone runs on the HIP path and keeps its bits, only the heads move, flags and mode come back."""
    fit = ftn.fit
    model, batches = _tiny_model(ftn, N, dev)
    heads = lambda m: [m.mu_head.weight, m.mu_head.bias, m.sigma_head.weight, m.sigma_head.bias]
    before = {k: v.clone() for k, v in model.state_dict().items()}
    flags = [p.requires_grad for p in model.parameters()]
    x, yb, mk = (t.to(dev) for t in batches[0])
    hidden, tail, hist, late, floor = model.head_inputs(x)
    assert all(blk._last_backend == "hip" for blk in model.blocks) and model._last_timeproj_backend == "hip"
    assert hidden.shape == (4, 4, 16) and not hidden.requires_grad and hist == 4 and tail.shape == (4, 4, N)
    ps = [p.detach().clone().requires_grad_() for p in heads(model)]
    hid = hidden.clone().requires_grad_()
    loss, bad = fit.head_nll(hid, *ps, tail, hist, yb, mk > 0, late, floor, model.min_sigma)
    assert fit._last_head_backend == "hip" and int(bad) == 0
    got = torch.autograd.grad(loss, ps + [hid])
    p64 = [p.detach().double().requires_grad_() for p in ps]
    h64 = hidden.double().requires_grad_()
    rate, disp, _ = fit._heads_torch(h64, *p64, tail.double(), hist, None if late is None else late.double(),
                                     None if floor is None else floor.double(), model.min_sigma)
    valid = mk > 0
    al, mu, yy = disp, rate, yb.double()
    l1 = torch.log1p(al * mu)
    ll = (torch.lgamma(yy + 1 / al) - torch.lgamma(1 / al) - torch.lgamma(yy + 1) - l1 / al
          + yy * (torch.log(al) + torch.log(mu) - l1))
    loss64 = -(ll * valid).sum() / valid.sum()
    Gm, Gs = torch.autograd.grad(loss64, [rate, disp], retain_graph=True)
    want = torch.autograd.grad(loss64, p64 + [h64])
    R, D, u = 16, 16, 2.0 ** -24
    assert abs(float(loss.detach()) - float(loss64.detach())) <= 64 * (D + 8) * u * abs(float(loss64.detach()))
    # G with respect to the pre-activations, for the bound's magnitude
    Gm_pre = (Gm * (1 - torch.exp(-(rate - 1e-6)))).reshape(R, N).abs()
    Gs_pre = (Gs * (1 - torch.exp(-(disp - 1e-6 - (model.min_sigma if floor is None else floor.double()))))).reshape(R, N).abs()
    Habs = hidden.double().reshape(R, D).abs()
    K = (R + 2 + 64 * (D + 8)) * u
    bounds = [K * Gm_pre.T @ Habs, K * Gm_pre.sum(0), K * Gs_pre.T @ Habs, K * Gs_pre.sum(0),
              (K * (Gm_pre @ p64[0].detach().abs() + Gs_pre @ p64[2].detach().abs())).reshape(4, 4, D)]
    frac = max(float(((a.double() - b).abs() / (bd + 1e-300)).max()) for a, b, bd in zip(got, want, bounds))
    print(f"FIT_ERR head_nll N={N}: gradients against fp64 autograd, largest fraction of the composed bound {frac:.4f}")
    assert frac <= 1.0

    losses = fit.refit_heads(model, batches, epochs=2, lr=1e-2, use_loss_mask=True)
    assert losses.shape == (6,) and losses.device.type == "cpu" and bool(torch.isfinite(losses).all())
    assert all(blk._last_backend == "hip" for blk in model.blocks) and fit._last_head_backend == "hip"
    assert [p.requires_grad for p in model.parameters()] == flags and not model.training
    for k, v in model.state_dict().items():
        changed = not torch.equal(v, before[k])
        assert changed == (k.startswith("mu_head.") or k.startswith("sigma_head.")), k
    assert float(losses[3:].mean()) < float(losses[:3].mean())     # the second pass over the batches starts lower


def _loss64(fit, hidden, ps, tail, hist, yb, valid, late, floor, min_sigma):
    """The torch composition and the restated formula in fp64 (dispersion >= 1e-3 + softplus here: well away from
    the band where fp64 autograd of the formula is not an oracle)."""
    rate, disp, _ = fit._heads_torch(hidden.double(), *ps, tail.double(), hist, None if late is None else late.double(),
                                     None if floor is None else floor.double(), min_sigma)
    yy = yb.double()
    l1 = torch.log1p(disp * rate)
    ll = (torch.lgamma(yy + 1 / disp) - torch.lgamma(1 / disp) - torch.lgamma(yy + 1) - l1 / disp
          + yy * (torch.log(disp) + torch.log(rate) - l1))
    return -(ll * valid).sum() / valid.sum()


@pytest.mark.parametrize("N", [1, 5])
def test_five_adam_steps_against_fp64_gradients(N, ftn, dev):
    """Five Adam steps of ``fit.refit_heads`` against five steps of the same optimizer driven by the fp64 gradients
    (cast to fp32 for the step).  ``d0``: two fp64-driven runs that differ only in summation order (the batch rows
    reversed).  The tolerance is the one measured on the MI355X and recorded in profiles/head_fit_error.json
    (``adam5``, by tools/head_fit_error.py), asserted at twice the recorded difference plus four times the
    recorded ``d0``; the figures are printed."""
    import copy
    import json
    from conftest import ROOT

    fit = ftn.fit
    model, batches = _tiny_model(ftn, N, dev)
    heads = lambda m: [m.mu_head.weight, m.mu_head.bias, m.sigma_head.weight, m.sigma_head.bias]
    steps = [batches[i % 3] for i in range(5)]
    runs = []
    for flip in (False, True):
        twin = copy.deepcopy(model)
        ps = heads(twin)
        for p in ps:
            p.requires_grad_(True)
        opt = torch.optim.Adam(ps, lr=1e-2)
        for x, yb, mk in steps:
            hidden, tail, hist, late, floor = twin.head_inputs(x.to(dev))
            yd, valid = yb.to(dev), mk.to(dev) > 0
            if flip:
                hidden, tail, yd, valid = (t.flip(0) for t in (hidden, tail, yd, valid))
                late = late if late is None or late.shape[0] == 1 else late.flip(0)
            p64 = [p.detach().double().requires_grad_() for p in ps]
            grads = torch.autograd.grad(_loss64(fit, hidden, p64, tail, hist, yd, valid, late, floor, twin.min_sigma), p64)
            opt.zero_grad(set_to_none=True)
            for p, g in zip(ps, grads):
                p.grad = g.float()
            opt.step()
        runs.append([p.detach().clone() for p in ps])
    fit.refit_heads(model, steps, epochs=1, lr=1e-2, use_loss_mask=True)
    assert fit._last_head_backend == "hip" and all(blk._last_backend == "hip" for blk in model.blocks)
    diff = max(float((a - b).abs().max()) for a, b in zip(heads(model), runs[0]))
    d0 = max(float((a - b).abs().max()) for a, b in zip(runs[0], runs[1]))
    print(f"FIT_ADAM N={N}: five Adam steps, largest parameter difference to the fp64-driven run {diff:.3e}, "
          f"between two fp64-driven runs {d0:.3e}")
    rec = json.loads((ROOT / "profiles" / "head_fit_error.json").read_text())["adam5"][f"N={N}"]
    assert diff <= 2 * rec["diff"] + 4 * rec["d0"]
