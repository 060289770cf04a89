"""The head refit's likelihood gradient on the host side (no GPU): the exports, the two oracles against each other on
the lattice, the torch backend of ``fit.nb_nll_grad`` against them, the fixture of what the reference's own fp32
autograd returned (tests/golden/nb_grad_cases.npz, written by make_golden_nb_grad.py), the autograd function, the
form rule of ``ftn_nb_nll_grad`` and every argument error before a launch."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN
import fit_oracle as fo


def _cases():
    with np.load(GOLDEN / "nb_grad_cases.npz") as z:
        return {k: z[k] for k in z.files}


CASES = ("floor_none", "mid_float", "high_bool", "floor_allfalse", "special")


def _case(z, name):
    y, rate, disp = (torch.from_numpy(z[f"{name}:{k}"]) for k in ("y", "rate", "disp"))
    mask = torch.from_numpy(z[f"{name}:mask"]) if f"{name}:mask" in z else None
    return y, rate, disp, mask


def test_abi_version_and_exports(ftn):
    assert {"ftn_nb_nll_grad", "ftn_nb_nll_grad_form", "ftn_nb_nll_grad_workspace"} <= set(ftn.lib.EXPORTS)
    lib = ftn.lib.load()
    assert lib.ftn_abi_version() == 14 and ftn.lib.ABI_VERSION == 14
    for name in ("nb_nll_grad", "negative_binomial_nll"):
        assert callable(getattr(ftn.fit, name)), name
    assert callable(ftn.runtime.nb_nll_grad)


def test_the_two_oracles_agree_within_a_sixteenth_of_the_bound():
    """Differentiating the formula and the closed form with the finite sum are independent; where both exist (the
    integer y) they agree within 1/16 of the bound on every element, so the bound is held against the truth and not
    against an oracle's own error.  The 40-digit closed form with two digammas covers the non-integer y the same
    way."""
    (d_rate, d_disp), (s_rate, s_disp, _, s_amp), (c_rate, c_disp, _, c_amp) = fo.lattice_oracles()
    y = fo.lattice()[0].numpy()
    whole = y == np.floor(y)
    assert whole.sum() == 6 * 13 * 6 and not np.isnan(s_disp[whole]).any() and np.isnan(s_disp[~whole]).all()
    assert (np.abs(d_disp - s_disp)[whole] <= fo.bound(d_disp, s_amp)[whole] / 16).all()
    assert (np.abs(d_rate - s_rate) <= fo.bound(d_rate) / 16).all()
    assert (np.abs(d_disp - c_disp) <= fo.bound(d_disp, c_amp) / 16).all()
    assert (np.abs(d_rate - c_rate) <= fo.bound(d_rate) / 16).all()


def test_torch_backend_on_the_lattice(ftn):
    """Every element of the lattice, against the differentiated formula, within the bound (times the scale 1 / n the
    gradients carry)."""
    y, rate, disp = fo.lattice()
    (d_rate, d_disp), _, (_, _, _, amp) = fo.lattice_oracles()
    loss, g_rate, g_disp = ftn.fit.nb_nll_grad(y, rate, disp, backend="torch")
    assert ftn.fit._last_backend == "torch" and loss.dim() == 0 and g_rate.dtype == g_disp.dtype == torch.float32
    n = y.numel()
    assert (np.abs(g_rate.double().numpy() * -n - d_rate) <= fo.bound(d_rate)).all()
    assert (np.abs(g_disp.double().numpy() * -n - d_disp) <= fo.bound(d_disp, amp)).all()


def test_dpsi_is_not_two_digammas_subtracted(ftn):
    """``_dpsi`` to 1e-11 relative where ``r`` is 1e8 times ``y`` (two fp64 digammas subtracted keep 1e-7 there) and
    where the upward shift does the work."""
    import mpmath as mp

    ys = [0.0, 1e-3, 0.37, 1.0, 7.0, 12.5, 400.0, 1e5]
    rs = [0.0333, 0.9, 7.5, 8.0, 33.0, 1e3, 1e8]
    Y, R = torch.meshgrid(torch.tensor(ys, dtype=torch.float64), torch.tensor(rs, dtype=torch.float64), indexing="ij")
    got = ftn.fit._dpsi(Y, R).numpy()
    with mp.workdps(40):
        want = np.array([[float(mp.digamma(mp.mpf(y) + mp.mpf(r)) - mp.digamma(mp.mpf(r))) for r in rs] for y in ys])
    assert (got[0] == 0).all()
    assert (np.abs(got - want) <= 1e-11 * want).all()


@pytest.mark.parametrize("name", CASES)
def test_golden_cases_against_the_reference(name, ftn):
    """The loss is the reference's (rtol 1e-6, the tolerance of test_score_host.py) wherever the reference's is
    finite; with a NaN or inf element planted the reference's loss is NaN (ll * 0) and ours is the fp64 mean over
    the valid elements.  The gradients' sup-norm error against 40 digits is no larger than that of the gradients the
    reference's fp32 autograd recorded - which is far from zero near the dispersion floor."""
    z = _cases()
    y, rate, disp, mask = _case(z, name)
    loss, g_rate, g_disp = ftn.fit.nb_nll_grad(y, rate, disp, mask, backend="torch")
    valid, yv, mv, av = fo.valid_of(y, rate, disp, mask)
    t_rate, t_disp, ll, _ = fo.closed_form(yv, mv, av)
    v = valid.numpy()
    scale = -1.0 / max(int(v.sum()), 1)
    t_rate, t_disp = np.where(v, t_rate, 0.0) * scale, np.where(v, t_disp, 0.0) * scale
    ref_loss = float(z[f"{name}:loss"])
    if np.isfinite(ref_loss):
        np.testing.assert_allclose(float(loss), ref_loss, rtol=1e-6, atol=0.0)
    else:
        assert name == "special"
    # against 40 digits: fp32 lgamma(y + r) - lgamma(r) cancels ~r log r against itself, a few 2^-24 of that each
    assert abs(float(loss) - np.where(v, ll, 0.0).sum() * scale) <= 2.0 ** -22 * (1e3 * np.log(1e3) + abs(float(loss)))
    assert ((g_rate.numpy() == 0) & (g_disp.numpy() == 0))[~v].all()
    for got, ref, want in ((g_rate, z[f"{name}:g_rate"], t_rate), (g_disp, z[f"{name}:g_disp"], t_disp)):
        ours = np.abs(got.double().numpy() - want).max()
        theirs = np.nan_to_num(np.abs(ref.astype(np.float64) - want), nan=np.inf).max()
        print(f"{name}: sup-norm error ours {ours:.3e} reference {theirs:.3e}")
        assert ours <= theirs
    if name == "floor_none":
        rel = np.abs(z[f"{name}:g_disp"] - t_disp) / np.abs(t_disp)
        assert np.median(rel) > 1e-2                       # the condition above discriminates


def test_all_false_mask_gives_zero_loss_and_gradients(ftn):
    y, rate, disp, mask = _case(_cases(), "floor_allfalse")
    loss, g_rate, g_disp = ftn.fit.nb_nll_grad(y, rate, disp, mask, backend="torch")
    assert float(loss) == 0.0 and not g_rate.any() and not g_disp.any()


def test_clamped_operands_get_zero_derivatives(ftn):
    """Below ``eps`` the clamp is active: the value enters the likelihood as ``eps`` and its derivative is 0."""
    y = torch.tensor([[[3.0, 3.0, 3.0]]])
    rate = torch.tensor([[[1e-9, 2.0, 2.0]]])
    disp = torch.tensor([[[0.5, 1e-9, 0.5]]])
    loss, g_rate, g_disp = ftn.fit.nb_nll_grad(y, rate, disp, backend="torch")
    assert g_rate[0, 0, 0] == 0 and g_disp[0, 0, 0] != 0 and g_disp[0, 0, 1] == 0 and g_rate[0, 0, 1] != 0
    assert bool(torch.isfinite(loss))


def test_masks_broadcast_as_the_references(ftn):
    y, rate, disp, mask = _case(_cases(), "high_bool")
    rows = mask[:, :, 0]
    a = ftn.fit.nb_nll_grad(y, rate, disp, rows, backend="torch")
    b = ftn.fit.nb_nll_grad(y, rate, disp, rows[:, :, None].expand_as(y), backend="torch")
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_the_loss_is_an_autograd_node(ftn):
    """``backward`` delivers ``nb_nll_grad``'s gradients times the incoming one, to rate and dispersion alone, in
    their dtypes."""
    y, rate, disp, mask = _case(_cases(), "mid_float")
    _, g_rate, g_disp = ftn.fit.nb_nll_grad(y, rate, disp, mask)
    rate, disp = rate.clone().requires_grad_(), disp.double().requires_grad_()
    yg = y.clone().requires_grad_()
    loss = ftn.fit.negative_binomial_nll(yg, rate, disp, mask)
    assert loss.requires_grad and loss.dim() == 0
    (3.0 * loss).backward()
    assert yg.grad is None and rate.grad.dtype == torch.float32 and disp.grad.dtype == torch.float64
    assert torch.equal(rate.grad, 3.0 * g_rate) and torch.equal(disp.grad, (3.0 * g_disp).double())


def test_argument_errors(ftn):
    fit = ftn.fit
    y, rate, disp = torch.zeros(2, 4, 4), torch.ones(2, 4, 4), torch.ones(2, 4, 4)
    with pytest.raises(ValueError, match="rate has shape"):
        fit.nb_nll_grad(y, rate[:, :3], disp)
    with pytest.raises(TypeError, match="dispersion must be a tensor"):
        fit.nb_nll_grad(y, rate, 1.0)
    with pytest.raises(ValueError, match="eps=0"):
        fit.nb_nll_grad(y, rate, disp, eps=0.0)
    with pytest.raises(ValueError, match="does not broadcast"):
        fit.nb_nll_grad(y, rate, disp, mask=torch.ones(3, 4))
    with pytest.raises(ValueError, match="backend 'cuda' is not"):
        fit.nb_nll_grad(y, rate, disp, backend="cuda")
    with pytest.raises(ValueError, match="nb_nll_grad: backend 'hip' takes fp32 \\[B, H, N\\] tensors"):
        fit.nb_nll_grad(y, rate, disp, backend="hip")
    with pytest.raises(ValueError, match="backend 'hip' takes"):
        fit.negative_binomial_nll(y, rate.requires_grad_(), disp, backend="hip")


def test_wrapper_validates_layout_on_the_host(ftn):
    rt = ftn.runtime
    y, r, d = torch.zeros(2, 8, 8), torch.ones(2, 8, 8), torch.ones(2, 8, 8)
    with pytest.raises(ValueError, match="nb_nll_grad: y must be an fp32 device tensor"):
        rt.nb_nll_grad(y, r, d)
    with pytest.raises(ValueError, match="\\[B, H, N\\]"):
        rt.nb_nll_grad(y[0], r, d)
    with pytest.raises(ValueError, match="dispersion needs contiguous rows"):
        rt.nb_nll_grad(y, r, torch.ones(2, 16, 8)[:, ::2])


def test_refit_heads_on_the_host(ftn):
    """The loop on CPU tensors (torch paths throughout): only the heads move, flags and mode come back, the losses
    are finite, and a head that produces a non-finite rate raises the reference's error at the end."""
    fit = ftn.fit
    L, H, N = 24, 4, 3
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(0)
    model = ftn.models.TimesNet(input_len=L, pred_len=H, d_model=16, d_ff=32, n_layers=1, k_periods=2,
                                kernel_set=[(3, 3)], dropout=0.0, activation="gelu", mode="direct",
                                use_checkpoint=False).train()
    batches = [(torch.rand(2, L, N, generator=g) + 1.0, torch.poisson(torch.full((2, H, N), 2.0), generator=g),
                torch.ones(2, H, N)) for _ in range(2)]
    with torch.no_grad():
        model(batches[0][0])
    before = {k: v.clone() for k, v in model.state_dict().items()}
    model.mu_head.bias.requires_grad_(False)
    flags = [p.requires_grad for p in model.parameters()]
    hidden, tail, hist, late, floor = model.head_inputs(batches[0][0])
    assert hidden.shape == (2, H, 16) and not hidden.requires_grad and hist == H and tail.shape == (2, H, N)
    losses = fit.refit_heads(model, batches, epochs=2, lr=1e-2)
    assert losses.shape == (4,) and bool(torch.isfinite(losses).all()) and fit._last_backend == "torch"
    assert model.training and [p.requires_grad for p in model.parameters()] == flags
    for k, v in model.state_dict().items():
        assert (not torch.equal(v, before[k])) == (k.startswith("mu_head.") or k.startswith("sigma_head.")), k
    with pytest.raises(ValueError, match="no batches"):
        fit.refit_heads(model, [])
    with pytest.raises(ValueError, match="head_nll: hidden"):
        fit.head_nll(hidden, model.mu_head.weight, model.mu_head.bias, model.sigma_head.weight, model.sigma_head.bias,
                     tail, hist, batches[0][1][:, :3])
    with torch.no_grad():
        model.mu_head.bias.fill_(float("nan"))
    with pytest.raises(RuntimeError, match="Predicted rate must be finite"):
        fit.refit_heads(model, batches[:1], optimizer=torch.optim.SGD(model.sigma_head.parameters(), lr=0.0))


FORMS = [  # (B, H, N, strides, misalign) -> (kernel, nparts)
    ((1, 1, 1, (0, 0, 0), 0), ("k_nb_grad<1>", 1)),
    ((6, 13, 8, (104, 104, 104), 0), ("k_nb_grad<4>", 1)),
    ((6, 13, 8, (104, 104, 104), 4), ("k_nb_grad<1>", 3)),
    ((6, 13, 8, (104, 106, 104), 0), ("k_nb_grad<1>", 3)),
    ((4096, 7, 1, (7, 7, 7), 0), ("k_nb_grad<1>", 112)),
    ((3, 7, 4, (28, 28, 28), 0), ("k_nb_grad<4>", 1)),
    ((3, 2, 6, (12, 12, 12), 0), ("k_nb_grad<4>", 1)),
    ((3, 7, 5, (35, 35, 35), 0), ("k_nb_grad<1>", 1)),
    ((256, 96, 512, (49152,) * 3, 0), ("k_nb_grad<4>", 1024)),
    ((256, 96, 512, (49152,) * 3, 8), ("k_nb_grad<1>", 1024)),
    ((5, 257, 1, (257,) * 3, 0), ("k_nb_grad<1>", 6)),
]


@pytest.mark.parametrize("args,want", FORMS)
def test_form_table(args, want, ftn):
    B, H, N, strides, mis = args
    assert ftn.runtime.nb_nll_grad_form_of(B, H, N, strides, mis) == want
    lib = ftn.lib.load()
    assert lib.ftn_nb_nll_grad_workspace(B, H, N) == 16 * min(1024, -(-B * H * N // 256))


A, M = 0x10000, 0x10004          # stand-ins for device addresses: 16-byte aligned / 4 bytes past a boundary
GOOD = dict(y=A, ybs=64, rate=A, rbs=64, disp=A, dbs=64, mask=None, kind=0, eps=1e-8, B=2, H=8, N=8, gr=A, gd=A + 64,
            loss=A, ws=A, wsb=16, scaled=1)
BAD = {
    "null y": dict(y=None), "null rate": dict(rate=None), "null dispersion": dict(disp=None),
    "null g_rate": dict(gr=None), "null g_disp": dict(gd=None), "null loss": dict(loss=None),
    "null workspace": dict(ws=None), "B = 0": dict(B=0), "H = 0": dict(H=0), "N < 0": dict(N=-1),
    "y batch stride below H N": dict(ybs=63), "rate batch stride below H N": dict(rbs=8),
    "negative stride": dict(dbs=-64), "H N beyond int32": dict(H=1 << 16, N=1 << 16, B=1),
    "B N beyond int32": dict(B=1 << 16, N=1 << 16, H=1), "mask without a kind": dict(mask=A),
    "kind without a mask": dict(kind=1), "unknown mask kind": dict(mask=A, kind=3), "eps = 0": dict(eps=0.0),
    "eps = 1": dict(eps=1.0), "y off by 2": dict(y=A + 2), "g_disp off by 1": dict(gd=A + 65),
    "workspace off by 4": dict(ws=M), "workspace too small": dict(wsb=8), "scaled = 2": dict(scaled=2),
    "one gradient buffer": dict(gd=A),
}


@pytest.mark.parametrize("name", list(BAD))
def test_entry_rejects_bad_arguments_before_any_launch(name, ftn):
    lib = ftn.lib.load()
    a = {**GOOD, **BAD[name]}
    assert lib.ftn_nb_nll_grad_form(2, 8, 8, 0, 0, 0, 0) > 0           # leaves an earlier message out of the way
    rc = lib.ftn_nb_nll_grad(a["y"], a["ybs"], a["rate"], a["rbs"], a["disp"], a["dbs"], a["mask"], a["kind"], a["eps"],
                             a["B"], a["H"], a["N"], a["gr"], a["gd"], a["loss"], a["ws"], a["wsb"], a["scaled"], None)
    assert rc < 0
    assert lib.ftn_last_error().decode().startswith("ftn_nb_nll_grad")
    with pytest.raises(ValueError, match="ftn_nb_nll_grad"):
        ftn.lib.check(rc, "ftn_nb_nll_grad")


@pytest.mark.parametrize("args", [(0, 8, 8, 0, 0, 0, 0), (2, 8, 8, -1, 0, 0, 0), (2, 8, 8, 0, 0, 0, 3),
                                  (2, 8, 8, 0, 0, 0, 16), (1, 1 << 16, 1 << 16, 0, 0, 0, 0)])
def test_form_rejects_bad_arguments(args, ftn):
    lib = ftn.lib.load()
    assert lib.ftn_nb_nll_grad_form(*args) < 0
    assert b"ftn_nb_nll_grad_form" in lib.ftn_last_error()
    assert lib.ftn_nb_nll_grad_workspace(0, 8, 8) == 0
