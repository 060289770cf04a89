"""The low-rank temporal context on the MI355X (``ftn_lrtc_basis``, ``ftn_lrtc_forward``: the 16 ``k_lrtc<RT,VEC,ADDX>``
forms, both coefficient-load forms, every lane geometry) against fp64 under an a-priori bound, plus the properties a
wrong index would break: writes confined to the output, a NaN confined to its series, a batch row independent of its
batch, the fused add equal to the separate one, and ``LowRankTemporalContext.forward`` adding ``add_to`` as torch does.

The accuracy metric (DESIGN section 4's convention): with the device's own fp32 basis b and column means m read back,
    ref = scale * sum_r (b[l,r] - m[r]) c[n,r] (+ x)                                             in fp64
    e   = |got - ref| / (|scale| sum_r |b[l,r]| |c[n,r]| + |scale| sum_r |m[r]| |c[n,r]| + |x|)  in u = 2^-24
and e <= R + 8 is asserted (one rounding of scale * c, R + RT fused multiply-adds, the add of x).
``test_every_form_ran`` prints the measured maximum per form (``-s``) beside the same e of the oracle's fp32 arithmetic
(einsum, time mean removed, scale) on the CPU, fed the same basis; DESIGN section 4 records that table.
"""
import numpy as np
import pytest
import torch

import oracle.timesblock_oracle as orc

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
GUARD, PAD = 1234.5, 64

RS = (1, 4, 5, 8, 9, 16, 17, 31, 32)
NS = (1, 3, 4, 5, 64, 252, 256, 260, 768, 1024, 1028, 2052)
LS = (1, 2, 47, 48, 49, 96, 97, 193, 385)
SCALES = (1e-6, -1.25, 1e6)
OFFSETS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))        # floats past the allocation: (x, out, coeff)

SWEPT = {}                                                    # R -> the compared cases of that rank, see _sweep


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _shifted(t, off, dev):
    """``t`` on the device, ``off`` floats into an allocation of its own (off = 1: 4 bytes past a 16-byte boundary)."""
    buf = torch.empty(t.numel() + off, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:].view(t.shape)
    view.copy_(t)
    return view


def _launch(ftn, dev, coeff, L, scale, x=None, offs=(0, 0, 0)):
    """``ftn_lrtc_forward`` through ``lib`` with out between guard words.  Returns (out [B,L,N] on the CPU, form)."""
    rt = ftn.runtime
    B, N, R = coeff.shape
    dc = _shifted(coeff, offs[2], dev)
    dx = None if x is None else _shifted(x, offs[0], dev)
    n = B * L * N
    buf = torch.full((PAD + offs[1] + n + PAD,), GUARD, device=dev)
    out = buf[PAD + offs[1]:PAD + offs[1] + n]
    assert (out.data_ptr() % 16 == 0) == (offs[1] == 0)
    form = rt.lrtc_form(dc, dx, out)
    basis = rt.state(dev).lrtc_basis(L, R)
    sc = torch.tensor([scale], dtype=torch.float32, device=dev)
    rc = ftn.lib.load().ftn_lrtc_forward(dc.data_ptr(), basis.data_ptr(), sc.data_ptr(),
                                         None if dx is None else dx.data_ptr(), out.data_ptr(), B, L, N, R,
                                         torch.cuda.current_stream(dev).cuda_stream)
    ftn.lib.check(rc, "ftn_lrtc_forward")
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:PAD + offs[1]] == GUARD).all()) and bool((host[PAD + offs[1] + n:] == GUARD).all()), \
        ("guard words overwritten", form, B, L, N, R)
    return host[PAD + offs[1]:PAD + offs[1] + n].view(B, L, N).clone(), form


def _ref(ftn, dev, coeff, L, scale, x):
    """(ref, den) in fp64 from the device's own basis; ``scale`` as the fp32 value the kernel reads."""
    R = coeff.shape[2]
    raw = ftn.runtime.state(dev).lrtc_basis(L, R).cpu().double()
    b, m = raw[:L * R].view(L, R), raw[L * R:]
    s = float(torch.tensor(scale, dtype=torch.float32))
    c = coeff.double()
    ref = s * torch.einsum("lr,bnr->bln", b - m, c)
    den = abs(s) * (torch.einsum("lr,bnr->bln", b.abs(), c.abs()) + torch.einsum("r,bnr->bn", m.abs(), c.abs())[:, None])
    if x is not None:
        ref, den = ref + x.double(), den + x.double().abs()
    return ref, den


def _einsum_fp32(ftn, dev, coeff, L, scale, x):
    """``orc.lrtc_forward``'s fp32 arithmetic (einsum, time mean removed, scale, + x) on the device's basis."""
    R = coeff.shape[2]
    b = ftn.runtime.state(dev).lrtc_basis(L, R).cpu()[:L * R].view(L, R)
    ctx = torch.einsum("lr,bnr->bln", b, coeff)
    ctx = (ctx - ctx.mean(dim=1, keepdim=True)) * torch.tensor(scale, dtype=torch.float32)
    return ctx if x is None else x + ctx


def _err_u(got, ref, den):
    den = torch.where(den > 0, den, torch.ones_like(den))
    return float(((got.double() - ref).abs() / den).max()) / U


def _case(iR, iN, addx):
    """The rotation of the table: every (R, N) pair runs plain and fused; L, B, the scale and which operand sits one
    float off a 16-byte boundary rotate so that each value meets every R and every N somewhere."""
    L = LS[(2 * iR + iN + addx) % len(LS)]
    B = (1, 3)[(iR + iN + addx) % 2]
    scale = SCALES[(iR + 2 * iN + addx) % 3]
    offs = OFFSETS[(iR + iN // 3 + 2 * addx) % 4] if (iN + iR) % 3 == 0 else OFFSETS[0]
    return L, B, scale, offs


def _sweep(R, ftn, dev):
    """Every N of the table at rank R, plain and fused, run and measured once: [(form, case, e, e of the fp32 einsum)].
    Only what was compared against fp64 is listed, so the coverage asserted at the end is coverage by comparison."""
    if R not in SWEPT:
        iR, rows = RS.index(R), []
        for iN, N in enumerate(NS):
            for addx in (0, 1):
                L, B, scale, offs = _case(iR, iN, addx)
                g = torch.Generator().manual_seed(10000 * R + 10 * N + addx)
                coeff = torch.randn(B, N, R, generator=g)
                x = torch.randn(B, L, N, generator=g) * abs(scale) if addx else None
                got, form = _launch(ftn, dev, coeff, L, scale, x, offs)
                want = ftn.runtime.lrtc_form_of(N, R, addx,
                                                (4 * (offs[1] | (offs[0] if addx else 0))) | 4 * offs[2] << 4)
                assert form == want, (form, want)
                assert bool(torch.isfinite(got).all())
                ref, den = _ref(ftn, dev, coeff, L, scale, x)
                e_cpu = _err_u(_einsum_fp32(ftn, dev, coeff, L, scale, x), ref, den)
                rows.append((form, (B, L, N, R, scale, offs), _err_u(got, ref, den), e_cpu))
        SWEPT[R] = rows
    return SWEPT[R]


@pytest.mark.parametrize("R", RS)
def test_accuracy_against_fp64(R, ftn, dev):
    for form, case, e, _ in _sweep(R, ftn, dev):
        assert e <= R + 8, (form, case, e)


@pytest.mark.parametrize("L,R", [(1, 1), (1, 4), (2, 1), (2, 5), (3, 8), (24, 4), (47, 32), (150, 1), (336, 16),
                                 (720, 32)])
def test_basis_matches_the_oracle(L, R, ftn, dev):
    """``k_lrtc_basis`` against ``orc.lrtc_basis`` at the tolerance of ``test_gpu_parity.py``; L = 1 (the column
    collapses to 0 through the eps clamp), L = 2, and more columns than time steps included.  The stored column means
    are those of the stored columns."""
    raw = ftn.runtime.state(dev).lrtc_basis(L, R).cpu()
    assert raw.numel() == (L + 1) * R and bool(torch.isfinite(raw).all())
    b, m = raw[:L * R].view(L, R), raw[L * R:]
    np.testing.assert_allclose(b.numpy(), orc.lrtc_basis(L, R).numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(m.numpy(), b.double().mean(dim=0).numpy(), rtol=0, atol=2 * U)
    if L == 1:
        assert bool((b == 0).all()) and bool((m == 0).all())


@pytest.mark.parametrize("N,R,L,offs", [(5, 4, 49, (0, 0, 0)), (260, 16, 97, (0, 0, 0)), (1028, 8, 50, (0, 0, 1)),
                                        (1027, 32, 193, (0, 1, 0)), (768, 9, 2, (0, 0, 0))])
def test_nan_coefficient_stays_in_its_series(N, R, L, offs, ftn, dev):
    g = torch.Generator().manual_seed(N + R)
    coeff = torch.randn(2, N, R, generator=g)
    hits = [(0, 0, 0), (1, N - 1, R - 1), (0, N // 2, R // 2)]
    for b, n, r in hits:
        coeff[b, n, r] = float("nan")
    got, _ = _launch(ftn, dev, coeff, L, 0.5, None, offs)
    want = torch.zeros(2, L, N, dtype=torch.bool)
    for b, n, _ in hits:
        want[b, :, n] = True
    assert torch.equal(torch.isnan(got), want)


@pytest.mark.parametrize("N,R,L,addx", [(5, 4, 49, 1), (256, 16, 96, 0), (260, 17, 97, 1), (1028, 8, 193, 1),
                                        (2052, 32, 48, 0), (3, 1, 385, 1)])
def test_row_is_bit_identical_in_any_batch(N, R, L, addx, ftn, dev):
    g = torch.Generator().manual_seed(N + R + L)
    coeff = torch.randn(3, N, R, generator=g)
    x = torch.randn(3, L, N, generator=g) if addx else None
    full, _ = _launch(ftn, dev, coeff, L, -1.25, x)
    for b in range(3):
        one, _ = _launch(ftn, dev, coeff[b:b + 1], L, -1.25, None if x is None else x[b:b + 1])
        assert torch.equal(one, full[b:b + 1]), b


@pytest.mark.parametrize("N,R,L,offs", [(5, 4, 49, (0, 0, 0)), (256, 16, 96, (0, 0, 0)), (256, 16, 96, (1, 0, 0)),
                                        (260, 5, 97, (0, 1, 0)), (1028, 32, 47, (0, 0, 0)), (768, 31, 2, (0, 0, 0)),
                                        (1, 8, 385, (0, 0, 0))])
def test_fused_add_equals_the_separate_add(N, R, L, offs, ftn, dev):
    """fused = fl(x + ctx) with the ctx the plain call stores: within 1 u of |x| + |ctx| (half an ulp of the sum)."""
    g = torch.Generator().manual_seed(N + R + L)
    coeff = torch.randn(3, N, R, generator=g)
    x = torch.randn(3, L, N, generator=g) * 3.0
    plain, _ = _launch(ftn, dev, coeff, L, 1.5, None, offs)
    fused, _ = _launch(ftn, dev, coeff, L, 1.5, x, offs)
    err = (fused.double() - (x.double() + plain.double())).abs()
    assert bool((err <= U * (x.double().abs() + plain.double().abs())).all()), float(err.max())


# ------------------------------------------------------------------------------------------------ the module's forward
ADD_SHAPES = {"dense": (3, 49, 5), "[1, L, N]": (1, 49, 5), "[L, N]": (49, 5), "[B, 1, 1]": (3, 1, 1), "[N]": (5,),
              "scalar": (), "[2, B, L, N]": (2, 3, 49, 5)}


@pytest.mark.parametrize("name", list(ADD_SHAPES))
def test_forward_adds_every_shape_as_torch_adds(name, ftn, dev):
    """``forward(coeff, L, add_to)`` on the HIP branch = ``add_to + forward(coeff, L)``: a dense [B, L, N] inside the
    kernel, anything else broadcast by torch; the same shape and, to 1 u, the same values as the CPU's torch branch."""
    mod = ftn.models.LowRankTemporalContext(4, 0.5).eval()
    g = torch.Generator().manual_seed(11)
    coeff = torch.randn(3, 5, 4, generator=g)
    add = torch.randn(ADD_SHAPES[name], generator=g)
    with torch.no_grad():
        want = mod(coeff, 49, add_to=add)
    assert mod._last_backend == "torch"
    mod = mod.to(dev)
    with torch.inference_mode():
        ctx = mod(coeff.to(dev), 49)
        got = mod(coeff.to(dev), 49, add_to=add.to(dev))
    assert mod._last_backend == "hip"
    assert got.shape == want.shape and got.dtype == want.dtype
    both = (add.double() + ctx.cpu().double())
    assert bool(((got.cpu().double() - both).abs() <= U * (add.double().abs() + ctx.cpu().double().abs())).all())
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("shape", [(3, 49, 4), (3, 48, 5), (2, 49, 5), (3, 49, 5, 1), (4, 49, 5)])
def test_forward_rejects_what_torch_rejects(shape, ftn, dev):
    """A shape ``add_to + ctx`` cannot broadcast raises torch's error on the HIP branch too (never an out-of-bounds
    read of add_to), with the same message."""
    mod = ftn.models.LowRankTemporalContext(4, 0.5).eval()
    coeff = torch.zeros(3, 5, 4)
    with torch.no_grad(), pytest.raises(RuntimeError) as cpu_err:
        mod(coeff, 49, add_to=torch.zeros(shape))
    mod = mod.to(dev)
    with torch.inference_mode(), pytest.raises(RuntimeError) as dev_err:
        mod(coeff.to(dev), 49, add_to=torch.zeros(shape, device=dev))
    assert mod._last_backend == "hip"
    assert str(dev_err.value) == str(cpu_err.value)


def test_add_to_on_another_device_raises_as_torch_raises(ftn, dev):
    mod = ftn.models.LowRankTemporalContext(4, 0.5).eval().to(dev)
    with torch.inference_mode(), pytest.raises(RuntimeError, match="same device"):
        mod(torch.zeros(3, 5, 4, device=dev), 49, add_to=torch.zeros(3, 49, 5))


def test_rank_33_takes_the_torch_branch_with_equal_values(ftn, dev):
    """Beyond the kernel's 32 columns the module computes in torch, on the device: the same values as the fp64 oracle
    to the tolerance of the HIP branch, and rank 32 beside it on the kernel."""
    g = torch.Generator().manual_seed(33)
    for R, backend in ((33, "torch"), (32, "hip")):
        mod = ftn.models.LowRankTemporalContext(R, -1.25).eval().to(dev)
        coeff = torch.randn(2, 7, R, generator=g)
        add = torch.randn(2, 97, 7, generator=g)
        with torch.inference_mode():
            ctx = mod(coeff.to(dev), 97)
            fused = mod(coeff.to(dev), 97, add_to=add.to(dev))
        assert mod._last_backend == backend
        ref = orc.lrtc_forward(coeff.double(), 97, -1.25)
        scale = float(ref.abs().max())
        np.testing.assert_allclose(ctx.cpu().numpy(), ref.numpy(), rtol=2e-5, atol=1e-5 * scale)
        np.testing.assert_allclose(fused.cpu().numpy(), (ref + add.double()).numpy(), rtol=2e-5, atol=1e-5 * scale)


def test_every_form_ran(ftn, dev):
    """All 16 ``k_lrtc<RT,VEC,ADDX>`` forms, each with both coefficient-load forms, and every lane geometry were
    compared against fp64 by the accuracy table (run here for whatever rank has not been yet); prints the table of
    DESIGN section 4: per form, the largest e as a share of its bound R + 8, and that case's e, rank and bound."""
    rows = [row for R in RS for row in _sweep(R, ftn, dev)]
    tf = ("false", "true")
    names = {f"k_lrtc<{rt},{v},{a}>" for rt in (4, 8, 16, 32) for v in tf for a in tf}
    print("\nform                   wide   kernel e [u]   at R   bound [u]   fp32 einsum on the CPU, max e [u]")
    for key in sorted({(f[0], f[1]) for f, _, _, _ in rows}):
        mine = [(e / (c[3] + 8), e, c[3], e_cpu) for f, c, e, e_cpu in rows if (f[0], f[1]) == key]
        _, e, R, _ = max(mine)
        print(f"{key[0]:22s} {str(key[1]):5s} {e:14.2f} {R:6d} {R + 8:11d} {max(m[3] for m in mine):35.3g}")
    assert {(f[0], f[1]) for f, _, _, _ in rows} == {(n, w) for n in names for w in (False, True)}
    for name in names:
        # a scalar-store form needs N % 4 != 0 (the table's such N are all below 256) or an operand off its boundary
        nqbs = {f[2] for f, _, _, _ in rows if f[0] == name}
        assert nqbs >= ({64, 128, 256} if name.split(",")[1] == "true" else {64}), (name, nqbs)
