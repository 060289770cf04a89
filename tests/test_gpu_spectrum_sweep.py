"""The time and frequency axis of the selector front end (``ftn_period_spectrum``, ``csrc/spectrum.hip``) against things
that do not share its code: an fp64 rFFT on the host over the shapes of ``test_spectrum_forms_table.SWEEP`` (every
32-bin block count up to 17, every k-loop tail, both folds at L mod 4 = 0 .. 3, both sides of every fit limit), the
twiddle tables entry by entry against fp64, the batch position of a row, the load width, the bytes around the outputs
and the edges of the value range.  ``FTN_SEL_ROW`` is never set: every case asserts the form the library chose."""
import functools

import numpy as np
import pytest
import torch

from test_spectrum_forms_table import P, Q, R, SWEEP, T

pytestmark = pytest.mark.gpu

RTOL = 1e-4                     # tests/test_gpu_median.py and test_gpu_parity.py::test_selector_matches_reference
ATOL_OF_SCALE = 2e-6            # times max |med64|


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _input(B, L, Cn):
    g = torch.Generator().manual_seed(1000 * L + 7 * Cn + B)
    return torch.randn(B, L, Cn, generator=g) * 3.0


def _run(rt, x, dev, form):
    """med [B, F] fp32 and psum [F] fp64 of the host tensor ``x``; the (name, vec) the library reports is asserted."""
    B, L, Cn = x.shape
    xd = x.contiguous().to(dev)
    assert rt.spectrum_form(B, L, Cn, xd.data_ptr() % 16) == form, (B, L, Cn)
    med, psum = rt.spectrum(xd)
    return med.cpu().numpy(), psum.cpu().numpy()


def _misaligned(x, dev):
    """``x`` on the device, 4 bytes past a 16-byte boundary."""
    buf = torch.empty(x.numel() + 4, dtype=torch.float32, device=dev)
    off = (-(buf.data_ptr() // 4)) % 4 + 1
    xm = buf[off:off + x.numel()].view(x.shape)
    xm.copy_(x)
    assert xm.is_contiguous() and xm.data_ptr() % 16 == 4
    return xm


# ---- a. med and psum against fp64 -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,Cn,form,vec", SWEEP)
def test_sweep_against_fp64(B, L, Cn, form, vec, ftn, dev):
    x = _input(B, L, Cn)
    med, psum = _run(ftn.runtime, x, dev, (form, bool(vec)))
    amp64 = np.abs(np.fft.rfft(x.numpy().astype(np.float64), axis=1))                       # [B, F, C]
    med64 = np.sort(amp64, axis=-1)[..., (Cn - 1) // 2]                                   # torch.median: the lower one
    scale = float(np.abs(med64).max())
    err = float(np.abs(med - med64).max())
    print(f"spectrum-sweep B={B} L={L} C={Cn} {form}{' vec' if vec else ''}: max|med - fp64| = {err:.3e}, "
          f"/ scale = {err / scale:.3e}")
    assert med.shape == (B, L // 2 + 1) and psum.shape == (L // 2 + 1,)
    # (C = 1: the median is the amplitude, so this line checks every (b, f) amplitude of the DFT itself)
    np.testing.assert_allclose(med, med64, rtol=RTOL, atol=ATOL_OF_SCALE * scale)
    np.testing.assert_allclose(psum / B, med64.sum(0) / B, rtol=RTOL, atol=ATOL_OF_SCALE * scale)
    # k_colsum adds the device's own medians in fp64: any order of B non-negative terms is within (B - 1) u of the
    # exact sum, so two orders differ by less than 2 B u (u = 2^-53)
    np.testing.assert_allclose(psum, med.astype(np.float64).sum(0), rtol=2 * B * 2.0 ** -53, atol=0)


# ---- b. the twiddle tables ----------------------------------------------------------------------------------------
_QUARTER_COS = np.array([1.0, 0.0, -1.0, 0.0])
_QUARTER_SIN = np.array([0.0, 1.0, 0.0, -1.0])


def _check_plane(got, f, t, L, valid, sin, what):
    """One [t][f] plane of the table against fp64: |tab - fp64| <= 2^-24 (half an fp32 ulp at 1: what rounding an fp64
    value of magnitude <= 1 to fp32 allows), exact zeros where ``valid`` is false, exact 0 / +-1 at quarter turns."""
    m = (f[None, :].astype(np.int64) * t[:, None].astype(np.int64)) % L                    # exact
    ang = 2.0 * np.pi * m.astype(np.float64) / L
    want = np.where(valid, np.sin(ang) if sin else np.cos(ang), 0.0)
    assert got.shape == want.shape, what
    bad = np.abs(got.astype(np.float64) - want) > 2.0 ** -24
    assert not bad.any(), (what, L, np.argwhere(bad)[:4].tolist())
    assert not got[~valid].any(), (what, L, "non-zero padding")
    quarter = valid & ((4 * m) % L == 0)
    exact = (_QUARTER_SIN if sin else _QUARTER_COS)[((4 * m) // L)[quarter]]
    assert (got[quarter] == exact).all(), (what, L, "quarter turns")


@pytest.mark.parametrize("L", [2, 3, 8, 12, 63, 64, 124, 128, 336, 1024])
def test_twiddle_tables_against_fp64(L, ftn, dev):
    lib = ftn.lib.load()
    F = L // 2 + 1
    FPAD = (F + 31) // 32 * 32
    quarter = L >= 8 and L % 4 == 0
    QP, FQ = (L // 4 + 2) // 2 * 2, ((F + 1) // 2 + 31) // 32 * 32
    floats = 2 * L * FPAD + (4 * QP * FQ if quarter else 0)
    assert lib.ftn_dft_table_bytes(L) == 4 * floats
    cached = ftn.runtime.state(dev).dft_table(L)
    assert cached.dtype == torch.float32 and cached.numel() == floats
    # built again inside a larger buffer: nothing is written behind the table
    guard = 64
    buf = torch.full((floats + guard,), -7.0, dtype=torch.float32, device=dev)
    assert lib.ftn_dft_table_init(buf.data_ptr(), L, torch.cuda.current_stream(dev).cuda_stream) == 0
    tab = buf.cpu().numpy()
    assert (tab[floats:] == -7.0).all()
    tab = tab[:floats]
    assert tab.tobytes() == cached.cpu().numpy().tobytes()
    f, t = np.arange(FPAD), np.arange(L)
    valid = np.broadcast_to(f[None, :] < F, (L, FPAD))
    _check_plane(tab[:L * FPAD].reshape(L, FPAD), f, t, L, valid, False, "cos")
    _check_plane(tab[L * FPAD:2 * L * FPAD].reshape(L, FPAD), f, t, L, valid, True, "sin")
    if quarter:
        planes = tab[2 * L * FPAD:].reshape(4, QP, FQ)                                 # cos / sin even, cos / sin odd
        tq = np.arange(QP)
        for p, what in enumerate(("cos even", "sin even", "cos odd", "sin odd")):
            fq = 2 * np.arange(FQ) + p // 2
            valid = (fq[None, :] < F) & (tq[:, None] <= L // 4)
            _check_plane(planes[p], fq, tq, L, valid, bool(p % 2), what)


# ---- c. a row does not depend on its batch ------------------------------------------------------------------------
# (B, L, C, rows of the sub-batch): F > 32, L mod 4 = 0 and != 0 where the form exists there; 64 of 70 rows keep a row
# form, any batch keeps k_spectrum (C = 130 at B >= 64) and the channel-tiled form
BATCH_CASES = [(9, 128, 33, (3, 6)), (9, 66, 33, (3, 6)), (70, 66, 130, (3, 67)),
               (70, 130, 5, (3, 67)), (70, 400, 64, (3, 67)), (70, 128, 5, (3, 67)), (70, 128, 64, (3, 67)),
               (9, 128, 100, (3, 6)), (70, 128, 100, (3, 67))]
BATCH_FORMS = [P, P, P, R, R, Q, Q, T, T]


@pytest.mark.parametrize("case,name", list(zip(BATCH_CASES, BATCH_FORMS)))
def test_row_does_not_depend_on_its_batch(case, name, ftn, dev):
    B, L, Cn, (b0, b1) = case
    rt = ftn.runtime
    form = rt.spectrum_form(B, L, Cn)
    assert form[0] == name and rt.spectrum_form(b1 - b0, L, Cn) == form
    x = _input(B, L, Cn)
    med, _ = _run(rt, x, dev, form)
    sub, _ = _run(rt, x[b0:b1], dev, form)
    assert sub.tobytes() == med[b0:b1].tobytes(), "a sub-batch changes the bits of its rows"
    # another batch position: another XCD and slot in k_spectrum, another workgroup in the row forms
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B + L))
    assert (perm != torch.arange(B)).any()
    moved, _ = _run(rt, x[perm], dev, form)
    assert moved.tobytes() == med[perm.numpy()].tobytes(), "moving a row changes its bits"


# ---- d. load width -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,Cn,name", [(64, 65, 64, R), (64, 64, 64, Q), (3, 64, 100, T),       # C % 4 == 0
                                         (65, 65, 5, R), (65, 64, 5, Q), (3, 64, 127, T)])        # C % 4 != 0
def test_scalar_loads_match_vector_loads(B, L, Cn, name, ftn, dev):
    """The two load widths of a row form differ in loads, not in arithmetic: x at 4 bytes past a 16-byte boundary gives
    the bits of the aligned call (for C % 4 != 0 both are the scalar form)."""
    rt = ftn.runtime
    x = _input(B, L, Cn).to(dev)
    xm = _misaligned(x, dev)
    assert x.data_ptr() % 16 == 0
    assert rt.spectrum_form(B, L, Cn, 0) == (name, Cn % 4 == 0)
    assert rt.spectrum_form(B, L, Cn, xm.data_ptr() % 16) == (name, False)
    med_a, psum_a = rt.spectrum(x)
    med_m, psum_m = rt.spectrum(xm)
    assert med_m.cpu().numpy().tobytes() == med_a.cpu().numpy().tobytes()
    assert psum_m.cpu().numpy().tobytes() == psum_a.cpu().numpy().tobytes()


# ---- e. only the outputs are written -------------------------------------------------------------------------------
SENTINEL = 0x7FF8A5A5           # a NaN as fp32 and, doubled, as fp64: an element left unwritten is not finite either


def _sentinel_buffer(n_inner, itemsize, guard, dev):
    """``guard`` bytes, ``n_inner`` elements, ``guard`` bytes, all 32-bit words SENTINEL."""
    words = (2 * guard + n_inner * itemsize) // 4
    return torch.full((words,), SENTINEL, dtype=torch.int32, device=dev)


@pytest.mark.parametrize("B,L,Cn,name", [(3, 64, 33, P), (64, 65, 5, R), (64, 64, 5, Q), (3, 64, 100, T)])
def test_only_the_outputs_are_written(B, L, Cn, name, ftn, dev):
    """F = 33: the second 32-bin block has 31 padded bins.  med, psum and the scratch of the tiled form sit inside
    larger buffers; through the C entry, everything around them keeps its bits and everything inside is finite."""
    rt, lib = ftn.runtime, ftn.lib.load()
    F = L // 2 + 1
    assert F == 33 and rt.spectrum_form(B, L, Cn)[0] == name
    x = _input(B, L, Cn).to(dev)
    guard = 1024                                                                         # bytes: keeps every alignment
    nscr = int(lib.ftn_period_spectrum_scratch_bytes(B, L, Cn))
    assert (nscr == 4 * B * F * Cn) if name == T else (nscr == 0)
    sizes = {"med": (B * F, 4), "psum": (F, 8), "scratch": (nscr // 4, 4)}
    bufs = {k: _sentinel_buffer(n, size, guard, dev) for k, (n, size) in sizes.items()}
    ptr = {k: b.data_ptr() + guard for k, b in bufs.items()}
    rc = lib.ftn_period_spectrum(x.data_ptr(), B, L, Cn, rt.state(dev).dft_table(L).data_ptr(), ptr["med"], ptr["psum"],
                                 torch.cuda.current_stream(dev).cuda_stream, None, ptr["scratch"] if nscr else None)
    assert rc == 0, lib.ftn_last_error()
    torch.cuda.synchronize(dev)
    out = {}
    for k, (n, size) in sizes.items():
        words = bufs[k].cpu().numpy()
        g, inner = guard // 4, n * size // 4
        assert (words[:g] == SENTINEL).all() and (words[g + inner:] == SENTINEL).all(), f"{k}: written outside"
        out[k] = words[g:g + inner].view(np.float64 if size == 8 else np.float32)
        assert np.isfinite(out[k]).all(), f"{k}: {int((~np.isfinite(out[k])).sum())} elements unwritten or not finite"
    med, psum = rt.spectrum(x)
    assert out["med"].tobytes() == med.cpu().numpy().tobytes()
    assert out["psum"].tobytes() == psum.cpu().numpy().tobytes()


# ---- f. edges of the value range -----------------------------------------------------------------------------------
EDGE_SHAPES = [(3, 12, 5, P), (64, 10, 8, R), (64, 12, 8, Q), (3, 12, 100, T)]


@pytest.mark.parametrize("B,L,Cn,name", EDGE_SHAPES)
def test_zero_batch_gives_exact_zeros(B, L, Cn, name, ftn, dev):
    form = ftn.runtime.spectrum_form(B, L, Cn)
    assert form[0] == name
    med, psum = _run(ftn.runtime, torch.zeros(B, L, Cn), dev, form)
    assert not med.any() and not psum.any()


@pytest.mark.parametrize("k", [20, -20])
@pytest.mark.parametrize("B,L,Cn,name", EDGE_SHAPES)
def test_power_of_two_scale_commutes(B, L, Cn, name, k, ftn, dev):
    """x 2^k scales every sum by 2^k and the square under the root by 4^k without a rounding, and the hardware root of
    4^k y is 2^k times the root of y: med scales exactly (|x| <= 16 and 2^-23 |x| stay far inside the fp32 range)."""
    form = ftn.runtime.spectrum_form(B, L, Cn)
    assert form[0] == name
    x = _input(B, L, Cn)
    med, _ = _run(ftn.runtime, x, dev, form)
    scaled, _ = _run(ftn.runtime, x * 2.0 ** k, dev, form)
    assert np.isfinite(scaled).all() and med.min() > 2.0 ** -40
    assert scaled.tobytes() == (med * np.float32(2.0 ** k)).tobytes()


@pytest.mark.parametrize("B,L,Cn,name", EDGE_SHAPES)
def test_one_nan_makes_its_row_nan(B, L, Cn, name, ftn, dev):
    """One NaN sample makes its channel NaN in every bin, and ``torch.median`` over the channels propagates it: the
    row's med is NaN (never a finite median of the other channels), every other row keeps its bits."""
    form = ftn.runtime.spectrum_form(B, L, Cn)
    assert form[0] == name
    x = _input(B, L, Cn)
    med, _ = _run(ftn.runtime, x, dev, form)
    xn = x.clone()
    xn[1, L - 1, Cn - 1] = float("nan")
    got, _ = _run(ftn.runtime, xn, dev, form)
    assert np.isnan(got[1]).all(), got[1]
    assert np.delete(got, 1, axis=0).tobytes() == np.delete(med, 1, axis=0).tobytes()
