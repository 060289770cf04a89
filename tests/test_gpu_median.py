"""The channel medians of the selector front end (``ftn_period_spectrum``: S1+S2) at every width class of the median
network, against things that do not share its code: an fp64 rFFT on the host, the order of the channels, and exact ties.

One bitonic network serves every kernel: V registers per lane and row for C <= 64 V, +inf padding, V in {1, 2, 4};
beyond 256 channels ``k_spectrum`` counts ranks.  The widths below sit on both sides of every such edge (64 | 65,
128 | 129, 256 | 257), at the smallest sizes and at odd ones.  L = 8 (L % 4 == 0) sends 64 < C <= 128 through the
channel-tiled quarter-fold kernel and ``k_median_rows`` with B F = 15 rows, so its last wave is ragged; L = 18 keeps
every width in ``k_spectrum``; B = 64 reaches the two row-resident kernels.  Every case asserts the form it ran."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-4                     # tests/test_gpu_parity.py::test_selector_matches_reference, same quantities
WIDTHS = (1, 2, 31, 33, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 300)
SHAPES = ([(3, L, C) for L in (8, 18) for C in WIDTHS] + [(64, L, C) for L in (8, 10) for C in (5, 64)])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def expected_form(B, L, C):
    if B >= 64:
        return "k_spectrum_rowq" if L % 4 == 0 else "k_spectrum_row"
    return "k_spectrum_rowq_tiled" if L % 4 == 0 and 64 < C <= 128 else "k_spectrum"


@functools.lru_cache(maxsize=None)
def _input(B, L, C):
    g = torch.Generator().manual_seed(1000 * L + 7 * C + B)
    return torch.randn(B, L, C, generator=g) * 3.0


def _run(rt, x, dev, form):
    """med [B, F] fp32 and psum [F] fp64 of ``x`` as numpy arrays; the form the library chose is asserted."""
    B, L, C = x.shape
    assert rt.spectrum_form(B, L, C)[0] == form, (B, L, C)
    med, psum = rt.spectrum(x.contiguous().to(dev))
    return med.cpu().numpy(), psum.cpu().numpy()


_BASE = {}


def _base(rt, dev, shape):
    """The device result for the shape's own input: computed once, shared by the tests, never written."""
    if shape not in _BASE:
        med, psum = _run(rt, _input(*shape), dev, expected_form(*shape))
        med.setflags(write=False)
        psum.setflags(write=False)
        _BASE[shape] = (med, psum)
    return _BASE[shape]


def _lower_median(amp):
    """torch.median over the last axis: sorted[(C - 1) // 2]."""
    return np.sort(amp, axis=-1)[..., (amp.shape[-1] - 1) // 2]


@pytest.mark.parametrize("B,L,C", SHAPES)
def test_median_and_batch_sum_against_fp64(B, L, C, ftn, dev):
    med, psum = _base(ftn.runtime, dev, (B, L, C))
    amp64 = np.abs(np.fft.rfft(_input(B, L, C).numpy().astype(np.float64), axis=1))       # [B, F, C]
    med64 = _lower_median(amp64)
    scale = float(np.abs(med64).max())
    err = np.abs(med - med64)
    print(f"B={B} L={L} C={C}: max|med - fp64| = {err.max():.3e}, scale = {scale:.3e}")
    np.testing.assert_allclose(med, med64, rtol=RTOL, atol=2e-6 * scale)
    np.testing.assert_allclose(psum / B, med64.sum(0) / B, rtol=RTOL, atol=2e-6 * scale)
    # k_colsum adds the device's own medians in fp64: any order of B non-negative terms is within (B - 1) u of the
    # exact sum, so two orders differ by less than 2 B u (u = 2^-53)
    np.testing.assert_allclose(psum, med.astype(np.float64).sum(0), rtol=2 * B * 2.0 ** -53, atol=0)


@pytest.mark.parametrize("B,L,C", SHAPES)
def test_median_does_not_depend_on_channel_order(B, L, C, ftn, dev):
    """An MFMA column's amplitude does not depend on the column it sits in, and the median of a multiset not on its
    order: a permutation of the channels leaves every bit of med in place.  A network that does not sort fails here."""
    rt = ftn.runtime
    med, _ = _base(rt, dev, (B, L, C))
    x = _input(B, L, C)
    perms = [torch.arange(C - 1, -1, -1)]
    perms += [torch.randperm(C, generator=torch.Generator().manual_seed(s)) for s in (1, 2, 3)]
    for i, p in enumerate(perms):
        got, _ = _run(rt, x[..., p], dev, expected_form(B, L, C))
        assert got.tobytes() == med.tobytes(), f"permutation {i}"


def _column_amps(rt, dev, cols, quarter):
    """|rFFT| [N, F] of N single series [N, L], as the kernel family of the case computes it: C = 1 inputs whose median
    is the amplitude itself.  k_spectrum and k_spectrum_row run the same MFMA sequence on the same operands (any batch
    below 64 rows stays in k_spectrum); the quarter-fold kernels round differently and need at least 64 rows."""
    N, L = cols.shape
    x1 = cols.reshape(N, L, 1)
    if quarter:
        reps = -(-64 // N)
        return _run(rt, x1.repeat(reps, 1, 1), dev, "k_spectrum_rowq")[0][:N]
    return np.concatenate([_run(rt, x1[i:i + 63], dev, "k_spectrum")[0] for i in range(0, N, 63)])


@pytest.mark.parametrize("B,L,C", SHAPES)
def test_median_of_exact_ties(B, L, C, ftn, dev):
    """Every channel duplicated (x[..., c] = x[..., c % m]): the median is, bit for bit, the lower median of the m
    distinct columns' amplitudes taken with their multiplicities, and no order of the duplicates changes it."""
    rt = ftn.runtime
    form = expected_form(B, L, C)
    x = _input(B, L, C)
    for m in sorted({m for m in (1, 3, math.ceil(C / 2)) if m <= C}):
        idx = torch.arange(C) % m
        xt = x[..., idx]
        got, _ = _run(rt, xt, dev, form)
        cols = x[..., :m].permute(0, 2, 1).reshape(B * m, L)                               # row b m + j = x[b, :, j]
        amps = _column_amps(rt, dev, cols, quarter=form.startswith("k_spectrum_rowq")).reshape(B, m, -1)
        want = _lower_median(amps.transpose(0, 2, 1)[..., idx.numpy()])                    # [B, F, C] -> [B, F]
        assert got.tobytes() == want.astype(np.float32).tobytes(), f"m={m}"
        p = torch.randperm(C, generator=torch.Generator().manual_seed(m))
        assert _run(rt, xt[..., p], dev, form)[0].tobytes() == got.tobytes(), f"m={m}, permuted"
