"""The element loop that ``k_nb_cdf``, ``k_nb_quantile`` and ``k_nb_sample`` share (csrc/ftn_nbq.h: nq_first, nq_at,
nq_load, NQ_LANE, NQ_RAISE) at the shapes where it can go wrong: one element, one quad, a ragged second workgroup in
either form, and batch strides that exceed H N and differ between the operands.  The result of a kernel must not
depend on its form: every case runs on 16-byte-aligned operands and again on copies 4 bytes off a boundary (the scalar
form wherever the first was the vector form), the two are compared bit for bit, and guard words behind every output
must come back untouched.  Rates in [0.5, 50] and dispersions in [0.05, 1] keep every answer far below 2^24, so the
flag stays 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 8
SENTINEL = -12345.0
LEVELS = [0.1, 0.9]
S, SEED, OFFSET = 5, (0x5EED << 32) | 0xF00D, 3          # S = 5: a second Philox block

# (shape, batch strides of (y, rate, disp) in elements, or None for contiguous operands)
CASES = {
    "one element": ((1, 1, 1), None),
    "one quad": ((1, 1, 4), None),
    "vector, ragged second workgroup": ((1, 257, 4), None),
    "scalar, ragged second workgroup": ((1, 257, 1), None),
    "batch strides of their own": ((2, 3, 4), (24, 16, 20)),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _place(vals, bstride, off, dev):
    """``vals`` [B,H,N] on the device as a view with batch stride ``bstride`` that starts ``off`` elements into its
    buffer (torch's allocations are 16-byte aligned: asserted)."""
    B, H, N = vals.shape
    bstride = H * N if bstride is None else bstride
    buf = torch.zeros(off + (B - 1) * bstride + H * N, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf.as_strided((B, H, N), (bstride, N, 1), off)
    v.copy_(vals)
    assert v.data_ptr() % 16 == 4 * off and (B == 1 or v.stride(0) == bstride)
    return v


def _guarded(shape, dev):
    """A contiguous fp32 output of ``shape`` with GUARD sentinel words behind it: ``(out, guard)``."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, device=dev)
    return buf[:n].view(shape), buf[n:]


def _run(ftn, dev, y, rate, disp):
    """The three kernels on these operands: ``(cdf, quantiles, samples)`` as int32 bit patterns on the host."""
    rt, lib = ftn.runtime, ftn.lib.load()
    B, H, N = rate.shape
    stream = torch.cuda.current_stream(dev).cuda_stream
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    F, gF = _guarded((B, H, N), dev)
    rc = lib.ftn_nb_cdf(y.data_ptr(), y.stride(0), rate.data_ptr(), rate.stride(0), disp.data_ptr(), disp.stride(0),
                        B, H, N, 1e-8, F.data_ptr(), None, flag.data_ptr(), stream)
    ftn.lib.check(rc, "ftn_nb_cdf")
    Q, gQ = _guarded((len(LEVELS), B, H, N), dev)
    rt.nb_quantiles(rate, disp, LEVELS, out=Q, flag=flag)
    X, gX = _guarded((S, B, H, N), dev)
    rt.nb_sample(rate, disp, S, SEED, OFFSET, out=X, flag=flag)
    torch.cuda.synchronize(dev)
    assert int(flag) == 0
    for g in (gF, gQ, gX):
        assert bool((g == SENTINEL).all())
    assert bool(((F >= 0) & (F <= 1)).all()) and bool((Q[1] >= Q[0]).all()) and bool((Q >= 0).all())
    assert bool((X >= 0).all()) and bool((X == X.floor()).all())
    return tuple(t.view(torch.int32).cpu() for t in (F, Q, X))


@pytest.mark.parametrize("name", list(CASES))
def test_result_does_not_depend_on_the_form(name, ftn, dev):
    rt = ftn.runtime
    shape, strides = CASES[name]
    g = torch.Generator().manual_seed(sum(shape))
    rate = torch.rand(shape, generator=g) * 49.5 + 0.5
    disp = torch.rand(shape, generator=g) * 0.95 + 0.05
    y = torch.poisson(rate, generator=g)
    ys, rs, ds = strides if strides is not None else (None, None, None)
    runs, forms = [], []
    for off in (0, 1):
        yv, rv, dv = _place(y, ys, off, dev), _place(rate, rs, off, dev), _place(disp, ds, off, dev)
        forms.append((rt.nbq_form(rv, dv, yv), rt.nbq_form(rv, dv), rt.nb_sample_form(rv, dv)))
        runs.append(_run(ftn, dev, yv, rv, dv))
    first = "vec4" if shape[2] % 4 == 0 else "scalar"
    assert forms[0] == (first,) * 3 and forms[1] == ("scalar",) * 3, forms
    for a, b, kernel in zip(runs[0], runs[1], ("k_nb_cdf", "k_nb_quantile", "k_nb_sample")):
        assert torch.equal(a, b), (name, kernel, int((a != b).sum()))
