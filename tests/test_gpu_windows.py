"""Device windows on the MI355X (``ftn_window_batch`` behind ``windows.DeviceWindows``): the HIP backend against every
batch the reference's loader yielded (tests/golden/windows_cases.npz) and, bit for bit, against the torch backend on
the same device tensors over the sweep of tests/windows_checks.py - N in {1, 5, 63, 64, 65, 193} x L in {1, 7, 28,
63, 64, 65, 130}, H, stride, F, Fs, ids and mask rotating, both layouts, batch sizes 1, N - 1, N, N + 1, 2 N + 3 and
one batch over every window - with -0, inf and NaN payloads among the values; one batch of 70 000 items; tables that
are column slices or sit one float off the 16-byte grid, with the forms the table test pins and outputs carved out of
a poisoned buffer; and end to end: ``eval_metrics`` over ``DeviceWindows`` equals ``eval_metrics`` over the same
batches as a list, and a ``GraphedForward`` whose input buffer is filled through ``out=`` equals the eager call."""
import numpy as np
import pytest
import torch

import windows_checks as wc

pytestmark = pytest.mark.gpu
POISON = 0x5A5AA5A5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return wc.fixture()


def _on(dev, t):
    return {k: None if v is None else torch.from_numpy(v).to(dev) for k, v in t.items()}


def _windows(ftn, d, shape, bs, layout, backend):
    return ftn.windows.DeviceWindows(d["X"], shape["L"], shape["H"], stride=shape["stride"], valid_mask=d["M"],
                                     series_static=d["static"], series_ids=d["ids"], time_features=d["marks"],
                                     batch_size=bs, layout=layout, backend=backend)


def _outs_of(batch, layout):
    """The batch tuple as the ``outs`` of ``runtime.window_batch_form`` (empty marks and shared pieces left out)."""
    named = dict(zip(wc.PIECES[:5], batch[:5]))
    for t in batch[5:] if layout == "series" else ():
        named["id" if t.dtype == torch.int64 else "static"] = t
    return {n: t for n, t in named.items() if t.numel()}


@pytest.mark.parametrize("case", ["probe", "bare", "rec3", "rec1", "one", "none", "concat"])
def test_hip_backend_reproduces_the_loader(case, ftn, dev, fx):
    meta, arrays = fx
    m = meta[case]
    w = wc.build(ftn, meta, arrays, case, device=dev)
    assert w.backend == "hip" and len(w) == m["batches"]
    for i, b in enumerate(w):
        want = [torch.from_numpy(arrays[f"{case}:b{i}:{j}"]) for j in range(m["pieces"])]
        assert w._last_backend == "hip" and all(t.device == dev for t in b)
        assert wc.batches_same(b, want), (case, i)
    assert list(wc.build(ftn, meta, arrays, "none", device=dev)) == []


@pytest.mark.parametrize("N", wc.SWEEP_N)
def test_sweep_against_the_torch_backend(N, ftn, dev):
    rt = ftn.runtime
    compared = 0
    for at, shape in enumerate(wc.sweep(N)):
        d = _on(dev, wc.sweep_tables(shape, 100 * N + at))
        for layout in ("series", "wide"):
            n_items = _windows(ftn, d, shape, 1, layout, "torch").n_items
            for bs in wc.batch_sizes(N if layout == "series" else 2, n_items):
                hip, ref = (_windows(ftn, d, shape, bs, layout, b) for b in ("hip", "torch"))
                assert len(hip) == len(ref) == -(-n_items // bs)
                for i in sorted({0, min(1, len(hip) - 1), len(hip) // 2, len(hip) - 1}):
                    got, want = hip.batch(i), ref.batch(i)
                    assert hip._last_backend == "hip" and ref._last_backend == "torch"
                    assert wc.batches_same(got, want), (shape, layout, bs, i)
                    compared += 1
            outs = _outs_of(got, layout)                        # the last batch: fresh, aligned outputs
            form = rt.window_batch_form(d["X"], shape["L"], shape["H"], outs, M=d["M"], marks=d["marks"],
                                        statics=d["static"], ids=d["ids"], layout=layout)
            assert form == wc.want_form(layout, N, shape["L"], shape["H"], F=shape["F"], outs=tuple(outs),
                                        has_mask=shape["mask"]), (shape, layout)
    assert compared >= 9 * (3 + 3)                              # every shape: several batches in either layout


def test_special_values_survive(ftn, dev):
    """Every bit pattern class - NaNs with payloads, both infinities, -0, a denormal - through both layouts and both
    load widths (N = 64: 16-byte forms; N = 5: 4-byte forms)."""
    pat = torch.tensor([0x7FC00001, -0x3EDCBB, 0x7F800001, 0x7F800000, -0x800000, -0x80000000, 1, 0x3F800000],
                       dtype=torch.int32)
    for N in (5, 64):
        X = pat.repeat(-(-20 * N // 8))[:20 * N].view(20, N).to(dev).view(torch.float32)
        for layout in ("series", "wide"):
            w = ftn.windows.DeviceWindows(X, 8, 4, batch_size=7, layout=layout, backend="hip")
            r = ftn.windows.DeviceWindows(X, 8, 4, batch_size=7, layout=layout, backend="torch")
            for i in range(len(w)):
                assert wc.batches_same(w.batch(i), r.batch(i)), (N, layout, i)
            x = w.batch(0)[0]
            assert bool(torch.isnan(x).any()) and bool(torch.isinf(x).any())


def test_a_batch_beyond_the_grid_limit(ftn, dev):
    """70 000 items in one batch (L = 4, N = 7): no grid dimension carries the count."""
    g = np.random.default_rng(3)
    X = torch.from_numpy(g.standard_normal((10_005, 7)).astype(np.float32)).to(dev)
    marks = torch.from_numpy(g.standard_normal((10_005, 3)).astype(np.float32)).to(dev)
    ids = torch.arange(7, device=dev) * 11
    kw = dict(time_features=marks, series_ids=ids, batch_size=70_000)
    w = ftn.windows.DeviceWindows(X, 4, 2, backend="hip", **kw)
    r = ftn.windows.DeviceWindows(X, 4, 2, backend="torch", **kw)
    assert w.n_items == 70_000 and len(w) == 1
    got = w.batch(0)
    assert got[0].shape == (70_000, 4, 1) and wc.batches_same(got, r.batch(0))


def _carve(buf, at, like):
    """A contiguous view of ``like``'s shape and dtype at word ``at`` of the poisoned int32 buffer; the next free word."""
    words = like.numel() * (2 if like.dtype == torch.int64 else 1)
    return buf[at:at + words].view(like.dtype).view(like.shape), at + words


@pytest.mark.parametrize("N", [5, 64])
def test_views_forms_and_poisoned_surroundings(N, ftn, dev):
    """Tables as column slices of wider ones (row strides that are and are not multiples of 4) and as views one float
    off the 16-byte grid; outputs carved out of one poisoned buffer, on and off the grid, with guard words between
    them that must keep their pattern.  The forms are those of tests/test_windows_forms_table.py."""
    rt = ftn.runtime
    for at, shape in enumerate(wc.sweep(N)[4:]):                # L = 64, 65, 130 and the two all-vector shapes
        t = wc.sweep_tables(shape, 900 + at)
        T, F = shape["T"], shape["F"]
        for pad, off in ((8, 0), (3, 0), (0, 1), (8, 1)):       # columns added to a row; floats off the grid
            d = _on(dev, t)
            for name, cols in (("X", N), ("M", N), ("marks", F)):
                if d[name] is None:
                    continue
                big = torch.zeros(T * (cols + pad) + 4 + off, device=dev)      # the base is on the 16-byte grid
                big = big[off:off + T * (cols + pad)].view(T, cols + pad)
                big[:, :cols] = d[name]
                d[name] = big[:, :cols]
                assert d[name].data_ptr() % 16 == 4 * off and d[name].stride(0) == cols + pad
            for layout in ("series", "wide"):
                ref = _windows(ftn, d, shape, 2 * N + 3, layout, "torch")
                hip = _windows(ftn, d, shape, 2 * N + 3, layout, "hip")
                for i in range(len(hip)):
                    want = ref.batch(i)
                    fill = want[:5] if layout == "wide" else want
                    for out_off in (0, 1):
                        buf = torch.full((sum(2 * p.numel() + 16 for p in fill) + 64,), POISON, dtype=torch.int32,
                                         device=dev)
                        carved, spans, pos = [], [], 4 + out_off
                        for p in fill:
                            pos += pos % 2 if p.dtype == torch.int64 else 0      # ids: 8-byte aligned
                            v, end = _carve(buf, pos, p)
                            carved.append(v if p.numel() else None)
                            spans.append((pos, end))
                            pos = (end + 7) // 4 * 4 + out_off                   # at least 3 guard words
                        got = hip.batch(i, out=tuple(carved) + (None,) * (len(want) - len(fill)))
                        assert hip._last_backend == "hip" and wc.batches_same(got, want), (shape, pad, off, layout, i)
                        keep = torch.ones_like(buf, dtype=torch.bool)
                        for a, b in spans:
                            keep[a:b] = False
                        assert bool((buf[keep] == POISON).all()), (shape, pad, off, layout, i, out_off)
                        outs = _outs_of(got, layout)
                        mis = {n: v.data_ptr() % 16 for n, v in outs.items()}
                        mis.update({n: d[n].data_ptr() % 16 for n in ("X", "M", "marks") if d[n] is not None})
                        form = rt.window_batch_form(d["X"], shape["L"], shape["H"], outs, M=d["M"], marks=d["marks"],
                                                    statics=d["static"], ids=d["ids"], layout=layout)
                        assert form == wc.want_form(layout, N, shape["L"], shape["H"], F=F, outs=tuple(outs),
                                                    x_stride=N + pad, m_stride=N + pad, marks_stride=F + pad,
                                                    has_mask=shape["mask"], misalign=mis), (shape, pad, off, layout)


# ---------------------------------------------------------------------------------------------------- end to end
def _tiny_model(ftn, dev, L, H, N, mode, **first):
    """The tiny TimesNet of tests/test_gpu_score.py (d_model 16, 2 blocks), built for N series; ``first``: the
    keyword tensors of its first call (statics and ids bind their layers there)."""
    cfg = dict(input_len=L, pred_len=H, d_model=16, d_ff=32, n_layers=2, k_periods=3, kernel_set=[(3, 3), (5, 5)],
               dropout=0.0, activation="gelu", mode=mode, use_checkpoint=False)
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(0)
    model = ftn.models.TimesNet(**cfg).eval().to(dev)           # on the device first: what the first call binds lives there
    with torch.no_grad():
        model((torch.rand(2, L, N, generator=g) + 1.0).to(dev), **{k: v.to(dev) for k, v in first.items()})
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_((0.1 * torch.randn(p.shape, generator=g)).to(dev))
    return model


def _table(T, N, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float32).view(T, 1)
    X = torch.poisson(2.0 + 1.5 * torch.sin(2 * torch.pi * t / 6.0) + torch.rand(T, N, generator=g), generator=g)
    return X, (torch.rand(T, N, generator=g) >= 0.2).float()


@pytest.mark.parametrize("mode", ["direct", "recursive"])
def test_eval_metrics_over_device_windows(mode, ftn, dev):
    """A whole rolling-origin backtest in the pipeline layout (one series per batch row): the same dictionary, bit for
    bit, as ``eval_metrics`` over the same batches materialised as a list by the torch backend."""
    sc = ftn.score
    L, H, N, T = 24, 6, 5, 40
    model = _tiny_model(ftn, dev, L, H, 1, mode, series_static=torch.rand(2, 1, 2),
                        series_ids=torch.tensor([[4], [0]]))
    X, M = _table(T, N, 5)
    static = torch.rand(N, 2, generator=torch.Generator().manual_seed(2))
    kw = dict(mode=mode, recursive_pred_len=H, stride=2, valid_mask=M, series_static=static,
              series_ids=torch.arange(N), batch_size=8, device=dev)
    w = ftn.windows.DeviceWindows(X, L, H, backend="hip", **kw)
    listed = list(ftn.windows.DeviceWindows(X, L, H, backend="torch", **kw))
    assert len(w) == len(listed) == 4 and w.n_items == 30 and listed[-1][0].shape == (6, L, 1)
    via = sc.eval_metrics(model, w, mode, H, use_loss_mask=True, n_series=N)
    assert w._last_backend == "hip"
    want = sc.eval_metrics(model, listed, mode, H, use_loss_mask=True, n_series=N)
    assert set(via) == set(want)
    for k in want:
        assert np.array_equal(np.asarray(via[k]), np.asarray(want[k]), equal_nan=True), (mode, k)
    assert np.isfinite(via["nll"]) and np.isfinite(via["smape"]) and int(np.sum(via["nll_count"])) > 0


def test_out_fills_a_captured_forward(ftn, dev):
    """``out=`` writes a batch straight into the input buffer of a ``GraphedForward``; the replay equals the eager
    forward on ``w.batch(i)``, and the short last batch runs eagerly."""
    L, H, N, T, B = 24, 6, 24, 37, 3
    model = _tiny_model(ftn, dev, L, H, N, "direct")
    X, M = _table(T, N, 9)
    w = ftn.windows.DeviceWindows(X, L, H, valid_mask=M, batch_size=B, layout="wide", device=dev, backend="hip")
    assert len(w) == 3 and w.n_items == 8
    first = w.batch(0)
    g = ftn.graph.GraphedForward(model, first[0])
    yb, mb = torch.empty_like(first[1]), torch.empty_like(first[2])
    for i in range(2):
        back = w.batch(i, out=(g.inputs[0], yb, mb, None, None))
        assert back[0] is g.inputs[0] and back[1] is yb
        rate, disp = g.replay()
        fresh = w.batch(i)
        with torch.inference_mode():
            want_rate, want_disp = model(fresh[0])
        assert wc.same_bits(rate, want_rate) and wc.same_bits(disp, want_disp), i
        assert wc.same_bits(yb, fresh[1]) and wc.same_bits(mb, fresh[2])
    last = w.batch(2)
    assert last[0].shape == (2, L, N)
    with torch.inference_mode():
        rate, _ = model(last[0])
    assert rate.shape == (2, H, N) and bool(torch.isfinite(rate).all())
