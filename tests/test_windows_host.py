"""Device windows without a GPU: the torch backend of ``windows.DeviceWindows`` bit for bit against every batch the
reference's ``SlidingWindowDataset`` + ``DataLoader`` yielded (tests/golden/windows_cases.npz: shapes, dtypes, order,
empties, the short last batch, a two-part concat), the wide layout against an item-by-item numpy restatement, ``out=``
buffers, the reference's error texts, the rejections of ``concat``, and every argument error of ``ftn_window_batch``,
which the host checks before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import windows_checks as wc


@pytest.fixture(scope="module")
def fx():
    return wc.fixture()


def test_exports_and_abi(ftn):
    L = ftn.lib
    assert {"ftn_window_batch", "ftn_window_batch_form"} <= set(L.EXPORTS)
    assert L.ABI_VERSION == 14 and L.load().ftn_abi_version() == 14
    assert (L.FTN_WIN_SERIES, L.FTN_WIN_WIDE, L.FTN_WIN_TILE_SERIES, L.FTN_WIN_TILE_STEPS) == (0, 1, 64, 32)
    assert ftn.runtime.WINDOW_PIECES == wc.PIECES


@pytest.mark.parametrize("case", ["probe", "bare", "rec3", "rec1", "one", "none", "concat"])
def test_torch_backend_reproduces_the_loader(case, ftn, fx):
    meta, arrays = fx
    m = meta[case]
    w = wc.build(ftn, meta, arrays, case)
    assert len(w) == m["batches"] and w.backend == "torch"
    p0 = m["parts"][0]
    H = p0["pred_len"] if p0["mode"] == "direct" else (p0["recursive_pred_len"] or 1)
    assert (w.input_len, w.target_len) == (p0["L"], H)
    want_starts = [np.arange(0, p["T"] - p["L"] - H + 1, max(1, p["stride"])) for p in m["parts"]]
    assert w.starts.tolist() == np.concatenate(want_starts).tolist() and w.starts.dtype == np.int64
    assert w.n_windows == sum(len(s) for s in want_starts)
    assert w.n_items == sum(len(s) * p["N"] for s, p in zip(want_starts, m["parts"]))
    got = list(w)
    assert len(got) == m["batches"]
    for i, b in enumerate(got):
        want = [torch.from_numpy(arrays[f"{case}:b{i}:{j}"]) for j in range(m["pieces"])]
        assert isinstance(b, tuple) and wc.batches_same(b, want), (case, i, [tuple(t.shape) for t in b])
        assert w._last_backend == "torch"
        assert wc.batches_same(w.batch(i), want)                # random access gives the same batch
    if m["batches"]:
        assert wc.batches_same(w.batch(-1), got[-1])
        assert got[-1][0].shape[0] == w.n_items - (len(w) - 1) * m["batch"]      # the last batch is short
    with pytest.raises(IndexError):
        w.batch(len(w))
    if case == "probe":                                         # batch 1 straddles windows 0 and 1
        assert p0["N"] == 5 and m["batch"] == 4 and got[1][6].flatten().tolist() == [arrays["probe:p0:ids"][i]
                                                                                   for i in (4, 0, 1, 2)]
    if case == "bare":
        assert len(got[0]) == 5 and got[0][3].shape == (4, 0) and got[0][3].dtype == torch.float32
        assert bool((got[0][2] == 1.0).all())                   # no valid_mask: ones
        xb, yb, mask, x_mark, y_mark, static, ids = ftn.score._unpack_batch(got[0])
        assert x_mark is None and y_mark is None and static is None and ids is None


@pytest.mark.parametrize("case", ["probe", "bare", "rec3", "concat"])
def test_other_batch_sizes_and_out_buffers(case, ftn, fx):
    """Any batch size cuts the same item sequence; ``out=`` fills the caller's buffers and returns them."""
    meta, arrays = fx
    m = meta[case]
    whole = wc.build(ftn, meta, arrays, case, batch_size=10 ** 6)
    items = whole.batch(0)
    assert len(whole) == 1 and items[0].shape[0] == whole.n_items
    for bs in (1, 3, 7, whole.n_items):
        w = wc.build(ftn, meta, arrays, case, batch_size=bs)
        assert len(w) == -(-whole.n_items // bs)
        for i in sorted({0, min(1, len(w) - 1), len(w) // 2, len(w) - 1}):
            want = [t[i * bs:(i + 1) * bs] for t in items]
            assert wc.batches_same(w.batch(i), want), (case, bs, i)
            bufs = tuple(torch.full_like(t, 7) for t in want)
            back = w.batch(i, out=bufs)
            assert all(a is b for a, b in zip(back, bufs)) and wc.batches_same(back, want), (case, bs, i)
            some = tuple(b if j % 2 else None for j, b in enumerate(bufs))      # None: that piece is allocated
            back = w.batch(i, out=some)
            assert all(s is None or s is b for s, b in zip(some, back)) and wc.batches_same(back, want)
    w = wc.build(ftn, meta, arrays, case)
    first = w.batch(0)
    with pytest.raises(ValueError, match="entries"):
        w.batch(0, out=first[:-1])
    with pytest.raises(ValueError, match=r"out\[0\]"):
        w.batch(0, out=(first[0][:, :-1],) + first[1:])
    with pytest.raises(ValueError, match=r"out\[1\]"):
        w.batch(0, out=(first[0], first[1].double()) + first[2:])


@pytest.mark.parametrize("layout", ["series", "wide"])
def test_torch_backend_against_the_definition(layout, ftn):
    """Both layouts item by item (numpy slices, one item at a time), with and without the optional pieces."""
    for shape in wc.sweep(5) + wc.sweep(64)[:3]:
        t = wc.sweep_tables(shape, 7)
        w = ftn.windows.DeviceWindows(t["X"], shape["L"], shape["H"], stride=shape["stride"], valid_mask=t["M"],
                                      series_static=t["static"], series_ids=t["ids"], time_features=t["marks"],
                                      batch_size=4, layout=layout, device="cpu")
        assert w.n_items == w.n_windows * (shape["N"] if layout == "series" else 1)
        for i in range(len(w)):
            k0, k1 = 4 * i, min(4 * i + 4, w.n_items)
            want = wc.items_numpy(t["X"], t["M"], t["marks"], t["static"], t["ids"], shape["L"], shape["H"],
                                  shape["stride"], layout, k0, k1)
            want = [a.reshape(k1 - k0, 0) if a.size == 0 and a.ndim == 2 else a for a in want]
            assert wc.batches_same(w.batch(i), want), (layout, shape, i)


def test_reference_error_texts_and_own_rejections(ftn):
    DW = ftn.windows.DeviceWindows
    X = np.zeros((12, 3), np.float32)
    with pytest.raises(ValueError, match="valid_mask must match wide_values shape"):
        DW(X, 4, 2, valid_mask=np.ones((12, 2)))
    with pytest.raises(ValueError, match="wide_values must contain at least one series column"):
        DW(np.zeros((12, 0), np.float32), 4, 2, device="cpu")
    with pytest.raises(ValueError, match="time_features must align with the temporal dimension of wide_values"):
        DW(X, 4, 2, time_features=np.zeros((11, 2)), device="cpu")
    with pytest.raises(ValueError, match=r"time_features must be a 2D array of shape \[T, F\]"):
        DW(X, 4, 2, time_features=np.zeros((12, 2, 2)), device="cpu")
    with pytest.raises(ValueError, match=r"series_static must have shape \[num_series, num_features\]"):
        DW(X, 4, 2, series_static=np.zeros((4, 2)), device="cpu")
    with pytest.raises(ValueError, match="series_ids must be a 1D sequence"):
        DW(X, 4, 2, series_ids=np.zeros((3, 1), np.int64), device="cpu")
    with pytest.raises(ValueError, match="series_ids length must match number of series"):
        DW(X, 4, 2, series_ids=[1, 2], device="cpu")
    with pytest.raises(ValueError, match="mode"):
        DW(X, 4, 2, mode="both", device="cpu")
    with pytest.raises(ValueError, match="layout"):
        DW(X, 4, 2, layout="long", device="cpu")
    with pytest.raises(ValueError, match="backend"):
        DW(X, 4, 2, backend="numpy", device="cpu")
    with pytest.raises(ValueError, match="hip"):
        DW(X, 4, 2, backend="hip", device="cpu")                # a CPU table
    with pytest.raises(ValueError, match="batch_size"):
        DW(X, 4, 2, batch_size=0, device="cpu")
    one = DW(X, 4, 2, time_features=np.arange(12.0), series_static=np.arange(3.0), device="cpu")       # 1-D: one column
    b = one.batch(0)
    assert b[3].shape == (len(b[0]), 4, 1) and b[5].shape == (len(b[0]), 1, 1)
    empty = DW(X, 4, 2, time_features=np.zeros((12, 0)), device="cpu")                                 # F = 0: no marks
    assert empty.batch(0)[3].shape == (len(b[0]), 0)
    nothing = DW(X, 8, 5, device="cpu")                         # T < L + H
    assert len(nothing) == 0 and nothing.n_items == 0 and list(nothing) == [] and nothing.starts.size == 0
    with pytest.raises(ValueError, match="no batches"):
        ftn.score.eval_metrics(torch.nn.Linear(1, 1), nothing, "direct", 5)


def test_concat_rejects_what_collate_could_not_stack(ftn):
    DW = ftn.windows.DeviceWindows
    X, X2 = np.zeros((12, 3), np.float32), np.zeros((15, 2), np.float32)
    kw = dict(device="cpu")
    base = DW(X, 4, 2, time_features=np.zeros((12, 2)), series_static=np.zeros((3, 2)), series_ids=[0, 1, 2], **kw)
    full = dict(time_features=np.zeros((15, 2)), series_static=np.zeros((2, 2)), series_ids=[5, 6])
    ok = DW.concat([base, DW(X2, 4, 2, **full, **kw)], batch_size=5)
    assert ok.n_items == 7 * 3 + 10 * 2 and len(ok) == 9
    for name, change in (("input_len", dict(L=5)), ("target length", dict(H=3)),
                         ("time features", dict(time_features=np.zeros((15, 3)))),
                         ("time features", dict(time_features=None)),
                         ("static features", dict(series_static=np.zeros((2, 1)))),
                         ("series_static given", dict(series_static=None)),
                         ("series_ids given", dict(series_ids=None))):
        args = {**full, **{k: v for k, v in change.items() if k not in ("L", "H")}}
        other = DW(X2, change.get("L", 4), change.get("H", 2), **args, **kw)
        with pytest.raises(ValueError, match=name):
            DW.concat([base, other])
    with pytest.raises(ValueError, match="layouts"):
        DW.concat([DW(X, 4, 2, **kw), DW(X2, 4, 2, layout="wide", **kw)])
    with pytest.raises(ValueError, match="number of series"):
        DW.concat([DW(X, 4, 2, layout="wide", **kw), DW(X2, 4, 2, layout="wide", **kw)])
    with pytest.raises(ValueError, match="statics and ids"):
        DW.concat([DW(X, 4, 2, layout="wide", series_ids=[0, 1, 2], **kw)] * 2)
    with pytest.raises(ValueError, match="non-empty"):
        DW.concat([])
    wide = DW.concat([DW(X + 1, 4, 2, layout="wide", **kw), DW(X[:9] + 2, 4, 2, layout="wide", **kw)], batch_size=4)
    assert [b[0].shape[0] for b in wide] == [4, 4, 3] and wide.batch(1)[0][:, 0, 0].tolist() == [1.0, 1.0, 1.0, 2.0]


def test_runtime_rejects_wrong_tensors_before_the_c_call(ftn):
    rt = ftn.runtime
    X = torch.zeros(12, 3)
    starts = torch.zeros(2, dtype=torch.int32)
    host = np.zeros(2, np.int32)
    with pytest.raises(ValueError, match="ROCm"):
        rt.window_batch(X, starts, host, 4, 2, 0, 2, {"x": torch.zeros(2, 4)})          # a CPU table
    with pytest.raises(ValueError, match="layout"):
        rt.window_batch(X, starts, host, 4, 2, 0, 2, {"x": torch.zeros(2, 4)}, layout="long")
    with pytest.raises(ValueError, match="2-D"):
        rt.window_batch(X[0], starts, host, 4, 2, 0, 2, {"x": torch.zeros(2, 4)})
    with pytest.raises(ValueError, match="layout"):
        rt.window_batch_form_of("long", 4, 4, 4)
    with pytest.raises(ValueError, match="not one of"):
        rt.window_batch_form_of("series", 4, 4, 4, outs=("z",))
    with pytest.raises(ValueError, match="misalign"):
        rt.window_batch_form_of("series", 4, 4, 4, outs=("x",), misalign={"y": 4})


def test_entry_rejects_bad_arguments_before_any_launch(ftn):
    """Every call below fails a host check; the device pointers are never dereferenced and nothing is enqueued, so
    the addresses need not be device memory."""
    lib = ftn.lib.load()
    Args = ftn.lib.FtnWindowArgs
    good = dict(X=0x10000, x_stride=8, M=0x20000, m_stride=8, marks=0x30000, marks_stride=3, statics=0x40000,
                ids=0x50000, starts=0x60000, T=40, item0=0, count=10, N=8, L=7, H=3, F=3, Fs=2, layout=0,
                x=0x100000, y=0x200000, mask=0x300000, x_mark=0x400000, y_mark=0x500000, static_out=0x600000,
                id_out=0x700000)

    def call(host=(0, 5, 30), entry=lib.ftn_window_batch, host_ptr=None, **change):
        a = Args()
        for k, v in {**good, **change}.items():
            setattr(a, k, v)
        arr = (C.c_int32 * max(len(host), 1))(*host)
        a.starts_host = (C.cast(arr, C.c_void_p).value if host else None) if host_ptr is None else host_ptr
        a.W = change.get("W", len(host))
        return entry(C.byref(a), None) if entry is lib.ftn_window_batch else entry(C.byref(a))

    form = lib.ftn_window_batch_form
    assert call(entry=form) == 64 << 8 | 32 << 16               # the good arguments pass the shared checks: scalar forms
    assert lib.ftn_window_batch(None, None) < 0 and form(None) < 0
    assert call(X=None) < 0 and call(starts=None) < 0 and call(host=()) < 0
    assert call(layout=2) < 0 and call(layout=-1) < 0
    assert call(N=0) < 0 and call(L=0) < 0 and call(H=0) < 0 and call(F=-1) < 0 and call(Fs=-1) < 0
    assert call(x_stride=7) < 0 and call(m_stride=7) < 0 and call(marks_stride=2) < 0
    assert call(marks=0x30000, F=0, x_mark=None, y_mark=None) < 0       # marks without features
    assert call(statics=0x40000, Fs=0, static_out=None) < 0
    assert call(marks=None, F=0) < 0 and call(marks=None, F=0, x_mark=None) < 0          # mark outputs without marks
    assert call(statics=None, Fs=0) < 0 and call(ids=None) < 0                           # static / id without tables
    assert call(layout=1, count=3) < 0                                                   # wide copies no statics, ids
    nothing = dict(x=None, y=None, mask=None, x_mark=None, y_mark=None, static_out=None, id_out=None)
    assert call(**nothing) < 0                                                           # no output
    assert call(count=0) < 0 and call(count=-1) < 0 and call(item0=-1) < 0
    assert call(item0=20, count=5) < 0 and call(item0=24, count=1) < 0 and call(count=25) < 0       # W N = 24 items
    assert call(layout=1, static_out=None, id_out=None, item0=2, count=2) < 0                        # W = 3 windows
    assert call(host=(0, 5, 31)) < 0 and call(host=(-1, 5, 30)) < 0 and call(T=39) < 0              # s + L + H <= T
    assert call(T=9) < 0 and call(W=0) < 0
    assert call(L=1 << 30, H=1 << 30) < 0 and call(L=1 << 27, N=16, x_stride=16, m_stride=16) < 0   # (L + H) N >= 2^31
    assert call(T=1 << 60, x_stride=1 << 20) < 0                                         # T x_stride beyond 64 bits
    for name in ("X", "M", "marks", "statics", "starts", "x", "y", "mask", "x_mark", "y_mark", "static_out"):
        assert call(**{name: good[name] + 2}) < 0, name                                  # 4-byte alignment
    assert call(ids=good["ids"] + 4) < 0 and call(id_out=good["id_out"] + 4) < 0         # 8-byte alignment
    assert b"ftn_window_batch" in lib.ftn_last_error()
    misaligned = (C.c_int32 * 4)(0, 5, 30, 0)
    assert call(host_ptr=C.addressof(misaligned) + 2) < 0
    assert call(entry=form, N=0) < 0 and call(entry=form, layout=3) < 0 and call(entry=form, x=good["x"] + 1) < 0
    assert b"ftn_window_batch_form" in lib.ftn_last_error()
