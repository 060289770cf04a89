"""Training windows without a GPU: the torch backend of ``windows.DeviceWindows(shuffle, drop_last, seed, augment)``
against the numpy restatement of the definitions (tests/train_windows_checks.py) and, for the shuffled batches,
against the reference loader's own rows (tests/golden/windows_cases.npz) picked by the order."""
import ctypes as C

import numpy as np
import pytest
import torch

import train_windows_checks as tc
import windows_checks as wc


@pytest.fixture(scope="module")
def fx():
    return wc.fixture()


def _concat(ftn, meta, arrays, case, layout="series", batch_size=None, **train):
    """``wc.build`` with the training arguments: through ``concat``'s overrides, which also covers one part."""
    w = wc.build(ftn, meta, arrays, case, layout=layout, batch_size=batch_size)
    return ftn.windows.DeviceWindows.concat([w], **train)


def _golden_rows(meta, arrays, case):
    m = meta[case]
    return [torch.from_numpy(np.concatenate([arrays[f"{case}:b{i}:{j}"] for i in range(m["batches"])]))
            for j in range(m["pieces"])]


def _np_batch(want):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in want]


def _fix_empty(want, B):
    return [a.reshape(B, 0) if a.size == 0 and a.ndim == 2 else a for a in want]


@pytest.mark.parametrize("n_items", [1, 2, 7, 40, 1000])
def test_order_is_the_restated_permutation(n_items, ftn):
    X = np.zeros((n_items + 2, 1), np.float32)                  # L = 2, H = 1: n_items windows of one series
    mk = lambda seed: ftn.windows.DeviceWindows(X, 2, 1, device="cpu", shuffle=True, seed=seed, batch_size=3)
    w = mk(5)
    assert w.n_items == n_items and w.epoch == 0
    got = w.order(epoch=3)
    assert got.dtype == torch.int64 and got.tolist() == tc.order(ftn, n_items, 5, 3).tolist()
    assert sorted(got.tolist()) == list(range(n_items))
    assert mk(5).order(epoch=3).tolist() == got.tolist()
    assert w.order(3) is got                                    # cached
    if n_items >= 7:
        assert w.order(epoch=4).tolist() != got.tolist() and mk(6).order(epoch=3).tolist() != got.tolist()
    assert ftn.windows.DeviceWindows(X, 2, 1, device="cpu", drop_last=True).order().tolist() == list(range(n_items))
    big = (1 << 63) + 12345                                     # both key words carry bits
    assert mk(big).order(epoch=(1 << 30) - 1).tolist() == tc.order(ftn, n_items, big, (1 << 30) - 1).tolist()


def test_order_sorts_the_keys_as_signed_integers(ftn):
    """The order walks the restated keys upwards as signed int64: it begins among the negative keys, which a sort of
    the same bit patterns as unsigned words would put last."""
    n = 4096
    w = ftn.windows.DeviceWindows(np.zeros((n + 2, 1), np.float32), 2, 1, device="cpu", shuffle=True, seed=9)
    k = tc.keys(ftn, n, 9, 2)
    x, y, _, _ = tc.philox_words(ftn, np.arange(n), 0, 2, 0, 9)
    assert k.view(np.uint64).tolist() == [(int(a) << 32) | int(b) for a, b in zip(x, y)]
    assert k.dtype == np.int64 and (k < 0).any() and (k > 0).any()
    walked = k[w.order(2).numpy()]
    assert (walked[1:] >= walked[:-1]).all() and walked[0] < 0 < walked[-1]
    assert w.order(2).tolist() != np.argsort(k.view(np.uint64), kind="stable").tolist()


@pytest.mark.parametrize("case", ["probe", "bare", "rec3", "concat"])
def test_shuffled_batches_are_the_loaders_rows_picked_by_the_order(case, ftn, fx):
    meta, arrays = fx
    rows = _golden_rows(meta, arrays, case)
    n = rows[0].shape[0]
    for bs in (1, 4, 7, n):
        for drop_last in (False, True):
            w = _concat(ftn, meta, arrays, case, batch_size=bs, shuffle=True, drop_last=drop_last, seed=11)
            assert w.backend == "torch" and w.n_items == n
            assert len(w) == (n // bs if drop_last else -(-n // bs))
            order = tc.order(ftn, n, 11, 2)
            assert w.order(2).tolist() == order.tolist()
            seen = []
            for i in range(len(w)):
                pick = torch.from_numpy(order[i * bs:(i + 1) * bs])
                want = [t[pick] for t in rows]
                got = w.batch(i, epoch=2)
                assert wc.batches_same(got, want), (case, bs, i)
                assert w._last_backend == "torch"
                seen += pick.tolist()
                if i in (0, len(w) - 1):
                    bufs = tuple(torch.full_like(t, 7) for t in want)
                    back = w.batch(i, out=bufs, epoch=2)
                    assert all(a is b for a, b in zip(back, bufs)) and wc.batches_same(back, want)
            if not drop_last:
                assert sorted(seen) == list(range(n))           # every item exactly once
            else:
                assert len(seen) == (n // bs) * bs and len(set(seen)) == len(seen)


@pytest.mark.parametrize("case", ["probe", "bare", "rec3", "concat"])
def test_wide_shuffled_batches_against_the_definition(case, ftn, fx):
    meta, arrays = fx
    if case == "concat":
        parts = tc.fixture_parts(arrays, meta, case)[:1]        # wide parts agree on N and carry no statics or ids
        for p in parts:
            p["static"] = p["ids"] = None
        parts = parts * 2
    else:
        parts = tc.fixture_parts(arrays, meta, case)
    DW = ftn.windows.DeviceWindows
    ws = [DW(p["X"], p["L"], p["H"], stride=p["stride"], valid_mask=p["M"], series_static=p["static"],
             series_ids=p["ids"], time_features=p["marks"], batch_size=3, layout="wide", device="cpu") for p in parts]
    n = ws[0].n_items * len(ws)
    order = tc.order(ftn, n, 4, 0)
    for bs in (1, 3, n):
        for drop_last in (False, True):
            w = DW.concat(ws, batch_size=bs, shuffle=True, drop_last=drop_last, seed=4)
            assert w.n_items == n and len(w) == (n // bs if drop_last else -(-n // bs))
            assert w.order(0).tolist() == order.tolist()
            seen = []
            for i in range(len(w)):
                pick = order[bs * i:bs * i + bs]
                want = _np_batch(_fix_empty(tc.expected(ftn, parts, "wide", pick)[0], len(pick)))
                assert wc.batches_same(w.batch(i, epoch=0), want), (case, bs, i)
                seen += pick.tolist()
                if i in (0, len(w) - 1):
                    n_own = 5                                   # the shared statics and ids are the tables themselves
                    bufs = tuple(torch.full_like(t, 7) for t in want[:n_own]) + tuple(want[n_own:])
                    back = w.batch(i, out=bufs, epoch=0)
                    assert all(a is b for a, b in zip(back[:n_own], bufs)) and wc.batches_same(back, want)
            if not drop_last:
                assert sorted(seen) == list(range(n))           # every item exactly once
            else:
                assert len(seen) == (n // bs) * bs and len(set(seen)) == len(seen)


@pytest.mark.parametrize("layout", ["series", "wide"])
@pytest.mark.parametrize("ts", [1, 2, 20])
def test_time_shift_moves_every_piece_of_an_item_together(ts, layout, ftn, fx):
    meta, arrays = fx
    parts = tc.fixture_parts(arrays, meta, "probe")
    T, L, H = parts[0]["X"].shape[0], parts[0]["L"], parts[0]["H"]
    assert T - L - H == 13
    w = _concat(ftn, meta, arrays, "probe", layout=layout, batch_size=4, shuffle=True, seed=3,
                augment={"time_shift": ts})
    n = w.n_items
    items = np.arange(n)
    want, _, starts = tc.expected(ftn, parts, layout, items, seed=3, epoch=1, ts=ts)
    plain, _, plain_starts = tc.expected(ftn, parts, layout, items)
    d = tc.delta(ftn, items, 3, 1, ts)
    assert d.min() >= -ts and d.max() <= ts and (starts != plain_starts).any()
    if ts == 20:                                                # the case cannot silently miss the clamps
        assert (plain_starts + d < 0).any() and (plain_starts + d > 13).any()
        assert (starts == 0).any() and (starts == 13).any()
    got = w.gather(items, epoch=1)
    assert wc.batches_same(got, _np_batch(_fix_empty(want, n)))
    X, marks = parts[0]["X"], parts[0]["marks"]
    M = parts[0]["M"]
    for r in (0, n // 2, n - 1):                                # x, y, mask and the marks share one start row
        s = int(starts[r])
        col = slice(r % X.shape[1], r % X.shape[1] + 1) if layout == "series" else slice(None)
        assert np.array_equal(got[0][r].numpy(), X[s:s + L, col], equal_nan=True)
        assert np.array_equal(got[1][r].numpy(), X[s + L:s + L + H, col], equal_nan=True)
        if M is not None:
            assert np.array_equal(got[2][r].numpy(), M[s + L:s + L + H, col])
        if marks is not None:
            assert np.array_equal(got[3][r].numpy(), marks[s:s + L]) and np.array_equal(got[4][r].numpy(),
                                                                                         marks[s + L:s + L + H])
    order = tc.order(ftn, n, 3, 1)                              # and the epoch's batches are those items in order
    b0 = w.batch(0, epoch=1)
    assert wc.batches_same(b0[:5], [t[torch.from_numpy(order[:4])] for t in got[:5]])


@pytest.mark.parametrize("layout", ["series", "wide"])
def test_noise_touches_x_only_and_equals_the_restatement(layout, ftn, fx):
    meta, arrays = fx
    parts = tc.fixture_parts(arrays, meta, "probe")
    sd = 0.25
    w = _concat(ftn, meta, arrays, "probe", layout=layout, batch_size=4, seed=8,
                augment={"add_noise_std": sd, "time_shift": 2})
    n = w.n_items
    items = np.arange(n)[::-1].copy()
    want, radius, _ = tc.expected(ftn, parts, layout, items, seed=8, epoch=5, ts=2, sd=sd)
    clean, _, _ = tc.expected(ftn, parts, layout, items, seed=8, epoch=5, ts=2)
    got = w.gather(items, epoch=5)
    assert wc.batches_same(got[1:], _np_batch(_fix_empty(want, n))[1:])          # y, mask, marks, statics, ids: copies
    x, xw, xc = got[0].numpy().astype(np.float64), want[0].astype(np.float64), clean[0].astype(np.float64)
    finite = np.isfinite(xc)
    bound = tc.spacing32(np.abs(xc[finite]) + sd * radius[finite])
    assert (np.abs(x[finite] - xw[finite]) <= bound).all()
    assert wc.same_bits(got[0], torch.from_numpy(want[0]))     # here both sides are numpy's fp64: equal
    assert (x[finite] != xc[finite]).mean() > 0.9
    again = w.gather(items[:3], epoch=5)                        # an item's bits do not depend on its batch or row
    assert wc.same_bits(again[0], got[0][:3])
    assert not wc.same_bits(w.gather(items[:3], epoch=6)[0], got[0][:3])


def test_noise_moments(ftn):
    T, N, L, H = 330, 4, 256, 1
    sd = 0.5
    w = ftn.windows.DeviceWindows(np.zeros((T, N), np.float32), L, H, device="cpu", batch_size=64, shuffle=True,
                                  seed=123, augment={"add_noise_std": sd})
    z = np.concatenate([b[0].numpy().reshape(-1) for b in w]).astype(np.float64) / sd
    n = z.size
    assert n >= 65536 and n == w.n_items * L
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    wide = ftn.windows.DeviceWindows(np.zeros((T, N), np.float32), L, H, device="cpu", batch_size=64, layout="wide",
                                     seed=123, augment={"add_noise_std": sd})
    z = np.concatenate([b[0].numpy().reshape(-1) for b in wide]).astype(np.float64) / sd
    n = z.size
    assert n >= 65536 and abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)


@pytest.mark.parametrize("layout", ["series", "wide"])
def test_zero_augment_is_the_plain_batch(layout, ftn, fx):
    meta, arrays = fx
    plain = wc.build(ftn, meta, arrays, "probe", layout=layout)
    w = _concat(ftn, meta, arrays, "probe", layout=layout, augment={"add_noise_std": 0.0, "time_shift": 0})
    assert not w._default and len(w) == len(plain)
    for i in range(len(plain)):
        assert wc.batches_same(w.batch(i), plain.batch(i))
    assert w.epoch == 0
    assert [wc.batches_same(a, b) for a, b in zip(w, plain)] == [True] * len(plain) and w.epoch == 1


def test_epochs_advance_with_iter_and_set_epoch_restores(ftn, fx):
    meta, arrays = fx
    w = _concat(ftn, meta, arrays, "probe", batch_size=4, shuffle=True, drop_last=True, seed=2,
                augment={"add_noise_std": 0.1, "time_shift": 1})
    assert w.epoch == 0
    it = iter(w)
    assert w.epoch == 1                                         # advanced when the iterator is created
    first = list(it)
    second = list(w)
    assert w.epoch == 2 and len(first) == len(second) == len(w)
    assert not all(wc.batches_same(a, b) for a, b in zip(first, second))
    assert w.order(0).tolist() != w.order(1).tolist()
    w.set_epoch(0)
    assert w.epoch == 0 and all(wc.batches_same(a, b) for a, b in zip(list(w), first))
    assert all(wc.batches_same(w.batch(i, epoch=1), b) for i, b in enumerate(second))


def test_argument_errors_come_before_any_work(ftn, fx):
    DW = ftn.windows.DeviceWindows
    X = np.zeros((12, 3), np.float32)
    for bad in ({"add_noise_std": -0.1}, {"time_shift": -1}, {"time_shift": 1 << 31}, {"noise": 1.0},
                {"add_noise_std": float("nan")}, {"add_noise_std": float("inf")}):
        with pytest.raises(ValueError):
            DW(None, 4, 2, device="cpu", augment=bad)           # the table is never looked at
    assert DW(X, 4, 2, device="cpu", augment={"time_shift": (1 << 31) - 1}).time_shift == (1 << 31) - 1
    w = DW(X, 4, 2, device="cpu", shuffle=True, batch_size=4)
    for bad in (-1, 1 << 30):
        with pytest.raises(ValueError, match="epoch"):
            w.set_epoch(bad)
        with pytest.raises(ValueError, match="epoch"):
            w.batch(0, epoch=bad)
        with pytest.raises(ValueError, match="epoch"):
            w.order(bad)
        with pytest.raises(ValueError, match="epoch"):
            w.gather([0], epoch=bad)
    assert w.epoch == 0
    for bad in ([-1], [w.n_items], [0, 1, 10 ** 12], torch.tensor([0, w.n_items])):
        with pytest.raises(ValueError, match="items"):
            w.gather(bad)
    with pytest.raises(ValueError):
        w.gather([])
    with pytest.raises(ValueError):
        w.gather([0.5])
    first = w.batch(0)
    with pytest.raises(ValueError, match="entries"):
        w.batch(0, out=first[:-1])
    with pytest.raises(ValueError, match=r"out\[0\]"):
        w.batch(0, out=(first[0][:, :-1],) + first[1:])
    with pytest.raises(ValueError, match=r"out\[1\]"):
        w.gather([0, 1, 2, 3], out=(first[0], first[1].double()) + first[2:])
    with pytest.raises(ValueError, match=r"out\[0\]"):
        w.gather([0, 1, 2], out=first)                          # three items into buffers of four rows
    with pytest.raises(ValueError):
        DW.concat([w], augment={"shift": 1})


def test_defaults_are_the_loader_of_today(ftn, fx):
    meta, arrays = fx
    for case in ("probe", "concat"):
        m = meta[case]
        w = wc.build(ftn, meta, arrays, case)
        assert w._default and not w.shuffle and not w.drop_last and w.seed == 0 and w.epoch == 0
        assert (w.time_shift, w.add_noise_std) == (0, 0.0)
        got = list(w)
        assert w.epoch == 0 and w._last_backend == "torch" and len(got) == m["batches"]
        for i, b in enumerate(got):
            assert wc.batches_same(b, [torch.from_numpy(arrays[f"{case}:b{i}:{j}"]) for j in range(m["pieces"])])
        again = ftn.windows.DeviceWindows.concat([w])
        assert again._default and wc.batches_same(again.batch(0), got[0])
        assert wc.batches_same(w.gather(range(m["batch"])), got[0])             # the primitive serves it too


def test_exports_and_entry_checks(ftn):
    L = ftn.lib
    assert {"ftn_window_gather", "ftn_epoch_keys"} <= set(L.EXPORTS) and L.ABI_VERSION == 14
    lib = L.load()
    assert lib.ftn_abi_version() == 14
    assert lib.ftn_epoch_keys(0, 1, 0, 0x1000, None) < 0 and lib.ftn_epoch_keys(4, 1, 1 << 30, 0x1000, None) < 0
    assert lib.ftn_epoch_keys(4, 1, 0, None, None) < 0 and lib.ftn_epoch_keys(4, 1, 0, 0x1004, None) < 0
    assert b"ftn_epoch_keys" in lib.ftn_last_error()
    good_w = dict(X=0x10000, x_stride=8, M=0x20000, m_stride=8, marks=0x30000, marks_stride=3, statics=0x40000,
                  ids=0x50000, starts=0x60000, T=40, item0=24, count=10, N=8, L=7, H=3, F=3, Fs=2, layout=0,
                  x=0x100000, y=0x200000, mask=0x300000, x_mark=0x400000, y_mark=0x500000, static_out=0x600000,
                  id_out=0x700000)
    good_g = dict(XT=0x800000, xt_stride=40, MT=0x900000, mt_stride=40, items=0xa00000, seed=1, noise_std=0.5,
                  epoch=3, ts=2)

    def call(host=(0, 5, 30), **change):
        g = L.FtnWindowGatherArgs()
        for k, v in {**good_w, **{k: v for k, v in change.items() if k in good_w}}.items():
            setattr(g.w, k, v)
        for k, v in {**good_g, **{k: v for k, v in change.items() if k in good_g}}.items():
            setattr(g, k, v)
        arr = (C.c_int32 * max(len(host), 1))(*host)
        g.w.starts_host = C.cast(arr, C.c_void_p).value if host else None
        g.w.W = len(host)
        return lib.ftn_window_gather(C.byref(g), None)

    assert lib.ftn_window_gather(None, None) < 0
    assert call(N=0) < 0 and call(layout=2) < 0 and call(x_stride=7) < 0 and call(X=None) < 0      # the shared checks
    assert call(host=(0, 5, 31)) < 0 and call(host=()) < 0 and call(T=9) < 0 and call(starts=None) < 0
    assert call(items=None) < 0 and call(items=0xa00004) < 0
    assert call(count=0) < 0 and call(item0=-1) < 0
    assert call(ts=-1) < 0 and call(noise_std=-0.5) < 0 and call(noise_std=float("nan")) < 0
    assert call(noise_std=float("inf")) < 0 and call(epoch=1 << 30) < 0
    assert call(XT=None) < 0 and call(xt_stride=39) < 0 and call(mt_stride=39) < 0 and call(XT=0x800002) < 0
    assert call(layout=1) < 0                                   # wide copies no statics and no ids
    assert b"ftn_window_gather" in lib.ftn_last_error()
