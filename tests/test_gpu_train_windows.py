"""Training windows on the MI355X (``ftn_window_gather`` and ``ftn_epoch_keys`` behind ``windows.DeviceWindows``): the
HIP backend bit for bit against the torch backend on the same device tensors - order, shuffled and time-shifted
batches - over N in {1, 3, 5, 64, 65} x L in {1, 7, 33} x H in {1, 3} x F in {0, 1, 3, 4} x Fs in {0, 2} in both
layouts, the four combinations of mask and ids rotating; a two-part concat, the short last batch, one item, a launch
past the grid limit, sliced tables; the noise against the fp64 restatement of tests/train_windows_checks.py; what a
launch must leave alone; the keys; and ``fit.refit_heads`` over a shuffled, augmented loader."""
import itertools

import numpy as np
import pytest
import torch

import train_windows_checks as tc
import windows_checks as wc

pytestmark = pytest.mark.gpu
POISON = 0x5A5AA5A5
GRID_N, GRID_L, GRID_H, GRID_F, GRID_FS = (1, 3, 5, 64, 65), (1, 7, 33), (1, 3), (0, 1, 3, 4), (0, 2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _tables(T, N, F, Fs, mask, ids, seed):
    g = np.random.default_rng(seed)
    t = {"X": g.standard_normal((T, N)).astype(np.float32), "M": None, "marks": None, "static": None, "ids": None}
    t["X"].reshape(-1).view(np.uint32)[:3] = (0x7FC00001, 0x80000000, 0xFF800000)[:min(3, T * N)]   # NaN payload, -0, -inf
    if mask:
        t["M"] = (g.random((T, N)) >= 0.3).astype(np.float32)
    if F:
        t["marks"] = g.standard_normal((T, F)).astype(np.float32)
    if Fs:
        t["static"] = g.standard_normal((N, Fs)).astype(np.float32)
    if ids:
        t["ids"] = (g.permutation(4 * N)[:N].astype(np.int64) << 33) + 7
    return t


def _on(dev, t):
    return {k: None if v is None else torch.from_numpy(v).to(dev) for k, v in t.items()}


def _windows(ftn, d, L, H, backend, layout="series", stride=1, **kw):
    return ftn.windows.DeviceWindows(d["X"], L, H, stride=stride, valid_mask=d["M"], series_static=d["static"],
                                     series_ids=d["ids"], time_features=d["marks"], layout=layout, backend=backend, **kw)


def _part(t, L, H, stride=1):
    return dict(t, L=L, H=H, stride=stride)


def _np_batch(want, B):
    return [torch.from_numpy(np.ascontiguousarray(a.reshape(B, 0) if a.size == 0 and a.ndim == 2 else a)) for a in want]


@pytest.mark.parametrize("N", GRID_N)
def test_grid_against_the_torch_backend(N, ftn, dev):
    compared, met = 0, set()
    for at, (L, H, F, Fs, layout) in enumerate(itertools.product(GRID_L, GRID_H, GRID_F, GRID_FS, ("series", "wide"))):
        iL, iH, iF, iFs = GRID_L.index(L), GRID_H.index(H), GRID_F.index(F), GRID_FS.index(Fs)
        combo = (iL + iH + iF + 2 * iFs) % 4                    # rotates independently of any one of L, H, F, Fs
        mask, ids = bool(combo & 1), bool(combo >> 1)
        met |= {(layout, "F", F, mask, ids), (layout, "Fs", Fs, mask, ids), (layout, "L", L, mask, ids),
                (layout, "H", H, mask, ids)}
        d = _on(dev, _tables(L + H + 6, N, F, Fs, mask, ids, 1000 * N + at))
        kw = dict(batch_size=4, shuffle=True, seed=77 + at, augment={"time_shift": 2})
        hip, ref = (_windows(ftn, d, L, H, b, layout, **kw) for b in ("hip", "torch"))
        assert hip.n_items == 7 * (N if layout == "series" else 1)
        order = hip.order(1)
        assert torch.equal(order, ref.order(1))
        for i in sorted({0, len(hip) - 1}):                     # the last batch is short where 4 does not divide
            got, want = hip.batch(i, epoch=1), ref.batch(i, epoch=1)
            assert hip._last_backend == "hip" and ref._last_backend == "torch"
            assert wc.batches_same(got, want), (N, L, H, F, Fs, layout, mask, ids, i)
            compared += 1
        assert wc.batches_same(hip.gather(order, epoch=1), ref.gather(order, epoch=1)), (N, L, H, F, Fs, layout)
    assert compared >= 96
    # every value of F, Fs, L and H met all four combinations of mask and ids in both layouts
    assert len(met) == 2 * 4 * (len(GRID_F) + len(GRID_FS) + len(GRID_L) + len(GRID_H))


def test_grid_shape_against_the_restatement(ftn, dev):
    """One grid shape per layout against the item-by-item numpy restatement, so the two backends cannot agree on a
    wrong shift; the restatement shows clamps at both ends."""
    L, H, N = 7, 3, 5
    t = _tables(L + H + 6, N, 3, 2, True, True, 5)
    for layout in ("series", "wide"):
        w = _windows(ftn, _on(dev, t), L, H, "hip", layout, batch_size=4, shuffle=True, seed=9, augment={"time_shift": 4})
        order = tc.order(ftn, w.n_items, 9, 2)
        assert w.order(2).tolist() == order.tolist()
        want, _, starts = tc.expected(ftn, [_part(t, L, H)], layout, order, seed=9, epoch=2, ts=4)
        assert (starts == 0).any() and (starts == 6).any()
        assert wc.batches_same(w.gather(order, epoch=2), _np_batch(want, len(order)))


def test_concat_batches_straddle_the_parts(ftn, dev):
    L, H = 7, 3
    ta, tb = _tables(14, 5, 3, 2, True, True, 1), _tables(17, 3, 3, 2, True, True, 2)
    for kw in (dict(shuffle=True, seed=5, augment={"time_shift": 1}), dict(drop_last=True)):
        made = {}
        for b in ("hip", "torch"):
            ws = [_windows(ftn, _on(dev, t), L, H, b, batch_size=8) for t in (ta, tb)]
            made[b] = ftn.windows.DeviceWindows.concat(ws, **kw)
        hip, ref = made["hip"], made["torch"]
        assert hip.n_items == 5 * 5 + 8 * 3 and hip.backend == "hip"
        order = hip.order(3).tolist()
        straddle = 0
        for i in range(len(hip)):
            got = hip.batch(i, epoch=3)
            assert wc.batches_same(got, ref.batch(i, epoch=3)), (kw, i)
            picked = order[8 * i:8 * i + 8]
            straddle += min(picked) < 25 <= max(picked)
            want, _, _ = tc.expected(ftn, [_part(ta, L, H), _part(tb, L, H)], "series", picked, seed=kw.get("seed", 0),
                                     epoch=3, ts=1 if "augment" in kw else 0)
            assert wc.batches_same(got, _np_batch(want, len(picked))), (kw, i)
        assert straddle >= 1 and len(hip) == (49 // 8 if "drop_last" in kw else 7)


def test_one_item_and_the_short_last_batch(ftn, dev):
    t = _tables(20, 3, 1, 0, False, True, 3)
    d = _on(dev, t)
    for layout in ("series", "wide"):
        for bs in (1, 5):
            hip, ref = (_windows(ftn, d, 7, 1, b, layout, batch_size=bs, shuffle=True, seed=1,
                                 augment={"time_shift": 3}) for b in ("hip", "torch"))
            n = hip.n_items
            for i in (0, len(hip) - 1):
                got = hip.batch(i)
                assert got[0].shape[0] == (bs if i == 0 else n - (len(hip) - 1) * bs)
                assert wc.batches_same(got, ref.batch(i)), (layout, bs, i)
        assert wc.batches_same(hip.gather([n - 1]), ref.gather([n - 1]))
        assert hip.gather([0])[0].shape[0] == 1


def test_a_launch_beyond_the_grid_limit(ftn, dev):
    """30 000 shuffled items of 185 words in one launch: more than 4096 units of 1024 words, count L > 4096 * 1024 / 8."""
    L, H, N = 33, 3, 7
    t = _tables(4330, N, 4, 0, True, True, 4)
    d = _on(dev, t)
    kw = dict(batch_size=30_000, shuffle=True, drop_last=True, seed=2, augment={"time_shift": 5})
    hip, ref = (_windows(ftn, d, L, H, b, **kw) for b in ("hip", "torch"))
    assert hip.n_items >= 30_000 and len(hip) == 1 and 30_000 * L > 4096 * 1024 // 8
    assert 30_000 * (L + 2 * H + (L + H) * 4 + 2) > 4096 * 1024
    got = hip.batch(0)
    assert got[0].shape == (30_000, L, 1) and wc.batches_same(got, ref.batch(0))


def test_row_and_column_slices(ftn, dev):
    L, H, N, T = 7, 3, 5, 16
    for layout in ("series", "wide"):
        t = _tables(T, N, 3, 0, True, False, 6)
        d = _on(dev, t)
        for name, cols in (("X", N), ("M", N), ("marks", 3)):
            big = torch.full((T + 5, cols + 3), 9.0, device=dev)
            big[3:3 + T, 2:2 + cols] = d[name]
            d[name] = big[3:3 + T, 2:2 + cols]                  # a row slice and a column slice at once
            assert d[name].stride(0) == cols + 3 and not d[name].is_contiguous()
        hip = _windows(ftn, d, L, H, "hip", layout, batch_size=4, shuffle=True, seed=3, augment={"time_shift": 2})
        order = tc.order(ftn, hip.n_items, 3, 0)
        want, _, _ = tc.expected(ftn, [_part(t, L, H)], layout, order, seed=3, epoch=0, ts=2)
        assert wc.batches_same(hip.gather(order, epoch=0), _np_batch(want, len(order)))


def test_refresh_drops_the_series_major_snapshot(ftn, dev):
    t = _tables(16, 5, 0, 0, True, False, 7)
    d = _on(dev, t)
    kw = dict(batch_size=4, shuffle=True, seed=3, augment={"time_shift": 1})
    hip, ref = (_windows(ftn, d, 7, 3, b, **kw) for b in ("hip", "torch"))
    before = hip.batch(0, epoch=0)
    assert wc.batches_same(before, ref.batch(0, epoch=0))
    d["X"].add_(1.0)                                            # the table changes in place
    d["M"].fill_(0.0)
    assert wc.batches_same(hip.batch(0, epoch=0)[:3], before[:3])       # the snapshot: x, y, mask as they were
    hip.refresh()
    after = hip.batch(0, epoch=0)
    assert wc.batches_same(after, ref.batch(0, epoch=0)) and not wc.same_bits(after[0], before[0])


@pytest.mark.parametrize("layout", ["series", "wide"])
def test_noise_against_the_fp64_restatement(layout, ftn, dev):
    L, H, N, sd = 33, 3, 5, 0.25
    t = _tables(L + H + 6, N, 3, 2, True, True, 8)
    t["X"] = np.nan_to_num(t["X"], nan=1.5, neginf=-2.0)
    w = _windows(ftn, _on(dev, t), L, H, "hip", layout, batch_size=4, shuffle=True, seed=21,
                 augment={"add_noise_std": sd, "time_shift": 2})
    n = w.n_items
    items = tc.order(ftn, n, 21, 4)
    want, radius, _ = tc.expected(ftn, [_part(t, L, H)], layout, items, seed=21, epoch=4, ts=2, sd=sd)
    clean, _, _ = tc.expected(ftn, [_part(t, L, H)], layout, items, seed=21, epoch=4, ts=2)
    got = w.gather(items, epoch=4)
    assert w._last_backend == "hip"
    assert wc.batches_same(got[1:], _np_batch(want, n)[1:])     # y, mask, marks, statics, ids: bit copies
    x, xw, xc = (a.astype(np.float64) for a in (got[0].cpu().numpy(), want[0], clean[0]))
    err, bound = np.abs(x - xw), tc.spacing32(np.abs(xc) + sd * radius)
    print(f"TRAIN_WIN noise {layout}: {int((err > 0).sum())} of {err.size} elements differ from numpy's fp64 by one "
          f"fp32 place, largest fraction of the bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all() and (x != xc).mean() > 0.9
    a = w.gather(items[:7], epoch=4)[0]                         # the same item in another batch and another row
    b = w.gather(np.concatenate([items[5:7], items[:5], items[20:23]]), epoch=4)[0]
    assert wc.same_bits(a, got[0][:7]) and wc.same_bits(b[2:7], got[0][:5]) and wc.same_bits(b[:2], got[0][5:7])
    assert wc.batches_same(w.batch(1, epoch=4)[:1], [got[0][4:8]])
    zero = _windows(ftn, _on(dev, t), L, H, "hip", layout, batch_size=4, shuffle=True, seed=21,
                    augment={"add_noise_std": 0.0, "time_shift": 2})
    assert wc.batches_same(zero.gather(items, epoch=4), _np_batch(clean, n))      # sd = 0: a bit copy


def _carve(buf, at, like):
    words = like.numel() * (2 if like.dtype == torch.int64 else 1)
    return buf[at:at + words].view(like.dtype).view(like.shape), at + words


@pytest.mark.parametrize("layout", ["series", "wide"])
def test_a_launch_leaves_everything_else_alone(layout, ftn, dev):
    """Outputs carved out of a poisoned buffer with guard words around each, three more rows behind each (a longer
    ``out``), and - for a launch over the first part of a concat alone - the rows of the other part's items."""
    L, H, N = 7, 3, 5
    wide = layout == "wide"
    ta = _tables(14, N, 3, 0 if wide else 2, True, not wide, 1)
    tb = _tables(17, N, 3, 0 if wide else 2, True, not wide, 2)
    ws = [_windows(ftn, _on(dev, t), L, H, "hip", layout, batch_size=6) for t in (ta, tb)]
    both = ftn.windows.DeviceWindows.concat(ws, shuffle=True, seed=6, augment={"time_shift": 1, "add_noise_std": 0.5})
    order = both.order(0)
    n0 = ws[0].n_items
    for i in range(len(both)):
        want = both.batch(i, epoch=0)
        B = want[0].shape[0]
        buf = torch.full((sum(2 * p.numel() + 8 * (p.numel() // B) + 16 for p in want) + 64,), POISON,
                         dtype=torch.int32, device=dev)
        carved, spans, pos = [], [], 5
        for p in want:
            pos += pos % 2 if p.dtype == torch.int64 else 0
            v, end = _carve(buf, pos, p)
            carved.append(v if p.numel() else None)
            spans.append((pos, end))
            pos = end + 3 * (p.numel() // B) * (2 if p.dtype == torch.int64 else 1) + 3     # three rows and guards
        got = both.batch(i, out=tuple(carved), epoch=0)
        assert wc.batches_same(got, want)
        keep = torch.ones_like(buf, dtype=torch.bool)
        for a, b in spans:
            keep[a:b] = False
        assert bool((buf[keep] == POISON).all()), (layout, i)
        # one part's launch: the other part's rows keep the poison
        p = both._parts[0]
        items = order[6 * i:6 * i + B].contiguous()
        mine = (items < n0).cpu()
        names = ["x", "y", "mask", "x_mark", "y_mark"] + ([] if wide else ["static", "id"])
        rows = {}
        for name, like in zip(names, want):
            fill = torch.full((like.numel() * (2 if like.dtype == torch.int64 else 1),), POISON, dtype=torch.int32,
                              device=dev)
            rows[name] = fill.view(like.dtype).view(like.shape)
        XT, MT = p.series_major() if not wide else (None, None)
        ftn.runtime.window_gather(p.X, p.starts, p.starts_host, L, H, 0, items, rows, XT=XT, M=p.M, MT=MT, marks=p.marks,
                                  statics=None if wide else p.statics, ids=None if wide else p.ids, layout=layout,
                                  time_shift=1, noise_std=0.5, seed=6, epoch=0)
        for name, like in zip(names, want):
            words = rows[name].reshape(B, -1).view(torch.int32).cpu()
            assert bool((words[~mine] == POISON).all()), (layout, i, name)
            assert wc.same_bits(rows[name][mine.to(dev)], like[mine.to(dev)]), (layout, i, name)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100_000])
def test_epoch_keys_equal_the_restatement(n, ftn, dev):
    for seed, epoch in ((0, 0), ((1 << 63) + 5, (1 << 30) - 1)):
        keys = ftn.runtime.epoch_keys(n, seed, epoch, dev)
        assert keys.dtype == torch.int64 and keys.cpu().numpy().tolist() == tc.keys(ftn, n, seed, epoch).tolist()
    with pytest.raises(ValueError, match="epoch"):
        ftn.runtime.epoch_keys(n, 0, 1 << 30, dev)


def test_refit_heads_over_shuffled_augmented_windows(ftn, dev):
    L, H, N, T = 24, 4, 5, 40
    cfg = dict(input_len=L, pred_len=H, d_model=16, d_ff=32, n_layers=2, k_periods=3, kernel_set=[(3, 3), (5, 5)],
               dropout=0.0, activation="gelu", mode="direct", use_checkpoint=False)
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(0)
    model = ftn.models.TimesNet(**cfg).eval()
    with torch.no_grad():
        model(torch.rand(2, L, N, generator=g) + 1.0)
        for p in model.parameters():
            if float(p.abs().sum()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    model = model.to(dev)
    t = torch.arange(T, dtype=torch.float32).view(T, 1)
    X = torch.poisson(2.0 + 1.5 * torch.sin(2 * torch.pi * t / 6.0) + torch.rand(T, N, generator=g), generator=g)
    M = (torch.rand(T, N, generator=g) >= 0.2).float()
    w = ftn.windows.DeviceWindows(X, L, H, valid_mask=M, batch_size=4, layout="wide", device=dev, shuffle=True,
                                  drop_last=True, seed=3, augment={"add_noise_std": 0.05, "time_shift": 1})
    assert w.backend == "hip" and len(w) == 3 and w.epoch == 0
    losses = ftn.fit.refit_heads(model, w, epochs=2, lr=1e-2, use_loss_mask=True)
    assert losses.shape == (2 * len(w),) and bool(torch.isfinite(losses).all())
    assert w.epoch == 2 and w._last_backend == "hip"
