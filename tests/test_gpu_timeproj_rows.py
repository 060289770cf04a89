"""The row-mapped readers of a cached ``seq`` (``ftn_timeproj_forward_rows``, ``ftn_timeproj_wide_forward_rows``,
``ftn_timeproj_backward_rows``) and ``ftn_refit_rows_gather``.  The contract is addressing alone: a mapped call on the
store has the bits of the unmapped call on the gathered copy ``store[rows]``, so every comparison is ``torch.equal``.
Store rows a map does not name hold NaN, so a finite result also shows that only mapped rows were read; an index
outside the store is clamped, and the store of that test lies between two NaN rows the test owns."""
import pytest
import torch

import ws_poison

pytestmark = pytest.mark.gpu

N_ITEMS = 11


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _map(kind, B, n, seed=0):
    k = torch.arange(B)
    if kind == "identity":
        return k % n
    if kind == "reversed":
        return (n - 1 - k) % n
    if kind == "repeat":
        return torch.full((B,), 7 % n)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(40 + seed))
    return perm[k % n]


def _store(i, n, L, D, rows, dev):
    """``[n, L, D]`` of normal draws with NaN in every row ``rows`` does not name."""
    store = torch.randn(n, L, D, generator=torch.Generator().manual_seed(500 + i))
    named = torch.zeros(n, dtype=torch.bool)
    named[rows] = True
    store[~named] = float("nan")
    return store.to(dev)


def _wb(i, S, L, dev):
    """``weight[-S:]`` / ``bias[-S:]`` of a taller projection: 4 bytes off the grid when L is odd (WV off)."""
    g = torch.Generator().manual_seed(600 + i)
    w, b = torch.randn(S + 1, L, generator=g).to(dev), torch.randn(S + 1, generator=g).to(dev)
    return w[-S:], b[-S:]


SS, LS, DS, BS = [1, 7, 17, 40, 96], [4, 24, 33], [8, 64, 96], [1, 3, 11, 16]
KINDS = ["identity", "reversed", "repeat", "permutation"]
# every S, L, D, B and map appears, rotated against each other; then the wide entries
FWD = [(SS[i % 5], LS[i % 3], DS[(i // 2) % 3], BS[i % 4], KINDS[(i // 3) % 4]) for i in range(20)] + \
      [(17, 24, 136, 3, "permutation"), (96, 33, 136, 16, "reversed"), (1, 24, 512, 11, "identity"),
       (1, 33, 136, 3, "repeat"), (40, 4, 512, 1, "permutation")]


@pytest.mark.parametrize("i,S,L,D,B,kind", [(i,) + c for i, c in enumerate(FWD)])
def test_forward_rows_has_the_bits_of_the_gathered_copy(i, S, L, D, B, kind, ftn, dev):
    rt = ftn.runtime
    rows = _map(kind, B, N_ITEMS, i)
    store, (wt, bt) = _store(i, N_ITEMS, L, D, rows, dev), _wb(i, S, L, dev)
    r = rows.to(dev)
    got = rt.timeproj_forward(store, wt, bt, rows=r)
    copy = store[r].contiguous()
    want = rt.timeproj_forward(copy, wt, bt)
    assert got.shape == (B, S, D) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    assert torch.equal(rt.timeproj_forward(copy, wt, bt, rows=None), want)


def test_every_forward_form_ran(ftn):
    rt = ftn.runtime
    forms = {rt.timeproj_form_at(L, S, D, 0 if L % 4 == 0 else 4) for S, L, D, _, _ in FWD}
    assert forms == {"k_timeproj_row", "k_timeproj_row_wide"} | {
        f"k_timeproj_bf<{n},{w}>" for n in (1, 2, 4, 6) for w in ("true", "false")}, forms
    for k, axis in enumerate((SS, LS, DS, BS, KINDS)):
        assert set(axis) <= {c[k] for c in FWD}


BWD = [(64, 24, 7, 64, "permutation"), (1, 24, 4, 16, "identity"), (8, 33, 7, 64, "permutation"),
       (9, 4, 17, 96, "reversed"), (17, 24, 40, 8, "repeat"), (17, 33, 1, 136, "permutation"),
       (9, 24, 96, 512, "identity")]


def _backward_case(i, B, L, S, D, rows, n, ftn, dev):
    rt = ftn.runtime
    store = _store(100 + i, n, L, D, rows, dev)
    dh = torch.randn(B, S, D, generator=torch.Generator().manual_seed(700 + i)).to(dev)
    r = rows.to(dev)
    want = rt.timeproj_backward(store[r].contiguous(), dh)
    log = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(rt, "_workspace", ws_poison.poisoned_workspace(0xFF, log))
        buf_w = torch.full((S * L + 64,), float("nan"), device=dev)
        buf_b = torch.full((S + 64,), float("nan"), device=dev)
        snap_w, snap_b = buf_w.clone(), buf_b.clone()
        got = rt.timeproj_backward(store, dh, dw=buf_w[32:32 + S * L].view(S, L), db=buf_b[32:32 + S], rows=r)
        assert ws_poison.check_guards(log) == 1
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for buf, snap, k in ((buf_w, snap_w, S * L), (buf_b, snap_b, S)):
        assert torch.equal(buf[:32].view(torch.int32), snap[:32].view(torch.int32))
        assert torch.equal(buf[32 + k:].view(torch.int32), snap[32 + k:].view(torch.int32))


@pytest.mark.parametrize("i,B,L,S,D,kind", [(i,) + c for i, c in enumerate(BWD)])
def test_backward_rows_has_the_bits_of_the_gathered_copy(i, B, L, S, D, kind, ftn, dev):
    """B around the chunk of 8 (and 64: eight chunks, the walk that keeps a chunk on one XCD), from a NaN-poisoned
    workspace between guards, outputs between guarded bytes."""
    assert ftn.runtime.timeproj_backward_form_of(B, L, S, D)[1] == -(-B // 8)
    _backward_case(i, B, L, S, D, _map(kind, B, N_ITEMS, i), N_ITEMS, ftn, dev)


def test_backward_rows_where_the_chunk_grows(ftn, dev):
    """More than 256 chunks of 8: the chunk becomes 9 rows, 228 chunks, and the map still follows every step."""
    B = 2049
    assert ftn.runtime.timeproj_backward_form_of(B, 4, 1, 4)[1] == 228
    _backward_case(50, B, 4, 1, 4, torch.arange(B) % 5, 5, ftn, dev)


def test_indices_out_of_range_are_clamped_and_reported(ftn, dev):
    rt = ftn.runtime
    n, L, S, D = N_ITEMS, 24, 7, 64
    g = torch.Generator().manual_seed(9)
    buf = torch.randn(n + 2, L, D, generator=g).to(dev)
    buf[0] = buf[-1] = float("nan")                             # what an index that was not clamped would read
    store = buf[1:n + 1]
    assert store.is_contiguous() and store.data_ptr() % 16 == 0
    rows = torch.tensor([3, -1, n, 2 ** 40, 0, n - 1, -(2 ** 40), 5, 6], device=dev)
    clamped = rows.clamp(0, n - 1)
    wt, bt = _wb(0, S, L, dev)
    dh = torch.randn(rows.numel(), S, D, generator=g).to(dev)
    got, want = rt.timeproj_forward(store, wt, bt, rows=rows), rt.timeproj_forward(store, wt, bt, rows=clamped)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    assert torch.equal(want, rt.timeproj_forward(store[clamped].contiguous(), wt, bt))
    gb, wb = rt.timeproj_backward(store, dh, rows=rows), rt.timeproj_backward(store, dh, rows=clamped)
    assert bool(torch.isfinite(gb[0]).all()) and torch.equal(gb[0], wb[0]) and torch.equal(gb[1], wb[1])
    # S == 1: the row forms
    g1, w1 = (rt.timeproj_forward(store, wt[-1:], bt[-1:], rows=x) for x in (rows, clamped))
    assert bool(torch.isfinite(g1).all()) and torch.equal(g1, w1)
    tail, y = torch.randn(n, 2, 3, generator=g).to(dev), torch.randn(n, 4, 3, generator=g).to(dev)
    status = torch.full((1,), 77, dtype=torch.int32, device=dev)
    tb, yb, _, _, ok, st = rt.refit_rows_gather(rows, tail, y, status=status)
    assert st is status and int(status) == 4 and torch.equal(ok, clamped)
    assert torch.equal(tb, tail[clamped]) and torch.equal(yb, y[clamped])
    status.fill_(4)
    ok2 = rt.refit_rows_gather(clamped, tail, y, status=status)[4]
    assert int(status) == 0 and torch.equal(ok2, clamped)


@pytest.mark.parametrize("i,N,hist,with_mask,with_late,off", [
    (0, 1, 4, True, True, 32), (1, 1, 3, False, True, 32), (2, 5, 4, True, False, 32), (3, 5, 2, False, False, 32),
    (4, 4, 4, True, True, 33), (5, 5, 4, True, True, 33)])
def test_refit_rows_gather_is_index_select(i, N, hist, with_mask, with_late, off, ftn, dev):
    """Each output is ``index_select`` of its store, between guarded bytes; ``off`` = 33 puts the outputs 4 bytes off
    the 16-byte grid (rows that would take 16-byte accesses move float by float)."""
    rt = ftn.runtime
    n, S, B = N_ITEMS, 4, 9
    g = torch.Generator().manual_seed(800 + i)
    tail, y = torch.randn(n, hist, N, generator=g).to(dev), torch.randn(n, S, N, generator=g).to(dev)
    mask = (torch.rand(n, S, N, generator=g) >= 0.3).float().to(dev) if with_mask else None
    late = torch.randn(n, S, N, generator=g).to(dev) if with_late else None
    rows = _map("permutation", B, n, i).to(dev)
    stores = (tail, y, mask, late)
    bufs = [None if t is None else torch.full((B * t[0].numel() + 2 * off + 3,), float("nan"), device=dev)
            for t in stores]
    snaps = [None if b is None else b.clone() for b in bufs]
    out = [None if t is None else b[off:off + B * t[0].numel()].view(B, *t.shape[1:]) for t, b in zip(stores, bufs)]
    okbuf = torch.full((B + 8,), -7, dtype=torch.int64, device=dev)
    status = torch.full((3,), 9, dtype=torch.int32, device=dev)
    res = rt.refit_rows_gather(rows, tail, y, mask, late, out=out, rows_ok=okbuf[4:4 + B], status=status[1:2])
    for t, o, r, buf, snap in zip(stores, out, res[:4], bufs, snaps):
        if t is None:
            assert r is None
            continue
        k = B * t[0].numel()
        assert r is o and torch.equal(o, t.index_select(0, rows))
        assert torch.equal(buf[:off].view(torch.int32), snap[:off].view(torch.int32))
        assert torch.equal(buf[off + k:].view(torch.int32), snap[off + k:].view(torch.int32))
    assert torch.equal(okbuf[4:4 + B], rows) and bool((okbuf[:4] == -7).all()) and bool((okbuf[4 + B:] == -7).all())
    assert status.tolist() == [9, 0, 9]
