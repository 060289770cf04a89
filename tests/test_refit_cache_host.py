"""The cached refit on the host (no GPU): ``fit.time_projection(rows=)`` against the ``index_select`` composition and
torch autograd to the bit, ``fit.OutputCache`` / ``fit.refit_output_cached(graphed=False)`` on a CPU model against
``fit.refit_output`` with a torch-backend ``DeviceAdamW``, the ValueErrors, ``bytes_needed``, and the argument checks
of the four new entry points (nothing here reaches a launch)."""
import copy

import pytest
import torch

from test_output_fit_host import H, L, OUT, _tiny


def _windows(ftn, N, layout, T=40, batch_size=4, **kw):
    g = torch.Generator().manual_seed(11 + N)
    t = torch.arange(T, dtype=torch.float32).view(T, 1)
    table = torch.poisson(2.0 + torch.sin(2 * torch.pi * t / 6.0) + torch.rand(T, N, generator=g), generator=g)
    valid = (torch.rand(T, N, generator=g) >= 0.2).float()
    return ftn.windows.DeviceWindows(table, L, H, valid_mask=valid, batch_size=batch_size, layout=layout,
                                     device="cpu", **kw)


def test_time_projection_rows_is_the_index_select_composition(ftn):
    fit = ftn.fit
    g = torch.Generator().manual_seed(5)
    store = torch.randn(7, 6, 8, generator=g)
    w, b = torch.randn(3, 6, generator=g).requires_grad_(), torch.randn(3, generator=g).requires_grad_()
    rows = torch.tensor([6, 0, 0, 3, 5])
    fit._last_timeproj_backend = None
    got = fit.time_projection(store, w, b, rows=rows)
    assert fit._last_timeproj_backend == "torch" and got.shape == (5, 3, 8)
    want = torch.matmul(w, store.index_select(0, rows)) + b.view(1, -1, 1)
    assert torch.equal(got, want)
    cot = torch.randn(5, 3, 8, generator=g)
    assert all(torch.equal(a, c) for a, c in zip(torch.autograd.grad(got, [w, b], cot),
                                                 torch.autograd.grad(want, [w, b], cot)))
    assert torch.equal(fit.time_projection(store, w, b), torch.matmul(w, store) + b.view(1, -1, 1))
    for bad in (rows.float(), rows.view(1, -1), rows[:0], [0, 1]):
        with pytest.raises(ValueError, match="rows must be an int64 vector"):
            fit.time_projection(store, w, b, rows=bad)


def _six_state(model):
    return {k: v.clone() for k, v in model.state_dict().items() if k.startswith(OUT)}


@pytest.mark.parametrize("N,layout,T", [(5, "wide", 40), (1, "series", 38)])
def test_cached_refit_equals_refit_output_on_the_cpu(N, layout, T, ftn):
    """``shuffle=False``: batch i of an epoch is canonical batch i, so the cached loop repeats ``refit_output``'s
    operands and, with the same torch-backend ``DeviceAdamW``, its bits - the short last batch included."""
    fit = ftn.fit
    model, _ = _tiny(ftn, N)
    win = _windows(ftn, N, layout, T=T)
    assert win.n_items % win.batch_size != 0
    model.output_inputs(win.batch(0)[0])                            # builds the lazy layers for these windows
    twin = copy.deepcopy(model)
    cache = fit.OutputCache(model, win, use_loss_mask=True)
    assert cache.seq.shape == (win.n_items, L, 16) and cache.tail.shape == (win.n_items, H, N if layout == "wide" else 1)
    assert fit.OutputCache.bytes_needed(model, win, True) == cache.nbytes == sum(
        t.numel() * 4 for t in (cache.seq, cache.tail, cache.y, cache.mask, cache.late) if t is not None)
    assert fit.OutputCache.bytes_needed(model, win, False) == cache.nbytes - cache.mask.numel() * 4
    for i in range(len(win)):
        k0, k1 = i * 4, min(i * 4 + 4, win.n_items)
        x, yb, mk = win.batch(i)[:3]
        seq, tail, hist, late, floor = model.output_inputs(x)
        assert torch.equal(cache.seq[k0:k1], seq) and torch.equal(cache.tail[k0:k1], tail) and hist == cache.hist
        assert torch.equal(cache.y[k0:k1], yb) and torch.equal(cache.mask[k0:k1], (mk > 0).float())
        assert (late is None) == (cache.late is None)
    flags = [p.requires_grad for p in model.parameters()]
    got = fit.refit_output_cached(model, win, epochs=2, lr=[1e-2, 5e-3], weight_decay=0.01, grad_clip=0.05,
                                  use_loss_mask=True, cache=cache, graphed=False)
    assert fit._last_optim_backend == "torch" and fit._last_timeproj_backend == "torch"
    assert [p.requires_grad for p in model.parameters()] == flags and not model.training
    six = ftn.fit._refit_params(twin)
    opt, want = fit.DeviceAdamW(six, weight_decay=0.01, max_norm=0.05, backend="torch"), []
    for lr in (1e-2, 5e-3):
        opt.set_lr(lr)
        want.append(fit.refit_output(twin, win, epochs=1, use_loss_mask=True, optimizer=opt))
    assert torch.equal(got, torch.cat(want)) and got.shape == (2 * len(win),)
    a, b = _six_state(model), _six_state(twin)
    assert all(torch.equal(a[k], b[k]) for k in a)
    cache.check(model)                                              # the six tensors moved: the cache stands
    with torch.no_grad():
        next(p for n_, p in model.named_parameters() if not n_.startswith(OUT)).mul_(1.0)
    with pytest.raises(ValueError, match="the backbone changed since the cache was filled"):
        cache.check(model)


def test_the_value_errors(ftn):
    fit = ftn.fit
    model, _ = _tiny(ftn, 5)
    win = _windows(ftn, 5, "wide")
    for aug in ({"time_shift": 2}, {"add_noise_std": 0.1}):
        with pytest.raises(ValueError, match="differ per epoch and have no cache"):
            fit.OutputCache(model, _windows(ftn, 5, "wide", shuffle=True, augment=aug))
    need = fit.OutputCache.bytes_needed(model, win)
    with pytest.raises(ValueError, match=f"need {need} bytes, max_bytes is {need - 1}"):
        fit.OutputCache(model, win, max_bytes=need - 1)
    cache = fit.OutputCache(model, win, max_bytes=need)
    with pytest.raises(ValueError, match="filled from other windows"):
        fit.refit_output_cached(model, _windows(ftn, 5, "wide"), cache=cache, graphed=False)
    with pytest.raises(ValueError, match="2 learning rates for 3 epochs"):
        fit.refit_output_cached(model, win, epochs=3, lr=[1e-3, 1e-3], cache=cache, graphed=False)
    with pytest.raises(ValueError, match="needs a cache filled with use_loss_mask"):
        fit.refit_output_cached(model, win, use_loss_mask=True, cache=cache, graphed=False)


def test_shuffled_epochs_advance_the_windows(ftn):
    """A training loader: the orders are those ``iter(windows)`` would have drawn, and ``drop_last`` is honoured."""
    fit = ftn.fit
    model, _ = _tiny(ftn, 5)
    win = _windows(ftn, 5, "wide", shuffle=True, drop_last=True, seed=3)
    assert win.n_items == 13 and len(win) == 3
    losses = fit.refit_output_cached(model, win, epochs=2, graphed=False)
    assert losses.shape == (6,) and win.epoch == 2 and bool(torch.isfinite(losses).all())


A, M = 0x10000, 0x10004          # stand-ins for device addresses: 16-byte aligned / 4 bytes past a boundary
FWD = dict(seq=A, n=11, rows=A, B=2, L=24, D=64, wt=A, bt=A, S=4, hid=A)
FWD_BAD = {"null rows": dict(rows=None), "rows off by 4": dict(rows=M), "n_items = 0": dict(n=0),
           "null seq": dict(seq=None), "B = 0": dict(B=0), "S = 0": dict(S=0), "D % 4": dict(D=66),
           "seq misaligned": dict(seq=M), "hidden misaligned": dict(hid=M)}


@pytest.mark.parametrize("name", list(FWD_BAD))
@pytest.mark.parametrize("entry,D", [("ftn_timeproj_forward_rows", 64), ("ftn_timeproj_wide_forward_rows", 256)])
def test_forward_rows_rejects_bad_arguments_before_any_launch(entry, D, name, ftn):
    lib = ftn.lib.load()
    a = {**FWD, "D": D, **FWD_BAD[name]}
    assert lib.ftn_timeproj_form(24, 4, 64, 0) > 0                      # leaves an earlier message out of the way
    rc = getattr(lib, entry)(a["seq"], a["n"], a["rows"], a["B"], a["L"], a["D"], a["wt"], a["bt"], a["S"], a["hid"],
                             None)
    assert rc != 0 and lib.ftn_last_error().decode().startswith(entry), lib.ftn_last_error()
    with pytest.raises(ValueError, match=entry):
        ftn.lib.check(rc, entry)


def test_the_widths_keep_their_ranges(ftn):
    lib = ftn.lib.load()
    assert lib.ftn_timeproj_forward_rows(A, 3, A, 2, 24, 132, A, A, 4, A, None) != 0
    assert lib.ftn_last_error().decode().startswith("ftn_timeproj_forward_rows")
    assert lib.ftn_timeproj_wide_forward_rows(A, 3, A, 2, 24, 128, A, A, 4, A, None) != 0
    assert lib.ftn_last_error().decode().startswith("ftn_timeproj_wide_forward_rows")


BWD = dict(seq=A, n=11, rows=A, dh=A, B=9, L=24, S=4, D=64, dw=A, db=A, ws=A, bytes=1 << 20)
BWD_BAD = {"null rows": dict(rows=None), "rows off by 4": dict(rows=M), "n_items = 0": dict(n=0),
           "null d_hidden": dict(dh=None), "B = 0": dict(B=0), "D % 4": dict(D=66), "D > 512": dict(D=516),
           "seq misaligned": dict(seq=M), "d_hidden misaligned": dict(dh=M), "workspace too small": dict(bytes=16)}


@pytest.mark.parametrize("name", list(BWD_BAD))
def test_backward_rows_rejects_bad_arguments_before_any_launch(name, ftn):
    lib = ftn.lib.load()
    a = {**BWD, **BWD_BAD[name]}
    assert lib.ftn_timeproj_form(24, 4, 64, 0) > 0
    rc = lib.ftn_timeproj_backward_rows(a["seq"], a["n"], a["rows"], a["dh"], a["B"], a["L"], a["S"], a["D"], a["dw"],
                                        a["db"], a["ws"], a["bytes"], None)
    assert rc != 0 and lib.ftn_last_error().decode().startswith("ftn_timeproj_backward_rows"), lib.ftn_last_error()


GAT = dict(rows=A, B=4, n=11, tail=A, tf=4, y=A, mask=None, late=None, rf=4, to=A, yo=A, mo=None, lo=None,
           ok=A + 0x1000, st=A)
GAT_BAD = {"null rows": dict(rows=None), "null status": dict(st=None), "null rows_ok": dict(ok=None),
           "n_items = 0": dict(n=0), "B = 0": dict(B=0), "rows off by 4": dict(rows=M), "rows_ok over rows": dict(ok=A + 8),
           "a mask store without an output": dict(mask=A), "a late output without a store": dict(lo=A),
           "tail longer than a row": dict(tf=8), "y off by 2": dict(y=A + 2)}


@pytest.mark.parametrize("name", list(GAT_BAD))
def test_gather_rejects_bad_arguments_before_any_launch(name, ftn):
    lib = ftn.lib.load()
    a = {**GAT, **GAT_BAD[name]}
    assert lib.ftn_timeproj_form(24, 4, 64, 0) > 0
    rc = lib.ftn_refit_rows_gather(a["rows"], a["B"], a["n"], a["tail"], a["tf"], a["y"], a["mask"], a["late"], a["rf"],
                                   a["to"], a["yo"], a["mo"], a["lo"], a["ok"], a["st"], None)
    assert rc != 0 and lib.ftn_last_error().decode().startswith("ftn_refit_rows_gather"), lib.ftn_last_error()


def test_exports_and_abi(ftn):
    assert {"ftn_timeproj_forward_rows", "ftn_timeproj_wide_forward_rows", "ftn_timeproj_backward_rows",
            "ftn_refit_rows_gather"} <= set(ftn.lib.EXPORTS)
    assert ftn.lib.load().ftn_abi_version() == 14


def test_wrappers_validate_on_the_host(ftn):
    rt = ftn.runtime
    seq, wt, bt = torch.zeros(5, 24, 64), torch.zeros(4, 24), torch.zeros(4)
    with pytest.raises(ValueError, match="rows must be a contiguous int64 vector"):
        rt.timeproj_forward(seq, wt, bt, rows=torch.zeros(3))
    with pytest.raises(ValueError, match="device"):
        rt.timeproj_forward(seq, wt, bt, rows=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="rows \\[B\\]"):
        rt.timeproj_backward(seq, torch.zeros(2, 4, 64), rows=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="tail \\[n_items, hist, N\\]"):
        rt.refit_rows_gather(torch.zeros(3, dtype=torch.int64), torch.zeros(5, 4, 2), torch.zeros(6, 4, 2))
