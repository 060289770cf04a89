"""Series groups along another axis, without a GPU: the torch backend of ``score.group_sums(..., axis=)`` bit for bit
against the numpy oracle on the moved axis, ``group_path_summary`` / ``group_path_metrics`` with the groups along the
batch axis against ``path_summary`` / ``path_metrics`` of the oracle's totals, the rejections, and every argument
error of ``ftn_group_sum_rows``, which the host checks before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import group_rows_checks as rc
import groups_checks as gc
import paths_checks as pc


def test_exports_and_abi(ftn):
    L = ftn.lib
    assert {"ftn_group_sum_rows", "ftn_group_sum_rows_form"} <= set(L.EXPORTS)
    assert L.ABI_VERSION == 14 and L.load().ftn_abi_version() == 14
    assert L.FTN_GROUP_TILE_COLS == 64


def _torch_sums(ftn, x, members, S, axis):
    sg = ftn.score.SeriesGroups.from_members(members, n_series=S)
    out = ftn.score.group_sums(torch.from_numpy(x), sg, axis=axis)
    assert ftn.score._last_backend == "torch" and out.dtype == torch.float32
    return out.numpy()


@pytest.mark.parametrize("S", rc.SS)
def test_torch_backend_with_axis_bit_equal_to_numpy(S, ftn):
    g = np.random.default_rng(140 + S)
    for name, members in gc.layouts(S).items():
        G = len(members)
        for shape, axis in (((3, S, 5), 1), ((S, 4), 0)):
            for kind, x in rc.values(g, shape, axis, members).items():
                want = rc.oracle(x, members, axis)
                got = _torch_sums(ftn, x, members, S, axis)
                assert got.shape == shape[:axis] + (G,) + shape[axis + 1:], (name, kind)
                assert gc.bits_equal(got, want), (name, kind, axis)
                assert gc.bits_equal(_torch_sums(ftn, x, members, S, axis - len(shape)), want), (name, kind, axis)


@pytest.mark.parametrize("S", rc.SS)
def test_the_last_axis_is_todays_result(S, ftn):
    g = np.random.default_rng(240 + S)
    members = gc.layouts(S)["overlap"]
    sg = ftn.score.SeriesGroups.from_members(members, n_series=S)
    for kind, x in gc.values(g, (3, 2, S), members).items():
        xt = torch.from_numpy(x)
        today = ftn.score.group_sums(xt, sg)
        assert gc.bits_equal(today.numpy(), gc.group_sum(x, members)), kind
        for axis in (-1, xt.dim() - 1):
            got = ftn.score.group_sums(xt, sg, axis=axis)
            assert gc.bits_equal(got.numpy(), today.numpy()), (kind, axis)
            assert gc.bits_equal(ftn.score.group_sums(xt, sg, None, axis).numpy(), today.numpy()), (kind, axis)


def _fixture_groups(ftn):
    ids, _ = gc.fixture()
    return ftn.score.SeriesGroups.from_ids(ids).with_total()


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_group_path_summary_and_metrics_along_the_batch_axis(reduce, ftn):
    sc = ftn.score
    sg = _fixture_groups(ftn)
    g = np.random.default_rng(19)
    P, B, H, N = 7, 193, 6, 1
    x, y = pc.counts(g, (P, B, H, N), 2.0), pc.counts(g, (B, H, N), 2.0)
    xt, yt = rc.oracle(x, sg.members, 1), rc.oracle(y, sg.members, 0)
    assert xt.shape == (P, 10, H, N) and yt.shape == (10, H, N)
    mask = np.ones((B, H, N), dtype=bool)
    member = sg.members[3][4]
    mask[member, 2, 0] = False                                  # one member row of store 3 (and of the total) at one step
    gmask = np.stack([mask[m].all(0) for m in sg.members], 0)
    assert gmask.shape == (10, H, N) and gmask.sum() == H * 10 - 2 and not gmask[3, 2, 0] and not gmask[9, 2, 0]
    for window in (None, 2, 6):
        for axis in (1, -3):
            got = sc.group_path_summary(torch.from_numpy(x), sg, pc.LEVELS, torch.from_numpy(y), window=window,
                                        reduce=reduce, want_sorted=True, axis=axis)
            want = sc.path_summary(torch.from_numpy(xt), pc.LEVELS, torch.from_numpy(yt), window=window,
                                   reduce=reduce, want_sorted=True)
            ora = pc.summary(xt, pc.LEVELS, window, reduce, yt)
            assert got["quantiles"].shape == (3, 10, H // (window or 1), N)
            for k in ("quantiles", "mean", "crps", "sorted"):
                assert torch.equal(got[k], want[k]), k
            assert pc.same(got["quantiles"].numpy(), ora["quantiles"])
            assert pc.same(got["sorted"].numpy(), ora["sorted"])
        for m, gm in ((None, None), (mask, gmask)):
            a = sc.group_path_metrics(torch.from_numpy(x), torch.from_numpy(y), sg, pc.LEVELS, window, reduce,
                                      None if m is None else torch.from_numpy(m), axis=1)
            b = sc.path_metrics(torch.from_numpy(xt), torch.from_numpy(yt), pc.LEVELS, window, reduce,
                                None if gm is None else torch.from_numpy(gm))
            for k in ("coverage", "pinball", "crps", "count"):
                assert torch.equal(a[k], b[k]), (k, window)
            w = window or 1
            expect = (H // w) * 10 - (0 if m is None else 2)
            assert int(a["count"]) == expect


def test_rejections(ftn):
    sc = ftn.score
    sg = sc.SeriesGroups.from_members([[0, 1]], n_series=3)
    for axis in (2, -3, 7):
        with pytest.raises(ValueError, match="axis"):
            sc.group_sums(torch.ones(3, 4), sg, axis=axis)
    with pytest.raises(ValueError, match="axis"):
        sc.group_sums(torch.ones(3, 4), sg, axis=0.0)
    with pytest.raises(ValueError, match="3 series"):
        sc.group_sums(torch.ones(4, 3), sg, axis=0)
    with pytest.raises(ValueError, match="3 series"):
        sc.group_sums(torch.ones(2, 4, 3), sg, axis=-2)
    with pytest.raises(ValueError, match="hip"):
        sc.group_sums(torch.ones(3, 4), sg, backend="hip", axis=0)                  # a CPU tensor
    x, y = torch.ones(2, 3, 4, 3), torch.ones(3, 4, 3)
    for fn, args in ((sc.group_path_summary, (x, sg, pc.LEVELS, y)), (sc.group_path_metrics, (x, y, sg, pc.LEVELS))):
        for axis in (0, 2, -2, -4, 4, None):
            with pytest.raises(ValueError, match="axis"):
                fn(*args, axis=axis)
        assert fn(*args, axis=1) is not None and fn(*args, axis=-3) is not None and fn(*args, axis=3) is not None
    with pytest.raises(ValueError, match="y must be"):
        sc.group_path_summary(x, sg, pc.LEVELS, torch.ones(3, 4), axis=1)
    with pytest.raises(ValueError, match="y must be"):
        sc.group_path_metrics(x, torch.ones(4, 3, 3), sg, pc.LEVELS, axis=1)
    with pytest.raises(ValueError, match="mask"):
        sc.group_path_metrics(x, y, sg, pc.LEVELS, mask=torch.ones(3, 4), axis=1)
    with pytest.raises(ValueError, match="samples"):
        sc.group_path_summary(x[0], sg, pc.LEVELS, axis=1)
    with pytest.raises(ValueError, match="3 series"):
        sc.group_path_summary(torch.ones(2, 4, 4, 3), sg, pc.LEVELS, axis=1)        # B is not n_series


def test_entry_rejects_bad_arguments_before_any_launch(ftn):
    """Every call below fails a host check; the device pointers are never dereferenced and nothing is enqueued, so
    the addresses need not be device memory."""
    lib = ftn.lib.load()
    X, ORD, OFF, OUT = 0x10000, 0x20000, 0x30000, 0x40000

    def call(x=X, outer=4, S=8, inner=5, ostride=48, mstride=6, order=ORD, off=OFF, host=(0, 3, 8), G=None, M=None,
             out=OUT, host_ptr=None):
        arr = (C.c_int * max(len(host), 1))(*host)
        hp = C.cast(arr, C.c_void_p).value if host_ptr is None else host_ptr
        return lib.ftn_group_sum_rows(x, outer, S, inner, ostride, mstride, order, off, hp if host else None,
                                      len(host) - 1 if G is None else G,
                                      host[-1] if M is None and host else (M or 0), out, None)

    assert call(x=None) < 0 and call(out=None) < 0 and call(off=None) < 0 and call(order=None) < 0
    assert call(host=()) < 0                                    # no host offsets
    assert call(x=X + 2) < 0 and call(out=OUT + 1) < 0 and call(order=ORD + 2) < 0 and call(off=OFF + 3) < 0
    assert call(inner=0) < 0 and call(S=0) < 0 and call(outer=0) < 0 and call(S=-1) < 0
    assert call(mstride=4) < 0                                  # member_stride < inner
    assert call(ostride=47) < 0                                 # outer_stride < S member_stride with outer > 1
    assert call(host=(0, 5, 3, 8)) < 0                          # not monotone
    assert call(host=(1, 3, 8)) < 0 and call(M=7) < 0 and call(M=9) < 0 and call(G=0) < 0 and call(G=2049) < 0
    assert call(host=tuple(range(0, 2050))) < 0                 # 2049 groups of one member: G and the chunks
    assert call(host=tuple(33 * i for i in range(1026))) < 0    # 1025 groups of 33: 2050 chunks
    assert call(outer=1 << 60, ostride=1 << 20) < 0             # outer * outer_stride beyond 64 bits
    assert call(S=(1 << 31) - 1, mstride=1 << 40, ostride=1 << 62) < 0              # S * member_stride beyond 64 bits
    assert call(outer=1 << 41, S=1, inner=1 << 20, mstride=1 << 20, ostride=1 << 20, host=(0, 1, 1)) < 0   # outer G inner
    assert b"ftn_group_sum_rows" in lib.ftn_last_error()
    misaligned = (C.c_int * 4)(0, 3, 8, 0)
    assert call(host_ptr=C.addressof(misaligned) + 2) < 0
