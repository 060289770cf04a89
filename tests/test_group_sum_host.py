"""Series groups without a GPU: ``score.SeriesGroups`` on the fixture of tests/golden/series_ids.json and on every
constructor and rejection, the torch backend of ``score.group_sums`` bit for bit against the numpy oracle of
tests/groups_checks.py, ``group_path_summary`` / ``group_path_metrics`` against ``path_summary`` / ``path_metrics`` of
the oracle's totals, and every argument error of ``ftn_group_sum``, which the host checks before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import groups_checks as gc
import paths_checks as pc


def test_exports_and_abi(ftn):
    L = ftn.lib
    assert {"ftn_group_sum", "ftn_group_sum_form"} <= set(L.EXPORTS)
    assert L.ABI_VERSION == 14 and L.load().ftn_abi_version() == 14
    assert (L.FTN_GROUP_CHUNK, L.FTN_GROUP_NMAX, L.FTN_GROUP_GMAX, L.FTN_GROUP_CHUNKS_MAX) == (32, 8192, 2048, 2048)
    sc = ftn.score
    assert (sc.GROUP_CHUNK, sc.GROUP_NMAX, sc.GROUP_GMAX, sc.GROUP_CHUNKS_MAX) == (32, 8192, 2048, 2048)


def test_from_ids_gives_the_recorded_stores(ftn):
    ids, stores = gc.fixture()
    assert len(ids) == 193 and len(stores) == 9 and max(n for _, n in stores) > 32
    sg = ftn.score.SeriesGroups.from_ids(ids)
    assert sg.names == [k for k, _ in stores] and sg.sizes() == [n for _, n in stores]      # first-appearance order
    assert sg.n_series == 193 and sg.n_groups == 9 and sg.n_chunks == sum((n + 31) // 32 for _, n in stores)
    assert sg.order.dtype == torch.int32 and sg.offsets.dtype == torch.int32
    assert sg.offsets.tolist() == np.concatenate([[0], np.cumsum([n for _, n in stores])]).tolist()
    for g, (store, _) in enumerate(stores):
        m = sg.order[sg.offsets[g]:sg.offsets[g + 1]].tolist()
        assert m == sorted(m) and all(ids[i].split("_", 1)[0] == store for i in m)
    assert sorted(sg.order.tolist()) == list(range(193))
    by_len = ftn.score.SeriesGroups.from_ids(ids, key=len)                                  # another key
    assert by_len.names == [str(k) for k in dict.fromkeys(len(s) for s in ids)] and sum(by_len.sizes()) == 193


def test_other_constructors(ftn):
    SG = ftn.score.SeriesGroups
    lab = SG.from_labels([2, -1, 0, 2, -1, 0, 0])
    assert lab.members == [[2, 5, 6], [], [0, 3]] and lab.n_series == 7 and lab.names == ["0", "1", "2"]
    assert SG.from_labels(torch.tensor([0, 1, -1])).members == [[0], [1]]
    mem = SG.from_members([[3, 1], [1, 2, 3], []], names=["a", "b", "c"], n_series=6)       # overlap, order kept
    assert mem.order.tolist() == [3, 1, 1, 2, 3] and mem.offsets.tolist() == [0, 2, 5, 5] and mem.n_series == 6
    assert SG.from_members([[0, 4]]).n_series == 5
    tot = mem.with_total()
    assert tot.names == ["a", "b", "c", "total"] and tot.members[-1] == list(range(6)) and tot.n_groups == 4
    assert mem.n_groups == 3 and mem.with_total("site").names[-1] == "site"
    assert mem.to("cpu") is mem and mem.to(torch.device("cpu")).order.device.type == "cpu"


def test_rejections(ftn):
    SG = ftn.score.SeriesGroups
    with pytest.raises(ValueError, match="outside"):
        SG.from_members([[0, 5]], n_series=5)
    with pytest.raises(ValueError, match="outside"):
        SG.from_members([[-1]], n_series=5)
    with pytest.raises(ValueError, match="duplicate"):
        SG.from_members([[0, 1], [2, 3, 2]], n_series=5)
    with pytest.raises(ValueError, match="G == 0"):
        SG.from_members([], n_series=5)
    with pytest.raises(ValueError, match="G == 0"):
        SG.from_labels([-1, -1])
    with pytest.raises(ValueError, match="below -1"):
        SG.from_labels([0, -2])
    with pytest.raises(ValueError, match="names"):
        SG.from_members([[0]], names=["a", "b"])
    sg = SG.from_members([[0, 1]], n_series=3)
    with pytest.raises(ValueError, match="N = 3"):
        ftn.score.group_sums(torch.ones(2, 4), sg)
    with pytest.raises(ValueError, match="backend"):
        ftn.score.group_sums(torch.ones(2, 3), sg, backend="numpy")
    with pytest.raises(ValueError, match="hip"):
        ftn.score.group_sums(torch.ones(2, 3), sg, backend="hip")                           # a CPU tensor
    with pytest.raises(ValueError, match="SeriesGroups"):
        ftn.score.group_sums(torch.ones(2, 3), [[0, 1]])


def _torch_sums(ftn, x, members, N):
    sg = ftn.score.SeriesGroups.from_members(members, n_series=N)
    out = ftn.score.group_sums(torch.from_numpy(x), sg)
    assert ftn.score._last_backend == "torch" and out.dtype == torch.float32
    return out.numpy()


@pytest.mark.parametrize("N", [1, 5, 33, 193, 260])
def test_torch_backend_bit_equal_to_numpy(N, ftn):
    g = np.random.default_rng(40 + N)
    for name, members in gc.layouts(N).items():
        for kind, x in gc.values(g, (3, 2, N), members).items():
            want = gc.group_sum(x, members)
            got = _torch_sums(ftn, x, members, N)
            assert got.shape == (3, 2, len(members)) and gc.bits_equal(got, want), (name, kind)
            if kind == "special":                               # NaN and inf reach only the groups that hold them
                for gi, m in enumerate(members):
                    held = (N // 2 in m) or (N > 1 and N - 1 in m)
                    assert bool(np.isfinite(want[..., gi]).all()) == (not held), (name, gi)


def test_torch_backend_group_sizes_and_empty(ftn):
    g = np.random.default_rng(5)
    sizes = [1, 31, 32, 33, 64, 65, 0]
    N = sum(sizes)
    perm = g.permutation(N).tolist()
    members, at = [], 0
    for s in sizes:
        members.append(perm[at:at + s])
        at += s
    for kind, x in gc.values(g, (4, N), members).items():
        want = gc.group_sum(x, members)
        got = _torch_sums(ftn, x, members, N)
        assert gc.bits_equal(got, want), kind
        assert (got[:, -1].view(np.uint32) == 0).all()          # the empty group: +0
    ints = gc.values(g, (4, N), members)["big"]                 # exact: the integer total itself
    exact = np.stack([ints[:, m].astype(np.int64).sum(1) for m in members], 1)
    assert exact.max() < 1 << 24 and np.array_equal(_torch_sums(ftn, ints, members, N).astype(np.int64), exact)
    assert _torch_sums(ftn, ints.astype(np.float64), members, N).dtype == np.float32        # another dtype: converted


def _fixture_groups(ftn):
    ids, _ = gc.fixture()
    return ftn.score.SeriesGroups.from_ids(ids).with_total()


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_group_path_summary_and_metrics_on_cpu(reduce, ftn):
    sc = ftn.score
    sg = _fixture_groups(ftn)
    g = np.random.default_rng(9)
    P, B, H, N = 7, 2, 6, 193
    x, y = pc.counts(g, (P, B, H, N), 2.0), pc.counts(g, (B, H, N), 2.0)
    xt, yt = gc.group_sum(x, sg.members), gc.group_sum(y, sg.members)
    mask = np.ones((B, H, N), dtype=bool)
    member = sg.members[3][4]
    mask[1, 2, member] = False                                  # one member of store 3 (and of the total) at one step
    gmask = np.stack([mask[..., m].all(-1) for m in sg.members], -1)
    assert gmask.sum() == B * H * 10 - 2 and not gmask[1, 2, 3] and not gmask[1, 2, 9]
    for window in (None, 2, 6):
        got = sc.group_path_summary(torch.from_numpy(x), sg, pc.LEVELS, torch.from_numpy(y), window=window,
                                    reduce=reduce, want_sorted=True)
        want = sc.path_summary(torch.from_numpy(xt), pc.LEVELS, torch.from_numpy(yt), window=window, reduce=reduce,
                               want_sorted=True)
        ora = pc.summary(xt, pc.LEVELS, window, reduce, yt)
        assert got["quantiles"].shape == (3, B, H // (window or 1), 10)
        for k in ("quantiles", "mean", "crps", "sorted"):
            assert torch.equal(got[k], want[k]), k
        assert pc.same(got["quantiles"].numpy(), ora["quantiles"]) and pc.same(got["sorted"].numpy(), ora["sorted"])
        for m, gm in ((None, None), (mask, gmask)):
            a = sc.group_path_metrics(torch.from_numpy(x), torch.from_numpy(y), sg, pc.LEVELS, window, reduce,
                                      None if m is None else torch.from_numpy(m))
            b = sc.path_metrics(torch.from_numpy(xt), torch.from_numpy(yt), pc.LEVELS, window, reduce,
                                None if gm is None else torch.from_numpy(gm))
            for k in ("coverage", "pinball", "crps", "count"):
                assert torch.equal(a[k], b[k]), (k, window)
            w = window or 1
            assert int(a["count"]) == B * (H // w) * 10 - (0 if m is None else 2)
    with pytest.raises(ValueError, match="mask"):
        sc.group_path_metrics(torch.from_numpy(x), torch.from_numpy(y), sg, pc.LEVELS, mask=torch.ones(2, 6))
    with pytest.raises(ValueError, match="y must be"):
        sc.group_path_summary(torch.from_numpy(x), sg, pc.LEVELS, torch.from_numpy(y[:, :3]))
    with pytest.raises(ValueError, match="samples"):
        sc.group_path_summary(torch.from_numpy(x[0]), sg, pc.LEVELS)


def test_entry_rejects_bad_arguments_before_any_launch(ftn):
    """Every call below fails a host check; the device pointers are never dereferenced and nothing is enqueued, so
    the addresses need not be device memory."""
    lib = ftn.lib.load()
    X, ORD, OFF, OUT = 0x10000, 0x20000, 0x30000, 0x40000

    def call(x=X, rows=4, N=8, stride=8, order=ORD, off=OFF, host=(0, 3, 8), G=None, M=None, out=OUT, host_ptr=None):
        arr = (C.c_int * max(len(host), 1))(*host)
        hp = C.cast(arr, C.c_void_p).value if host_ptr is None else host_ptr
        return lib.ftn_group_sum(x, rows, N, stride, order, off, hp if host else None, len(host) - 1 if G is None else G,
                                 host[-1] if M is None and host else (M or 0), out, None)

    assert call(x=None) < 0 and call(out=None) < 0 and call(off=None) < 0 and call(order=None) < 0
    assert call(host=()) < 0                                    # no host offsets
    assert call(stride=7) < 0 and call(N=0) < 0 and call(N=8193, stride=8193) < 0 and call(rows=0) < 0
    assert call(host=(0, 5, 3, 8)) < 0                          # not monotone
    assert call(host=(1, 3, 8)) < 0 and call(M=7) < 0 and call(M=9) < 0 and call(G=0) < 0 and call(G=2049) < 0
    assert call(host=tuple(range(0, 2050))) < 0                 # 2049 groups of one member: G and the chunks
    assert call(host=tuple(33 * i for i in range(1026))) < 0    # 1025 groups of 33: 2050 chunks
    assert call(x=X + 2) < 0 and call(out=OUT + 1) < 0 and call(order=ORD + 2) < 0 and call(off=OFF + 3) < 0
    assert call(rows=1 << 60, stride=1 << 20) < 0               # rows * row_stride beyond 64 bits
    assert b"ftn_group_sum" in lib.ftn_last_error()
    misaligned = (C.c_int * 4)(0, 3, 8, 0)
    assert call(host_ptr=C.addressof(misaligned) + 2) < 0
