"""Series-group sums on the MI355X (``ftn_group_sum`` behind ``score.group_sums``): every N, row count and group
layout of tests/groups_checks.py against its numpy oracle, bit for bit (the definition fixes the order of every
addition, so no tolerance applies), with the form that ran, the torch backend on the same tensor, strided and
misaligned views, guard words around the output, repeated calls, permuted rows, and the group path summaries and
metrics end to end on the fixture's stores."""
import numpy as np
import pytest
import torch

import groups_checks as gc
import paths_checks as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _groups(ftn, members, N, dev):
    return ftn.score.SeriesGroups.from_members(members, n_series=N, device=dev)


def _hip(ftn, xd, sg):
    out = ftn.score.group_sums(xd, sg, backend="hip")
    assert ftn.score._last_backend == "hip" and out.dtype == torch.float32
    return out


@pytest.mark.parametrize("N", gc.NS)
def test_every_layout_against_the_oracle(N, ftn, dev):
    rt, sc = ftn.runtime, ftn.score
    g = np.random.default_rng(2000 + N)
    for name, members in gc.layouts(N).items():
        sg = _groups(ftn, members, N, dev)
        G = len(members)
        for rows in gc.ROWS:
            for kind, x in gc.values(g, (rows, N), members).items():
                where = (N, name, rows, kind)
                xd = torch.from_numpy(x).to(dev)
                assert rt.group_sum_form(xd, sg.offsets_host) == gc.form(N, N, 0, gc.chunks(members)), where
                want = gc.group_sum(x, members)
                got = _hip(ftn, xd, sg)
                assert tuple(got.shape) == (rows, G) and gc.bits_equal(got.cpu().numpy(), want), where
                again = _hip(ftn, xd, sg)
                assert torch.equal(got.view(torch.int32), again.view(torch.int32)), where
                if kind in ("big", "special") and rows == 7:
                    ref = sc.group_sums(xd, sg, backend="torch")                 # the same device tensor
                    assert sc._last_backend == "torch" and gc.bits_equal(ref.cpu().numpy(), want), where
                if kind == "normal" and rows > 1:
                    perm = torch.from_numpy(g.permutation(rows)).to(dev)
                    moved = _hip(ftn, xd[perm].contiguous(), sg)
                    assert torch.equal(moved.view(torch.int32), got[perm].view(torch.int32)), where


@pytest.mark.parametrize("N", [4, 64, 193, 260])
def test_views_reach_their_form_and_agree(N, ftn, dev):
    rt = ftn.runtime
    g = np.random.default_rng(7 + N)
    members = gc.layouts(N)["overlap"]
    sg = _groups(ftn, members, N, dev)
    c = gc.chunks(members)
    P, B, H = 3, 2, 5
    x = (g.standard_normal((P, B, H, N)) * 10.0).astype(np.float32)
    want = gc.group_sum(x, members)
    for pad in (4, 3):                                          # a slice of a wider tensor: row stride above N
        wide = torch.zeros(P, B, H, N + pad, device=dev)
        wide[..., :N] = torch.from_numpy(x).to(dev)
        view = wide[..., :N]
        rows2d = ftn.score._group_rows(view)
        assert rows2d.data_ptr() == wide.data_ptr() and rows2d.stride(0) == N + pad     # passed without a copy
        assert rt.group_sum_form(rows2d, sg.offsets_host) == gc.form(N, N + pad, 0, c)
        assert gc.bits_equal(_hip(ftn, view, sg).cpu().numpy(), want), pad
    wide = torch.zeros(P, B, H, N + 4, device=dev)              # a base off the 16-byte grid: the scalar form
    wide[..., 1:N + 1] = torch.from_numpy(x).to(dev)
    view = wide[..., 1:N + 1]
    rows2d = ftn.score._group_rows(view)
    assert rows2d.data_ptr() == wide.data_ptr() + 4 and rows2d.data_ptr() % 16 == 4
    assert rt.group_sum_form(rows2d, sg.offsets_host) == gc.form(N, N + 4, 4, c) == f"scalar/t{gc.tile_rows(N, c)}"
    assert gc.bits_equal(_hip(ftn, view, sg).cpu().numpy(), want)
    dense = torch.from_numpy(x).to(dev)                         # [P, B, H, N] itself: one view of P B H rows
    rows2d = ftn.score._group_rows(dense)
    assert rows2d.data_ptr() == dense.data_ptr() and tuple(rows2d.shape) == (P * B * H, N)
    got = _hip(ftn, dense, sg)
    assert tuple(got.shape) == (P, B, H, len(members)) and gc.bits_equal(got.cpu().numpy(), want)
    host = ftn.score.SeriesGroups.from_members(members, n_series=N)             # groups built on the host: moved once
    assert gc.bits_equal(ftn.score.group_sums(dense, host).cpu().numpy(), want) and ftn.score._last_backend == "hip"
    assert host.to(dev) is host.to(dev) and host.to(dev).order.device == dev and host.order.device.type == "cpu"
    moved = dense.permute(1, 0, 2, 3)                           # dims that do not collapse: copied, same totals
    assert gc.bits_equal(_hip(ftn, moved, sg).cpu().numpy(), want.transpose(1, 0, 2, 3))


@pytest.mark.parametrize("N", [5, 64, 260])
def test_guard_words_around_the_output(N, ftn, dev):
    rt = ftn.runtime
    g = np.random.default_rng(11 + N)
    sentinel = -12345.0
    for name in ("own", "mod3", "empty"):
        members = gc.layouts(N)[name]
        sg = _groups(ftn, members, N, dev)
        G = len(members)
        for rows in (7, 67):
            x = g.poisson(2.0, (rows, N)).astype(np.float32)
            want = gc.group_sum(x, members)
            for lead in (4, 1):
                buf = torch.full((rows * G + 2 * lead + 3,), sentinel, device=dev)
                out = buf[lead:lead + rows * G].view(rows, G)
                got = rt.group_sum(torch.from_numpy(x).to(dev), sg.order, sg.offsets, sg.offsets_host, out=out)
                assert got.data_ptr() == out.data_ptr() and gc.bits_equal(got.cpu().numpy(), want), (name, rows, lead)
                assert bool((buf[:lead] == sentinel).all()) and bool((buf[lead + rows * G:] == sentinel).all())


def test_a_group_does_not_depend_on_the_rows_or_the_other_groups(ftn, dev):
    g = np.random.default_rng(17)
    N = 260
    row = (g.standard_normal(N) * 1e3).astype(np.float32)
    mine = g.permutation(N)[:70].tolist()
    seen = set()
    for rows, at, others in ((1, 0, []), (7, 3, [[1, 2, 3]]), (67, 66, [list(range(N)), []]),
                             (130, 64, [[i] for i in range(100)])):
        x = (g.standard_normal((rows, N)) * 1e3).astype(np.float32)
        x[at] = row
        members = others + [mine]
        got = _hip(ftn, torch.from_numpy(x).to(dev), _groups(ftn, members, N, dev)).cpu().numpy()
        assert gc.bits_equal(got, gc.group_sum(x, members))
        seen.add(got[at, -1].tobytes())
    assert len(seen) == 1


def _fixture_groups(ftn, dev):
    ids, stores = gc.fixture()
    sg = ftn.score.SeriesGroups.from_ids(ids, device=dev).with_total()
    assert sg.names == [k for k, _ in stores] + ["total"] and sg.order.device == dev
    return sg


@pytest.mark.parametrize("P", [5, 100])
def test_group_path_summary_end_to_end(P, ftn, dev):
    sc = ftn.score
    sg = _fixture_groups(ftn, dev)
    g = np.random.default_rng(31 + P)
    B, H, N = 2, 6, 193
    x, y = pc.counts(g, (P, B, H, N), 2.0), pc.counts(g, (B, H, N), 2.0)
    xt, yt = gc.group_sum(x, sg.members), gc.group_sum(y, sg.members)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    for window in (None, 2, 6):
        for reduce in ("sum", "max"):
            where = (P, window, reduce)
            want = pc.summary(xt, pc.LEVELS, window, reduce, yt)
            out = sc.group_path_summary(xd, sg, pc.LEVELS, yd, window=window, reduce=reduce, want_sorted=True)
            assert sc._last_backend == "hip"
            got = {k: v.cpu().numpy() for k, v in out.items()}
            assert got["quantiles"].shape == (3, B, H // (window or 1), 10), where
            assert pc.same(got["quantiles"], want["quantiles"]) and pc.same(got["sorted"], want["sorted"]), where
            mean64 = want["sorted"].astype(np.float64).sum(0) / P
            assert pc.within_ulp(got["mean"], mean64, want["mean_scale"]), where
            assert pc.within_ulp(got["crps"], want["crps64"], want["scale"]), where


@pytest.mark.parametrize("P", [5, 100])
def test_group_path_metrics_end_to_end(P, ftn, dev):
    sc = ftn.score
    sg = _fixture_groups(ftn, dev)
    g = np.random.default_rng(57 + P)
    B, H, N = 2, 6, 193
    x, y = pc.counts(g, (P, B, H, N), 2.0), pc.counts(g, (B, H, N), 2.0)
    xt, yt = gc.group_sum(x, sg.members), gc.group_sum(y, sg.members)
    mask = np.ones((B, H, N), dtype=bool)
    mask[1, 2, sg.members[3][4]] = False                        # one member of store 3 (and of the total) at one step
    gmask = np.stack([mask[..., m].all(-1) for m in sg.members], -1)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    xtd, ytd = torch.from_numpy(xt).to(dev), torch.from_numpy(yt).to(dev)
    for window in (None, 2, 6):
        for reduce in ("sum", "max"):
            for m, gm in ((None, None), (mask, gmask)):
                a = sc.group_path_metrics(xd, yd, sg, pc.LEVELS, window, reduce,
                                          None if m is None else torch.from_numpy(m).to(dev))
                assert sc._last_backend == "hip"
                b = sc.path_metrics(xtd, ytd, pc.LEVELS, window, reduce,
                                    None if gm is None else torch.from_numpy(gm).to(dev))
                for k in ("coverage", "pinball", "crps", "count"):
                    assert torch.equal(a[k], b[k]), (k, P, window, reduce)
                assert int(a["count"]) == B * (H // (window or 1)) * 10 - (0 if m is None else 2)
