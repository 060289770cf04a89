"""Series groups along another axis on the MI355X (``ftn_group_sum_rows`` behind ``score.group_sums(..., axis=)``):
every member count, inner extent and group layout against the numpy oracle on the moved axis, bit for bit (the
definition fixes the order of every addition, so no tolerance applies), with the form that ran, the existing kernel
on the transposed copy, the torch backend on the same tensor, the limits, strided and misaligned views, guard words
around the output, the independence of a column's total from everything around it, and the group path summaries and
metrics end to end with the fixture's stores along the batch axis."""
import numpy as np
import pytest
import torch

import group_rows_checks as rc
import groups_checks as gc
import paths_checks as pc

pytestmark = pytest.mark.gpu

INNER = [1, 3, 4, 5, 28, 33, 67]     # degenerate, scalar, one quad, scalar, the pipeline's H, past 32 lanes, a partial tile


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


def _groups(ftn, members, S, dev):
    return ftn.score.SeriesGroups.from_members(members, n_series=S, device=dev)


def _hip(ftn, xd, sg, axis=1, entry="ftn_group_sum_rows"):
    out = ftn.score.group_sums(xd, sg, backend="hip", axis=axis)
    assert ftn.score._last_backend == "hip" and out.dtype == torch.float32
    assert ftn.score._last_group_entry == entry
    return out


def _same_bits(a, b):
    return gc.bits_equal(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("inner", INNER)
@pytest.mark.parametrize("S", rc.SS)
def test_every_layout_against_the_oracle(S, inner, ftn, dev):
    rt, sc = ftn.runtime, ftn.score
    g = np.random.default_rng(3000 + 100 * S + inner)
    for name, members in gc.layouts(S).items():
        sg = _groups(ftn, members, S, dev)
        G, c = len(members), gc.chunks(members)
        for outer in (1, 3):
            for kind, x in rc.values(g, (outer, S, inner), 1, members).items():
                where = (S, inner, name, outer, kind)
                xd = torch.from_numpy(x).to(dev)
                v = sc._group_slabs(xd, 1)
                assert v.data_ptr() == xd.data_ptr(), where
                if inner == 1:                                  # N fastest: the existing kernel on the [outer, S] view
                    entry = "ftn_group_sum"
                    assert rt.group_sum_form(v[:, :, 0], sg.offsets_host) == gc.form(S, S, 0, c), where
                else:
                    entry = "ftn_group_sum_rows"
                    want_form = rc.form(inner, inner, S * inner if outer > 1 else 0, 0)
                    assert rt.group_sum_rows_form(v, sg.offsets_host) == want_form, where
                want = rc.oracle(x, members, 1)
                got = _hip(ftn, xd, sg, 1, entry)
                assert tuple(got.shape) == (outer, G, inner) and gc.bits_equal(got.cpu().numpy(), want), where
                assert _same_bits(_hip(ftn, xd, sg, 1, entry), got), where
                moved = sc.group_sums(xd.movedim(1, -1).contiguous(), sg, backend="hip")
                assert sc._last_group_entry == "ftn_group_sum" and _same_bits(moved.movedim(-1, 1), got), where
                if kind in ("big", "special"):
                    ref = sc.group_sums(xd, sg, backend="torch", axis=1)             # the same device tensor
                    assert sc._last_backend == "torch" and _same_bits(ref, got), where


def test_the_group_and_chunk_limits(ftn, dev):
    rt = ftn.runtime
    S = 2048
    members = gc.layouts(S)["own"]                              # G = 2048, 2048 chunks: two passes of 1024
    sg = _groups(ftn, members, S, dev)
    g = np.random.default_rng(41)
    x = (g.standard_normal((1, S, 5)) * 100.0).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    assert rt.group_sum_rows_form(xd, sg.offsets_host) == rc.form(5, 5, 0, 0) == "scalar/i4" and rc.passes(5, 2048) == 2
    got = _hip(ftn, xd, sg)
    assert gc.bits_equal(got.cpu().numpy(), rc.oracle(x, members, 1)) and _same_bits(got, xd)  # a group of one: itself


@pytest.mark.parametrize("inner", [64, 35])
def test_groups_that_run_across_the_passes_of_a_tile(inner, ftn, dev):
    """A tile of 64 columns takes 64 chunks a pass, one of 32 takes 128: groups of 130 and 132 chunks begin, run through
    and end at different places in a pass, between empty groups and short ones, and give the bits of the oracle - and
    one member list gives the same bits wherever its chunks fall."""
    S = 4200
    g = np.random.default_rng(71 + inner)
    mine = g.permutation(S)[:4160].tolist()                     # 130 chunks
    every = list(range(S))                                      # 132 chunks
    x = (g.standard_normal((2, S, inner)) * 1e3).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    seen = set()
    for others in ([], [[]], [every], [list(range(1000)), [], every, list(range(0, S, 2))],
                   [[i] for i in range(50)] + [every] + [[]], [list(range(31 * 32 + 1))]):
        members = others + [mine, [], [7]]
        sg = _groups(ftn, members, S, dev)
        assert ftn.runtime.group_sum_rows_form(xd, sg.offsets_host) == rc.form(inner, inner, S * inner, 0)
        assert rc.passes(inner, gc.chunks(members)) >= 2
        got = _hip(ftn, xd, sg).cpu().numpy()
        assert gc.bits_equal(got, rc.oracle(x, members, 1)), len(others)
        seen.add(got[:, -3].tobytes())
    assert len(seen) == 1


@pytest.mark.parametrize("inner", [5, 1])
def test_more_members_than_the_series_kernel_takes(inner, ftn, dev):
    rt, sc = ftn.runtime, ftn.score
    S = 8200
    assert S > sc.GROUP_NMAX
    members = [list(range(0, S, 2)), list(range(1, S, 2)), list(range(S))]
    sg = _groups(ftn, members, S, dev)
    g = np.random.default_rng(43 + inner)
    for kind, x in rc.values(g, (2, S, inner), 1, members).items():
        xd = torch.from_numpy(x).to(dev)
        assert rt.group_sum_rows_form(xd, sg.offsets_host) == rc.form(inner, inner, S * inner, 0)
        got = _hip(ftn, xd, sg)                                 # backend="hip" ran the new kernel
        assert gc.bits_equal(got.cpu().numpy(), rc.oracle(x, members, 1)), kind
    with pytest.raises(ValueError, match="hip"):                # along the last axis the old limit stands
        sc.group_sums(xd.movedim(1, -1).contiguous(), sg, backend="hip")


def test_views_reach_their_form_and_agree(ftn, dev):
    rt, sc = ftn.runtime, ftn.score
    S, inner, outer = 193, 8, 3
    g = np.random.default_rng(47)
    members = gc.layouts(S)["overlap"]
    sg = _groups(ftn, members, S, dev)
    c = gc.chunks(members)
    x = (g.standard_normal((outer, S, inner)) * 10.0).astype(np.float32)
    want = rc.oracle(x, members, 1)
    xd = torch.from_numpy(x).to(dev)
    for pad in (4, 3):                                          # a slice of a wider tensor: member stride above inner
        wide = torch.zeros(outer, S, inner + pad, device=dev)
        wide[..., :inner] = xd
        view = wide[..., :inner]
        v = sc._group_slabs(view, 1)
        assert v.data_ptr() == wide.data_ptr() and v.stride() == (S * (inner + pad), inner + pad, 1)    # no copy
        form = rt.group_sum_rows_form(v, sg.offsets_host)
        assert form == rc.form(inner, inner + pad, S * (inner + pad), 0) == ("vec4/i8" if pad == 4 else "scalar/i8")
        assert gc.bits_equal(_hip(ftn, view, sg).cpu().numpy(), want), pad
    tall = torch.zeros(outer, S + 7, inner, device=dev)         # a slice along the member axis of a taller tensor
    tall[:, 2:S + 2] = xd
    view = tall[:, 2:S + 2]
    v = sc._group_slabs(view, 1)
    assert v.data_ptr() == tall.data_ptr() + 2 * inner * 4 and v.stride() == ((S + 7) * inner, inner, 1)
    assert rt.group_sum_rows_form(v, sg.offsets_host) == rc.form(inner, inner, (S + 7) * inner, 0) == "vec4/i8"
    assert gc.bits_equal(_hip(ftn, view, sg).cpu().numpy(), want)
    wide = torch.zeros(outer, S, inner + 4, device=dev)         # a base off the 16-byte grid: the scalar form
    wide[..., 1:inner + 1] = xd
    view = wide[..., 1:inner + 1]
    v = sc._group_slabs(view, 1)
    assert v.data_ptr() == wide.data_ptr() + 4 and v.data_ptr() % 16 == 4
    assert rt.group_sum_rows_form(v, sg.offsets_host) == rc.form(inner, inner + 4, S * (inner + 4), 4) == "scalar/i8"
    assert gc.bits_equal(_hip(ftn, view, sg).cpu().numpy(), want)
    P, H, N = 2, 5, 2                                           # [P, B, H, N = 2]: H and N collapse into inner = 2 H
    x4 = (g.standard_normal((P, S, H, N)) * 10.0).astype(np.float32)
    x4d = torch.from_numpy(x4).to(dev)
    v = sc._group_slabs(x4d, 1)
    assert v.data_ptr() == x4d.data_ptr() and tuple(v.shape) == (P, S, 2 * H)
    got = _hip(ftn, x4d, sg)
    assert tuple(got.shape) == (P, 3, H, N) and gc.bits_equal(got.cpu().numpy(), rc.oracle(x4, members, 1))
    host = sc.SeriesGroups.from_members(members, n_series=S)    # groups built on the host: moved once
    assert gc.bits_equal(sc.group_sums(x4d, host, axis=1).cpu().numpy(), rc.oracle(x4, members, 1))
    assert sc._last_backend == "hip" and sc._last_group_entry == "ftn_group_sum_rows"
    moved = x4d.permute(0, 1, 3, 2)                             # dims that do not collapse: copied, same totals
    assert sc._group_slabs(moved, 1).data_ptr() != x4d.data_ptr()
    assert gc.bits_equal(_hip(ftn, moved, sg).cpu().numpy(), rc.oracle(x4.transpose(0, 1, 3, 2), members, 1))
    front = x4d.permute(1, 0, 2, 3)                             # the members along dim 0 of a permuted tensor: copied
    assert gc.bits_equal(_hip(ftn, front, sg, 0).cpu().numpy(), rc.oracle(x4.transpose(1, 0, 2, 3), members, 0))
    x1 = (g.standard_normal((P, S, 1, 1)) * 10.0).astype(np.float32)     # [P, B, 1, 1]: the existing kernel answers
    x1d = torch.from_numpy(x1).to(dev)
    flat = sc._group_slabs(x1d, 1)[:, :, 0]
    assert flat.data_ptr() == x1d.data_ptr() and tuple(flat.shape) == (P, S) and flat.stride(1) == 1
    assert rt.group_sum_form(flat, sg.offsets_host) == gc.form(S, S, 0, c)
    got = _hip(ftn, x1d, sg, 1, "ftn_group_sum")
    assert tuple(got.shape) == (P, 3, 1, 1) and gc.bits_equal(got.cpu().numpy(), rc.oracle(x1, members, 1))
    strided = torch.zeros(P, S, 2, device=dev)                  # one column of two: members 2 apart, the new kernel
    strided[..., 0] = x1d[:, :, 0, 0]
    got = _hip(ftn, strided[..., :1], sg)
    assert gc.bits_equal(got.cpu().numpy(), rc.oracle(x1[:, :, 0], members, 1))


@pytest.mark.parametrize("inner", [5, 28])
def test_guard_words_around_the_output(inner, ftn, dev):
    rt = ftn.runtime
    g = np.random.default_rng(51 + inner)
    sentinel = -12345.0
    for S in (5, 260):
        for name in ("own", "mod3", "empty"):
            members = gc.layouts(S)[name]
            sg = _groups(ftn, members, S, dev)
            G, c = len(members), gc.chunks(members)
            for outer in (1, 3):
                x = g.poisson(2.0, (outer, S, inner)).astype(np.float32)
                xd = torch.from_numpy(x).to(dev)
                want = rc.oracle(x, members, 1)
                n = outer * G * inner
                for lead in (4, 1):
                    buf = torch.full((n + 2 * lead + 3,), sentinel, device=dev)
                    out = buf[lead:lead + n].view(outer, G, inner)
                    form = rt.group_sum_rows_form(xd, sg.offsets_host, out)
                    assert form == rc.form(inner, inner, S * inner if outer > 1 else 0, 4 * (lead % 4))
                    got = rt.group_sum_rows(xd, sg.order, sg.offsets, sg.offsets_host, out=out)
                    where = (S, name, outer, lead)
                    assert got.data_ptr() == out.data_ptr() and gc.bits_equal(got.cpu().numpy(), want), where
                    assert bool((buf[:lead] == sentinel).all()) and bool((buf[lead + n:] == sentinel).all()), where


def test_a_total_depends_on_its_members_and_its_column_alone(ftn, dev):
    g = np.random.default_rng(57)
    S, inner = 260, 67
    column = (g.standard_normal(S) * 1e3).astype(np.float32)
    mine = g.permutation(S)[:70].tolist()
    seen = set()
    for outer, o_at, col, others in ((1, 0, 0, []), (3, 2, 66, [list(range(S))]), (7, 3, 63, [[1, 2, 3], []]),
                                     (2, 1, 64, [[i] for i in range(100)]), (5, 0, 35, [[i] for i in range(100)]),
                                     (2, 0, 36, [list(range(S)), [i for i in range(0, S, 2)]])):
        x = (g.standard_normal((outer, S, inner)) * 1e3).astype(np.float32)
        x[o_at, :, col] = column
        members = others + [mine]
        got = _hip(ftn, torch.from_numpy(x).to(dev), _groups(ftn, members, S, dev)).cpu().numpy()
        assert gc.bits_equal(got, rc.oracle(x, members, 1))
        seen.add(got[o_at, -1, col].tobytes())
    assert len(seen) == 1
    narrow = np.ascontiguousarray(column.reshape(1, S, 1).repeat(2, 2))             # inner = 2: another tile, scalar
    got = _hip(ftn, torch.from_numpy(narrow).to(dev), _groups(ftn, [mine], S, dev)).cpu().numpy()
    assert {got[0, 0, 0].tobytes(), got[0, 0, 1].tobytes()} == seen


def _fixture_groups(ftn, dev):
    ids, stores = gc.fixture()
    sg = ftn.score.SeriesGroups.from_ids(ids, device=dev).with_total()
    assert sg.names == [k for k, _ in stores] + ["total"] and sg.order.device == dev and sg.n_series == 193
    return sg


@pytest.mark.parametrize("P", [5, 100])
def test_pipeline_group_path_summary_end_to_end(P, ftn, dev):
    sc = ftn.score
    sg = _fixture_groups(ftn, dev)
    g = np.random.default_rng(61 + P)
    B, H, N = 193, 6, 1
    x, y = pc.counts(g, (P, B, H, N), 2.0), pc.counts(g, (B, H, N), 2.0)
    xt, yt = rc.oracle(x, sg.members, 1), rc.oracle(y, sg.members, 0)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    for window in (None, 2, 6):
        for reduce in ("sum", "max"):
            where = (P, window, reduce)
            want = pc.summary(xt, pc.LEVELS, window, reduce, yt)
            out = sc.group_path_summary(xd, sg, pc.LEVELS, yd, window=window, reduce=reduce, want_sorted=True, axis=1)
            assert sc._last_backend == "hip"
            got = {k: v.cpu().numpy() for k, v in out.items()}
            assert got["quantiles"].shape == (3, 10, H // (window or 1), N), where
            assert pc.same(got["quantiles"], want["quantiles"]) and pc.same(got["sorted"], want["sorted"]), where
            mean64 = want["sorted"].astype(np.float64).sum(0) / P
            assert pc.within_ulp(got["mean"], mean64, want["mean_scale"]), where
            assert pc.within_ulp(got["crps"], want["crps64"], want["scale"]), where
    assert gc.bits_equal(sc.group_sums(xd, sg, backend="hip", axis=1).cpu().numpy(), xt)
    assert sc._last_group_entry == "ftn_group_sum_rows"


@pytest.mark.parametrize("P", [5, 100])
def test_pipeline_group_path_metrics_end_to_end(P, ftn, dev):
    sc = ftn.score
    sg = _fixture_groups(ftn, dev)
    g = np.random.default_rng(67 + P)
    B, H, N = 193, 6, 1
    x, y = pc.counts(g, (P, B, H, N), 2.0), pc.counts(g, (B, H, N), 2.0)
    xt, yt = rc.oracle(x, sg.members, 1), rc.oracle(y, sg.members, 0)
    mask = np.ones((B, H, N), dtype=bool)
    mask[sg.members[3][4], 2, 0] = False                        # one member row of store 3 (and of the total) at one step
    gmask = np.stack([mask[m].all(0) for m in sg.members], 0)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    xtd, ytd = torch.from_numpy(xt).to(dev), torch.from_numpy(yt).to(dev)
    for window in (None, 2, 6):
        for reduce in ("sum", "max"):
            for m, gm in ((None, None), (mask, gmask)):
                a = sc.group_path_metrics(xd, yd, sg, pc.LEVELS, window, reduce,
                                          None if m is None else torch.from_numpy(m).to(dev), axis=1)
                assert sc._last_backend == "hip"
                b = sc.path_metrics(xtd, ytd, pc.LEVELS, window, reduce,
                                    None if gm is None else torch.from_numpy(gm).to(dev))
                for k in ("coverage", "pinball", "crps", "count"):
                    assert torch.equal(a[k], b[k]), (k, P, window, reduce)
                assert int(a["count"]) == (H // (window or 1)) * 10 - (0 if m is None else 2)
