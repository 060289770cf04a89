"""The kernel forms of ``ftn_table_moments``, ``ftn_table_spectrum`` and ``ftn_table_affine`` (``ftn_table_*_form``,
host-only: the launches dispatch through the same functions) pinned for every shape of the GPU sweep
(tests/table_checks.py) in each table layout, for the realistic shapes, and at the boundaries the kernels have:

* spectrum staging chunks of 128 rows: T = 128 | 129 is one chunk (column tile LDS-resident) against two (streamed),
  256 | 257 two against three; bin blocks of 128 bins: T = 257 | 258 is one partial against two;
* moments row blocks: 32 rows up to T = 1024, then doubled (T = 1024 | 1025 is 32 blocks of 32 against 17 of 64);
* 16-byte lanes only where the header's conditions hold, 4-byte lanes everywhere else."""
import pytest

import table_checks as tc


def test_literal_forms(ftn):
    rt = ftn.runtime
    mom, spec, aff = rt.table_moments_form_of, rt.table_spectrum_form_of, rt.table_affine_form_of
    base = dict(chunk=0, resident=0, lane_axis=0)
    assert mom(731, 512) == dict(load_bytes=16, col_tile=1024, block=32, partials=23, **base)
    assert mom(731, 37, mask=True, diffs=True) == dict(load_bytes=4, col_tile=256, block=32, partials=23, **base)
    assert mom(1024, 512)["partials"] == 32 and mom(1025, 512) == dict(load_bytes=16, col_tile=1024, block=64,
                                                                      partials=17, **base)
    assert mom(4096, 30490) == dict(load_bytes=4, col_tile=256, block=128, partials=32, **base)
    assert mom(1913, 512, x_stride=514)["load_bytes"] == 4 and mom(1913, 512, x_stride=516)["load_bytes"] == 16
    assert mom(1913, 512, misalign={"X": 4})["load_bytes"] == 4
    assert mom(1913, 512, misalign={"M": 4})["load_bytes"] == 16            # without the mask flag M is not read
    assert mom(1913, 512, mask=True, misalign={"M": 4})["load_bytes"] == 4
    sp = dict(col_tile=64, block=128, chunk=128, lane_axis=0)
    assert spec(731, 512) == dict(load_bytes=16, resident=0, partials=3, **sp)
    assert spec(1913, 512) == dict(load_bytes=16, resident=0, partials=8, **sp)
    assert spec(4096, 30490) == dict(load_bytes=4, resident=0, partials=16, **sp)
    assert spec(65536, 4)["partials"] == 256
    assert spec(128, 64) == dict(load_bytes=16, resident=1, partials=1, **sp)
    assert spec(129, 64) == dict(load_bytes=16, resident=0, partials=1, **sp)
    assert spec(257, 64)["partials"] == 1 and spec(258, 64)["partials"] == 2
    assert spec(1, 8)["partials"] == 0 and spec(2, 8)["partials"] == 1
    assert spec(731, 512, has_mask=False, misalign={"M": 4})["load_bytes"] == 16
    assert spec(731, 512, m_stride=514)["load_bytes"] == 4
    with pytest.raises(ValueError, match="outside the supported"):
        spec(65537, 4)
    af = dict(col_tile=0, block=1024, chunk=0, resident=0, partials=0)
    assert aff(731, 512, 1) == dict(load_bytes=16, lane_axis=2, **af)                 # the table: series contiguous
    assert aff(731, 510, 1) == dict(load_bytes=4, lane_axis=0, **af)
    assert aff(1, 193, 28) == dict(load_bytes=16, lane_axis=1, **af)                  # the pipeline layout [B, H, 1], axis 0
    assert aff(1, 193, 7) == dict(load_bytes=4, lane_axis=0, **af)
    assert aff(8, 193, 28, series=True, n_cols=30490, inverse=True) == dict(load_bytes=16, lane_axis=1, **af)
    assert aff(4, 64, 1, x_strides=(66, 1)) == dict(load_bytes=4, lane_axis=0, **af)
    assert aff(4, 64, 1, x_strides=(68, 1)) == dict(load_bytes=16, lane_axis=2, **af)
    assert aff(4, 64, 1, misalign={"out": 4}) == dict(load_bytes=4, lane_axis=0, **af)
    assert aff(4, 64, 4, x_strides=(512, 6)) == dict(load_bytes=4, lane_axis=0, **af)
    assert aff(4, 64, 4, x_strides=(512, 8)) == dict(load_bytes=16, lane_axis=1, **af)


@pytest.mark.parametrize("case", tc.sweep(), ids=tc.case_id)
def test_sweep_forms(case, ftn):
    rt = ftn.runtime
    T, N = case["T"], case["N"]
    masked = case["mask"] != "none"
    for layout in tc.LAYOUTS:                                   # the case's own layout and the other two
        kw = tc.layout_args(dict(case, layout=layout))
        assert rt.table_moments_form_of(T, N, mask=masked, diffs=True, **kw) == tc.want_moments_form(T, N, mask=masked, **kw)
        assert rt.table_moments_form_of(T, N, **kw) == tc.want_moments_form(T, N, **kw)
        assert rt.table_spectrum_form_of(T, N, has_mask=masked, **kw) == tc.want_spectrum_form(T, N, has_mask=masked, **kw)
        xs = (kw.get("x_stride", N), 1)
        mis = {"x": kw.get("misalign", {}).get("X", 0)}
        assert rt.table_affine_form_of(T, N, 1, x_strides=xs, misalign=mis) == tc.want_affine_form(T, N, 1, x_strides=xs,
                                                                                                 misalign=mis)


def test_sweep_covers_the_boundaries(ftn):
    """The sweep reaches what it is meant to reach, by the library's own form queries: both load widths of the moments
    and of the spectrum, the 16-byte forms on a strided table (row stride > N) with and without a mask at every
    staging-chunk and bin-block boundary, and every pairing of mask kind, layout and N that a rotation could hide."""
    rt = ftn.runtime
    Ts = set(tc.SWEEP_T)
    assert {127, 128, 129, 130, 255, 256, 257, 258} <= Ts       # two lengths on either side of both chunk boundaries
    forms = {(tc.want_spectrum_form(T, 64)["resident"], tc.want_spectrum_form(T, 64)["partials"]) for T in Ts}
    assert forms == {(1, 0), (1, 1), (0, 1), (0, 2)}
    cases = tc.sweep()
    assert [c["T"] for c in cases[:len(tc.SWEEP_T)]] == list(tc.SWEEP_T)
    assert {c["N"] for c in cases} == set(tc.SWEEP_N)
    assert {(c["mask"], c["layout"]) for c in cases} == {(m, l) for m in tc.MASKS for l in tc.LAYOUTS}
    for N in tc.SWEEP_N:                                        # neither the mask nor the layout is a function of N
        mine = [c for c in cases if c["N"] == N]
        assert len({c["layout"] for c in mine}) > 1, N
        if N % 4 == 0:                                          # the widths that can take 16-byte loads meet every mask kind
            assert {c["mask"] for c in mine} == set(tc.MASKS) and {"slice4", "dense"} & {c["layout"] for c in mine}, N
    assert sum(len({c["mask"] for c in cases if c["N"] == N}) > 1 for N in tc.SWEEP_N) >= 7
    seen = {"moments": set(), "spectrum": set()}
    wide_strided = {}                                           # T -> the mask kinds of its 16-byte cases with stride > N
    for c in cases:
        kw = tc.layout_args(c)
        masked = c["mask"] != "none"
        mom = rt.table_moments_form_of(c["T"], c["N"], mask=masked, diffs=True, **kw)
        spec = rt.table_spectrum_form_of(c["T"], c["N"], has_mask=masked, **kw)
        seen["moments"].add(mom["load_bytes"])
        seen["spectrum"].add(spec["load_bytes"])
        if mom["load_bytes"] == 16 and spec["load_bytes"] == 16 and kw.get("x_stride", c["N"]) > c["N"]:
            wide_strided.setdefault(c["T"], set()).add(masked)
    assert seen == {"moments": {4, 16}, "spectrum": {4, 16}}
    for T in (128, 129, 256, 257, 258):
        assert T in wide_strided, T
    assert {m for v in wide_strided.values() for m in v} == {False, True}
    assert any(len(v) == 2 for v in wide_strided.values())
