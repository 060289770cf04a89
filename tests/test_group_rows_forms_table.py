"""``ftn_group_sum_rows_form`` (host-only; the launch dispatches through it) pinned to the independent statement of
the header's rule in tests/group_rows_checks.py over inner extents, chunk counts, strides and base alignments."""
import pytest

import group_rows_checks as rc

INNER = [1, 3, 4, 5, 28, 33, 64, 260]
CHUNKS = [1, 20, 256, 257, 2048]


@pytest.mark.parametrize("inner", INNER)
def test_form_matches_the_header_rule(inner, ftn):
    rt, f = ftn.runtime, ftn.lib.load().ftn_group_sum_rows_form
    for chunks in CHUNKS:
        for pad in (0, 4, 3, 8):                                # member strides that are multiples of 4 and not
            ms = inner + pad
            for os_ in (0, 300 * ms, 300 * ms + 4, 300 * ms + 2):
                for mis in (0, 4, 8, 12):
                    where = (inner, chunks, ms, os_, mis)
                    assert rt.group_sum_rows_form_of(inner, ms, os_, mis, chunks) == rc.form(inner, ms, os_, mis), where
                    assert f(inner, ms, os_, mis, chunks) == rc.form_word(inner, ms, os_, mis, chunks), where
    assert rt.group_sum_rows_form_of(inner) == rc.form(inner, inner, 0, 0)      # the defaults: dense, aligned, no chunk


def test_the_rule_at_its_corners(ftn):
    rt, f = ftn.runtime, ftn.lib.load().ftn_group_sum_rows_form
    assert [rc.tile_cols(i) for i in (1, 3, 4, 5, 28, 33, 64, 67, 260)] == [1, 3, 4, 4, 28, 32, 64, 64, 64]
    assert rc.passes(28, 0) == 1 and rc.passes(28, 146) == 1 and rc.passes(28, 147) == 2 and rc.passes(28, 2048) == 15
    assert rc.passes(64, 64) == 1 and rc.passes(64, 65) == 2 and rc.passes(260, 2048) == 32 and rc.passes(1, 2048) == 1
    assert rt.group_sum_rows_form_of(28, 28, 28 * 8192, 0, 20) == "vec4/i28"
    assert rt.group_sum_rows_form_of(28, 28, 28 * 8192, 0, 2048) == "vec4/i28"      # the chunks move only the passes
    assert f(28, 28, 28 * 8192, 0, 2048) == 2 | 28 << 8 | 15 << 16
    assert rt.group_sum_rows_form_of(28, 28, 28 * 8192, 4, 20) == "scalar/i28"
    assert rt.group_sum_rows_form_of(28, 30, 30 * 8192, 0, 20) == "scalar/i28"
    assert rt.group_sum_rows_form_of(28, 28, 28 * 8192 + 2, 0, 20) == "scalar/i28"
    assert rt.group_sum_rows_form_of(64, 64, 0, 0, 0) == "vec4/i64"


def test_form_function_rejects(ftn):
    lib = ftn.lib.load()
    f = lib.ftn_group_sum_rows_form
    assert f(0, 4, 0, 0, 1) < 0 and f(4, 3, 0, 0, 1) < 0 and f(4, 4, -1, 0, 1) < 0
    assert f(4, 4, 0, 0, 2049) < 0 and f(4, 4, 0, 0, -1) < 0
    assert f(4, 4, 0, 16, 1) < 0 and f(4, 4, 0, 2, 1) < 0 and f(4, 4, 0, -4, 1) < 0
    assert b"ftn_group_sum_rows_form" in lib.ftn_last_error()
    assert f(4, 4, 0, 0, 2048) >= 0
