"""The dispatch table of the series-group kernel (``ftn_group_sum_form``; host-only, no GPU needed): the load width
and the tile height it reports equal the rule of include/flowtimes.h as tests/groups_checks.py restates it, over
(N, row stride, misalignment, chunk count), at the limits, and for the layouts the GPU test uses."""
import pytest

import groups_checks as gc

TABLE = [  # (N, row stride, address & 15, chunks)
    (1, 1, 0, 1), (3, 3, 0, 3), (4, 4, 0, 1), (4, 4, 4, 1), (4, 6, 0, 1), (4, 8, 0, 4), (5, 8, 0, 2),
    (33, 33, 0, 2), (64, 64, 0, 2), (64, 64, 8, 64), (64, 65, 0, 2), (64, 68, 12, 2), (193, 193, 0, 10),
    (193, 196, 0, 17), (260, 260, 0, 9), (260, 260, 0, 260), (260, 264, 4, 9), (512, 512, 0, 25), (512, 512, 0, 41),
    (512, 1024, 0, 0), (2048, 2048, 0, 2048), (4096, 4096, 0, 128), (8192, 8192, 0, 256), (8192, 8192, 0, 2048),
    (8191, 8192, 0, 2048), (8192, 8196, 8, 1),
]


@pytest.mark.parametrize("N,stride,mis,chunks", TABLE)
def test_form_follows_the_stated_rule(N, stride, mis, chunks, ftn):
    rt = ftn.runtime
    got = rt.group_sum_form_of(N, stride, mis, chunks)
    assert got == gc.form(N, stride, mis, chunks)
    width, t = got.split("/t")
    T = int(t)
    row_bytes = 4 * (N + N // 32 + 1) + 8 * chunks
    assert width == ("vec4" if N % 4 == 0 and stride % 4 == 0 and mis == 0 else "scalar")
    assert 1 <= T <= 64 and (T * row_bytes <= 32768 or T == 1) and (T == 64 or (T + 1) * row_bytes > 32768)
    assert T * row_bytes + 4 * (2048 + 1 + 256) <= 65536        # with the group table: inside 64 KiB of LDS
    raw = ftn.lib.load().ftn_group_sum_form(N, stride, mis, chunks)
    assert raw >> 8 == T and bool(raw & 2) == (width == "vec4") and raw & ~(2 | 0xFF00) == 0


def test_form_of_every_tested_layout(ftn):
    rt = ftn.runtime
    for N in gc.NS:
        for name, members in gc.layouts(N).items():
            c = gc.chunks(members)
            assert rt.group_sum_form_of(N, None, 0, c) == gc.form(N, N, 0, c), (N, name)
            assert gc.tile_rows(N, c) < max(gc.ROWS)            # the largest row count spans more than one tile
            assert rt.group_sum_form_of(N, N + 3, 0, c).startswith("scalar") and \
                rt.group_sum_form_of(N, N + 4, 4, c).startswith("scalar")


def test_form_rejects_bad_arguments(ftn):
    raw = ftn.lib.load().ftn_group_sum_form
    assert raw(0, 8, 0, 1) < 0 and raw(8193, 8193, 0, 1) < 0 and raw(8, 7, 0, 1) < 0
    assert raw(8, 8, 0, -1) < 0 and raw(8, 8, 0, 2049) < 0
    assert raw(8, 8, 2, 1) < 0 and raw(8, 8, 16, 1) < 0 and raw(8, 8, -4, 1) < 0
    assert b"ftn_group_sum_form" in ftn.lib.load().ftn_last_error()
    with pytest.raises(ValueError, match="ftn_group_sum_form"):
        ftn.runtime.group_sum_form_of(9000)
