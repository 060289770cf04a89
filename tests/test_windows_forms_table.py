"""The kernel form of ``ftn_window_batch`` (``ftn_window_batch_form``, host-only: the launch dispatches through the same
function) pinned for every shape of the GPU sweep (tests/windows_checks.py) in both layouts: dense tables, column
slices with a row stride that is and is not a multiple of 4, and tables and outputs one float off the 16-byte grid.
The 16-byte form is pinned where the header's conditions hold and the 4-byte form everywhere else."""
import pytest

import windows_checks as wc


def _outs(shape, layout):
    outs = ["x", "y", "mask"] + (["x_mark", "y_mark"] if shape["F"] else [])
    if layout == "series":
        outs += (["static"] if shape["Fs"] else []) + (["id"] if shape["ids"] else [])
    return tuple(outs)


def test_literal_forms(ftn):
    f = ftn.runtime.window_batch_form_of
    T = wc.TILE
    assert T == (ftn.lib.FTN_WIN_TILE_SERIES, ftn.lib.FTN_WIN_TILE_STEPS)
    # the pipeline shape: N = 193 is odd, nothing moves 16 bytes
    assert f("series", 193, 28, 7) == {"vec": (), "tile": T}
    assert f("series", 192, 28, 7) == {"vec": ("x",), "tile": T}                         # H = 7: y and mask stay scalar
    assert f("series", 192, 28, 8, F=4, outs=wc.PIECES[:5]) == {"vec": wc.PIECES[:5], "tile": T}
    assert f("series", 192, 28, 8, F=3, outs=wc.PIECES[:5]) == {"vec": ("x", "y", "mask"), "tile": T}
    assert f("series", 192, 30, 8) == {"vec": ("y", "mask"), "tile": T}                  # L = 30: x stays scalar
    assert f("series", 192, 28, 8, has_mask=False) == {"vec": ("x", "y", "mask"), "tile": T}         # ones: stored only
    assert f("series", 192, 28, 8, x_stride=194) == {"vec": ("mask",), "tile": T}
    assert f("series", 192, 28, 8, x_stride=196, m_stride=200) == {"vec": ("x", "y", "mask"), "tile": T}
    assert f("series", 192, 28, 8, misalign={"X": 4}) == {"vec": ("mask",), "tile": T}
    assert f("series", 192, 28, 8, misalign={"M": 8}) == {"vec": ("x", "y"), "tile": T}
    assert f("series", 192, 28, 8, misalign={"y": 12}) == {"vec": ("x", "mask"), "tile": T}
    assert f("series", 192, 28, 8, F=4, outs=("x_mark", "id")) == {"vec": ("x_mark",), "tile": None}
    assert f("series", 192, 28, 8, F=4, outs=("y_mark",), misalign={"marks": 4}) == {"vec": (), "tile": None}
    assert f("series", 192, 28, 8, F=4, outs=("y_mark",), marks_stride=6) == {"vec": (), "tile": None}
    # the bench layout: rows of N = 512 series, whatever L and H are
    assert f("wide", 512, 336, 96) == {"vec": ("x", "y", "mask"), "tile": None}
    assert f("wide", 512, 335, 95) == {"vec": ("x", "y", "mask"), "tile": None}
    assert f("wide", 510, 336, 96) == {"vec": (), "tile": None}
    assert f("wide", 512, 336, 96, x_stride=514) == {"vec": ("mask",), "tile": None}
    assert f("wide", 512, 336, 96, misalign={"x": 4}) == {"vec": ("y", "mask"), "tile": None}


@pytest.mark.parametrize("N", wc.SWEEP_N)
def test_sweep_forms(N, ftn):
    f = ftn.runtime.window_batch_form_of
    seen = set()
    for shape in wc.sweep(N):
        L, H, F = shape["L"], shape["H"], shape["F"]
        for layout in ("series", "wide"):
            outs = _outs(shape, layout)
            variants = [dict(), dict(x_stride=N + 8, m_stride=N + 12, marks_stride=F + 4 if F else None),
                        dict(x_stride=N + 3, m_stride=N + 1, marks_stride=F + 1 if F else None),
                        dict(misalign={"X": 4}), dict(misalign={"M": 4} if shape["mask"] else {}),
                        dict(misalign={"x": 4, "mask": 4}), dict(misalign={"y": 4})] + (
                            [dict(misalign={"marks": 4}), dict(misalign={"x_mark": 4})] if F else [])
            for kw in variants:
                got = f(layout, N, L, H, F=F, Fs=shape["Fs"], outs=outs, has_mask=shape["mask"], **kw)
                want = wc.want_form(layout, N, L, H, F=F, outs=outs, has_mask=shape["mask"], **kw)
                assert got == want, (layout, shape, kw)
                seen.add(got["vec"])
            for name in outs[:5]:                               # a piece asked for alone takes the form it takes in company
                alone = f(layout, N, L, H, F=F, Fs=shape["Fs"], outs=(name,), has_mask=shape["mask"])
                together = f(layout, N, L, H, F=F, Fs=shape["Fs"], outs=outs, has_mask=shape["mask"])
                assert (name in alone["vec"]) == (name in together["vec"]), (layout, shape, name)
    if N % 4:
        assert all(not ({"x", "y", "mask"} & set(v)) for v in seen)             # an odd row never moves 16 bytes
    else:
        assert any({"x", "y", "mask"} <= set(v) for v in seen) and () in seen
