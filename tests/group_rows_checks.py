"""What the tests of series groups along another axis share: the oracle (``groups_checks.group_sum`` on the moved
axis, moved back), an independent statement of the form rule of include/flowtimes.h (``ftn_group_sum_rows_form``), and
test values with the members along a chosen axis."""
import numpy as np

import groups_checks as gc

SS = [1, 5, 33, 193, 260]
KINDS = ("counts", "big", "normal", "special")


def oracle(x, members, axis):
    """``x`` with the members along ``axis`` -> the same array with the G totals along ``axis``."""
    return np.ascontiguousarray(np.moveaxis(gc.group_sum(np.moveaxis(x, axis, -1), members), -1, axis))


def values(g, shape, axis, members):
    """``gc.values`` (the NaN and inf of ``special`` sit in two members) with the members along ``axis`` of ``shape``."""
    axis %= len(shape)
    moved = tuple(n for d, n in enumerate(shape) if d != axis) + (shape[axis],)
    return {k: np.ascontiguousarray(np.moveaxis(v, -1, axis)) for k, v in gc.values(g, moved, members).items()}


def tile_cols(inner):
    """The header's rule: the whole row up to 64 columns, a multiple of 4 from 4 on."""
    t = min(inner, 64)
    return t - t % 4 if t >= 4 else t


def passes(inner, n_chunks):
    """The header's rule: the fp64 chunk sums of a pass stay within 32 KiB."""
    per = 32768 // (8 * tile_cols(inner))
    return max(1, -(-n_chunks // per))


def form(inner, member_stride, outer_stride, misalign):
    """The form name ``runtime.group_sum_rows_form_of`` must give (its chunk count moves only the passes)."""
    vec = inner % 4 == 0 and member_stride % 4 == 0 and outer_stride % 4 == 0 and misalign % 16 == 0
    return f"{'vec4' if vec else 'scalar'}/i{tile_cols(inner)}"


def form_word(inner, member_stride, outer_stride, misalign, n_chunks):
    """The word ``ftn_group_sum_rows_form`` must return."""
    vec = form(inner, member_stride, outer_stride, misalign).startswith("vec4")
    return (2 if vec else 0) | tile_cols(inner) << 8 | passes(inner, n_chunks) << 16
