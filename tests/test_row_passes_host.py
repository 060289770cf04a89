"""Row passes, host side (no GPU): ``ftn_timesblock_rows_per_pass`` against ``ftn_timesblock_workspace_bytes``, the
argument checks of the ``_rows`` entry points (all made before anything is enqueued, so they run without a device), and
the row limit the one-shot entry points keep."""
import ctypes as C

import pytest

FAKE = 1 << 20            # a non-null, 256-aligned "device pointer": never dereferenced
L = 48


@pytest.fixture(scope="module")
def setup(ftn):
    lib = ftn.lib.load()
    sd = ftn.synth.make_inception_params(16, 32, [(3, 3)], 2.0, 0)
    _, plan = ftn.pack.pack_inception(sd, 16, 32, [(3, 3)], 2.0, "gelu", "f16x2")
    mg = C.c_int(0)
    pxb = lib.ftn_selector_px_bound(L, 2, L, 1, C.byref(mg))
    assert pxb > 0 and mg.value >= 1
    return lib, plan, mg.value, pxb


def _ws(lib, plan, B, mg, pxb):
    return lib.ftn_timesblock_workspace_bytes(C.byref(plan), B, L, mg, pxb)


def test_exports(ftn):
    assert {"ftn_timesblock_forward_rows", "ftn_timesblock_forward_norm_rows",
            "ftn_timesblock_rows_per_pass"} <= set(ftn.lib.EXPORTS)


@pytest.mark.parametrize("rows", [1, 2, 7, 100, 4097, 65534])
def test_rows_per_pass_is_the_largest_that_fits(setup, rows):
    """A cap of exactly the workspace of ``rows`` rows, and one byte less: the answer is ``rows`` (or more only where
    the rounded-up workspace of more rows is no larger), and never a size whose workspace exceeds the cap."""
    lib, plan, mg, pxb = setup
    cap = _ws(lib, plan, rows, mg, pxb)
    got = lib.ftn_timesblock_rows_per_pass(C.byref(plan), L, mg, pxb, cap)
    assert got >= rows and _ws(lib, plan, got, mg, pxb) <= cap
    assert got == 65535 or _ws(lib, plan, got + 1, mg, pxb) > cap
    below = lib.ftn_timesblock_rows_per_pass(C.byref(plan), L, mg, pxb, cap - 1)
    assert below < rows and (below == 0 or _ws(lib, plan, below, mg, pxb) <= cap - 1)
    assert _ws(lib, plan, below + 1, mg, pxb) > cap - 1


def test_rows_per_pass_edges(setup, ftn):
    lib, plan, mg, pxb = setup
    one = _ws(lib, plan, 1, mg, pxb)
    assert lib.ftn_timesblock_rows_per_pass(C.byref(plan), L, mg, pxb, one - 1) == 0      # one row does not fit
    assert lib.ftn_timesblock_rows_per_pass(C.byref(plan), L, mg, pxb, one) >= 1
    assert lib.ftn_timesblock_rows_per_pass(C.byref(plan), L, mg, pxb, 0) == 65535         # no cap
    assert lib.ftn_timesblock_rows_per_pass(C.byref(plan), L, mg, pxb, 1 << 60) == 65535
    assert lib.ftn_timesblock_rows_per_pass(C.byref(plan), 1, mg, pxb, 0) == 0             # a shape the block cannot run
    assert ftn.runtime.rows_per_pass(plan, L, mg, pxb) == 65535
    # no cap, but rows * pixels per row must stay below 2^31: the answer is the largest pass the block can index
    Lbig = 40000
    mgb = C.c_int(0)
    pxbig = lib.ftn_selector_px_bound(Lbig, 2, Lbig, 1, C.byref(mgb))
    got = lib.ftn_timesblock_rows_per_pass(C.byref(plan), Lbig, mgb.value, pxbig, 0)
    assert 1 <= got < 65535 and got * pxbig <= 0x7fffffff < (got + 1) * pxbig


def _fwd(lib, plan, mg, pxb, B, rows, ws_bytes, flags=0, norm=False):
    if norm:
        return lib.ftn_timesblock_forward_norm_rows(FAKE, FAKE, B, L, C.byref(plan), FAKE, FAKE, FAKE, mg, pxb, flags,
                                                    FAKE, FAKE, 1e-5, FAKE, ws_bytes, None, None, rows)
    return lib.ftn_timesblock_forward_rows(FAKE, FAKE, B, L, C.byref(plan), FAKE, FAKE, FAKE, mg, pxb, 0, flags, FAKE,
                                           ws_bytes, None, None, rows)


@pytest.mark.parametrize("norm", [False, True])
def test_rows_entry_points_reject_bad_arguments_before_any_launch(setup, norm):
    lib, plan, mg, pxb = setup
    B = 100
    need = _ws(lib, plan, B, mg, pxb)
    for rows in (0, 65536, -1):
        rc = _fwd(lib, plan, mg, pxb, B, rows, need, norm=norm)
        assert rc < 0 and b"rows_per_pass" in lib.ftn_last_error(), rows
    # a workspace one byte short of one pass (the pass is min(B, rows_per_pass) rows)
    for rows, n in ((40, 40), (100, 100), (65535, 100)):
        need_n = _ws(lib, plan, n, mg, pxb)
        rc = _fwd(lib, plan, mg, pxb, B, rows, need_n - 1, norm=norm)
        assert rc < 0 and b"workspace" in lib.ftn_last_error(), rows
    # stage A done by the selector's launch: a single pass only
    rc = _fwd(lib, plan, mg, pxb, B, 50, need, flags=1, norm=norm)
    assert rc < 0 and b"single pass" in lib.ftn_last_error()
    rc = _fwd(lib, plan, mg, pxb, B, 50, need, flags=2, norm=norm)
    assert rc < 0 and b"flags" in lib.ftn_last_error()
    rc = _fwd(lib, plan, mg, pxb, 0, 50, need, norm=norm)
    assert rc < 0 and b"bad shape" in lib.ftn_last_error()
    # B beyond the one-shot limit is a shape the _rows entry points take: the next check is the workspace
    rc = _fwd(lib, plan, mg, pxb, 70000, 65535, 256, norm=norm)
    assert rc < 0 and b"workspace" in lib.ftn_last_error()


def test_one_shot_entry_points_keep_their_row_limit(setup, ftn):
    lib, plan, mg, pxb = setup
    big = 1 << 40
    rc = lib.ftn_timesblock_forward(FAKE, FAKE, 65536, L, C.byref(plan), FAKE, FAKE, FAKE, mg, pxb, 0, 0, FAKE, big, None, None)
    assert rc < 0 and b"bad shape" in lib.ftn_last_error()
    rc = lib.ftn_timesblock_forward_norm(FAKE, FAKE, 65536, L, C.byref(plan), FAKE, FAKE, FAKE, mg, pxb, 0, FAKE, FAKE,
                                         1e-5, FAKE, big, None, None)
    assert rc < 0 and b"bad shape" in lib.ftn_last_error()
    rc = lib.ftn_timesblock_forms(C.byref(plan), 65536, L, 0, 0, C.byref(ftn.lib.FtnForms()))
    assert rc < 0 and b"bad shape" in lib.ftn_last_error()
    # the fused finalize + stage A keeps it too (its workspace is one of all B rows)
    rc = lib.ftn_period_finalize_stage_a(FAKE, 1, 65536, FAKE, 65536, L, 2, L, 1, 0, 0, 0.0, FAKE, FAKE, FAKE, FAKE,
                                         C.byref(plan), FAKE, mg, pxb, FAKE, big, None, None, None)
    assert rc < 0 and b"bad shape" in lib.ftn_last_error()


def test_block_policy_without_a_device(ftn, monkeypatch):
    """``TimesBlock._pass_rows``: one pass unless B > 65535 or a knob asks for fewer rows; a cap below one row names
    the bytes."""
    T = ftn.models.timesnet
    lib, plan_args = ftn.lib.load(), (16, 32, [(3, 3)], 2.0)
    blk = T.TimesBlock(16, [(3, 3)], 0.0, "gelu", d_ff=32, bottleneck_ratio=2.0)
    sd = ftn.synth.make_inception_params(*plan_args, 0)
    _, plan = ftn.pack.pack_inception(sd, 16, 32, [(3, 3)], 2.0, "gelu", "f16x2")
    mg = C.c_int(0)
    pxb = lib.ftn_selector_px_bound(L, 2, L, 1, C.byref(mg))
    bounds = lambda: (mg.value, pxb)
    monkeypatch.setattr(T, "_PASS_ENV", (None, None))
    assert blk._pass_rows(7, L, plan, bounds) is None and blk._pass_rows(65535, L, plan, bounds) is None
    assert blk._pass_rows(65536, L, plan, bounds) == 65535
    blk.rows_per_pass = 3
    assert blk._pass_rows(7, L, plan, bounds) == 3 and blk._pass_rows(3, L, plan, bounds) is None
    blk.rows_per_pass = None
    blk.workspace_cap_bytes = _ws(lib, plan, 5, mg.value, pxb)
    rows = blk._pass_rows(100, L, plan, bounds)
    assert rows >= 5 and _ws(lib, plan, rows, mg.value, pxb) <= blk.workspace_cap_bytes
    assert blk._pass_rows(2, L, plan, bounds) is None
    one = _ws(lib, plan, 1, mg.value, pxb)
    blk.workspace_cap_bytes = one - 1
    with pytest.raises(ValueError, match=rf"{one - 1} bytes.*{one} bytes"):
        blk._pass_rows(2, L, plan, bounds)
    blk.workspace_cap_bytes = None
    monkeypatch.setattr(T, "_PASS_ENV", (4, None))                  # FTN_ROWS_PER_PASS=4
    assert blk._pass_rows(9, L, plan, bounds) == 4
    blk.rows_per_pass = 0
    with pytest.raises(ValueError, match="rows_per_pass"):
        blk._pass_rows(9, L, plan, bounds)
