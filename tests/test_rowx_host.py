"""The row exchange of a series-sharded forward (FtnRowExchange, include/flowtimes.h, ABI 13) on the host side: the
ctypes mirror of the struct, the buffer-size formula, the argument checks of every new entry point, and the
unchanged FtnExchange.  No GPU: every call here is refused before anything is enqueued."""
import ctypes as C
import re

import pytest

from conftest import ROOT

CHUNK = 16384


def _header():
    return (ROOT / "include" / "flowtimes.h").read_text()


def _a256(v):
    return (v + 255) // 256 * 256


def test_ctypes_row_exchange_matches_header(ftn):
    X = ftn.lib.FtnRowExchange
    body = re.search(r"typedef struct FtnRowExchange \{(.*?)\} FtnRowExchange;", _header(), re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"^\s*([a-z0-9_]+\*?)\s+([^;]+);", body, re.M):
        for n in names.split(","):
            fields.append((ctype, n.strip()))
    assert fields == [("void*", "slots[FTN_XCHG_MAXWORLD]"), ("int32_t", "world"), ("int32_t", "rank"),
                      ("int32_t", "rows_per_rank"), ("int32_t", "width"), ("int32_t", "kind"),
                      ("int32_t", "reserved")]
    assert [f[0] for f in X._fields_] == ["slots", "world", "rank", "rows_per_rank", "width", "kind", "reserved"]
    assert X.slots.offset == 0 and X.world.offset == 128 and X.rank.offset == 132
    assert X.rows_per_rank.offset == 136 and X.width.offset == 140 and X.kind.offset == 144 and C.sizeof(X) == 152
    assert int(re.search(r"FTN_ROWX_CHUNK (\d+)", _header()).group(1)) == ftn.lib.FTN_ROWX_CHUNK == CHUNK
    assert ftn.lib.load().ftn_abi_version() == 14


def test_exchange_layout_unchanged(ftn):
    X = ftn.lib.FtnExchange
    assert [f[0] for f in X._fields_] == ["slots", "world", "rank", "F_cap", "seq", "mode"]
    assert X.seq.offset == 144 and X.mode.offset == 152 and C.sizeof(X) == 160
    assert ftn.lib.load().ftn_exchange_bytes(2, 1024) == 34048


@pytest.mark.parametrize("world,rows,width", [(1, 1, 4), (2, 2, 336 * 64), (8, 32, 720 * 128), (3, 5, 96 * 12),
                                              (16, 1, 24 * 128)])
def test_rowx_bytes_formula(ftn, world, rows, width):
    slot = rows * width
    nblk = -(-slot // CHUNK)
    half = _a256(world * slot * 4) + _a256(world * nblk * 8)
    assert ftn.lib.load().ftn_rowx_bytes(world, rows, width) == 2 * half + 256


@pytest.mark.parametrize("world,rows,width", [(0, 1, 4), (17, 1, 4), (2, 0, 4), (2, 1, 0), (2, 1, 6), (2, 1, 2),
                                              (2, 1 << 15, 1 << 14)])
def test_rowx_bytes_refuses(ftn, world, rows, width):
    assert ftn.lib.load().ftn_rowx_bytes(world, rows, width) == 0


def _xch(ftn, world=2, rank=0, rows=2, width=8 * 16, kind=0, mapped=True):
    x = ftn.lib.FtnRowExchange()
    x.world, x.rank, x.rows_per_rank, x.width, x.kind = world, rank, rows, width, kind
    for r in range(min(world, ftn.lib.FTN_XCHG_MAXWORLD)):
        x.slots[r] = 4096 * (r + 1) if mapped or r == rank else None
    return x


def _bad_structs(ftn):
    yield "world > 16", _xch(ftn, world=17)
    yield "world 0", _xch(ftn, world=0)
    yield "rank >= world", _xch(ftn, rank=2)
    yield "rank < 0", _xch(ftn, rank=-1)
    yield "width % 4", _xch(ftn, width=130)
    yield "rows 0", _xch(ftn, rows=0)
    yield "kind 2", _xch(ftn, kind=2)
    yield "peer unmapped", _xch(ftn, mapped=False)


def test_every_entry_point_refuses_bad_arguments(ftn):
    lib = ftn.lib.load()
    fake = C.c_void_p(4096)
    for what, x in _bad_structs(ftn):
        ref = C.byref(x)
        assert lib.ftn_rowx_push(fake, ref, None) < 0, what
        assert lib.ftn_rowx_reduce(ref, 8, 16, None, 0, None, None, 1e-5, fake, None) < 0, what
        assert lib.ftn_rowx_gather(ref, fake, None) < 0, what
        assert lib.ftn_rowx_error(ref, None) < 0, what
        assert lib.ftn_rowx_calls(ref, None) < 0, what
        assert b"row exchange" in lib.ftn_last_error(), what
    good = _xch(ftn)
    ref = C.byref(good)
    # null pointers
    assert lib.ftn_rowx_push(None, ref, None) < 0
    assert lib.ftn_rowx_push(fake, None, None) < 0
    assert lib.ftn_rowx_reduce(ref, 8, 16, None, 0, None, None, 1e-5, None, None) < 0
    assert lib.ftn_rowx_reduce(None, 8, 16, None, 0, None, None, 1e-5, fake, None) < 0
    assert lib.ftn_rowx_gather(ref, None, None) < 0
    assert lib.ftn_rowx_gather(None, fake, None) < 0
    assert lib.ftn_rowx_error(None, None) < 0 and lib.ftn_rowx_calls(None, None) < 0
    # misaligned data
    assert lib.ftn_rowx_push(C.c_void_p(4100), ref, None) < 0 and b"aligned" in lib.ftn_last_error()
    assert lib.ftn_rowx_reduce(ref, 8, 16, None, 0, None, None, 1e-5, C.c_void_p(4100), None) < 0
    # the consumer must match the exchange's kind; the reduce's L*D must be the width, D a multiple of 4 <= 128
    assert lib.ftn_rowx_gather(ref, fake, None) < 0 and b"kind 1" in lib.ftn_last_error()
    assert lib.ftn_rowx_reduce(C.byref(_xch(ftn, kind=1)), 8, 16, None, 0, None, None, 1e-5, fake, None) < 0
    assert b"kind 0" in lib.ftn_last_error()
    assert lib.ftn_rowx_reduce(ref, 4, 16, None, 0, None, None, 1e-5, fake, None) < 0          # 4*16 != 128
    assert lib.ftn_rowx_reduce(ref, 32, 6, None, 0, None, None, 1e-5, fake, None) < 0          # D % 4 (and width)
    wide = _xch(ftn, width=2 * 132)
    assert lib.ftn_rowx_reduce(C.byref(wide), 2, 132, None, 0, None, None, 1e-5, fake, None) < 0   # D > 128
    # LayerNorm needs both parameters; add_bstride is 0 or L*D
    assert lib.ftn_rowx_reduce(ref, 8, 16, None, 0, fake, None, 1e-5, fake, None) < 0
    assert lib.ftn_rowx_reduce(ref, 8, 16, fake, 64, None, None, 1e-5, fake, None) < 0
    # allocation: refused before any runtime call for a bad shape
    own = C.c_void_p()
    handle = C.create_string_buffer(64)
    assert lib.ftn_rowx_alloc(17, 1, 4, C.byref(own), handle) < 0
    assert lib.ftn_rowx_alloc(2, 1, 6, C.byref(own), handle) < 0
    assert lib.ftn_rowx_alloc(2, 1, 4, None, handle) < 0
    assert lib.ftn_rowx_alloc(2, 1, 4, C.byref(own), None) < 0
    assert lib.ftn_rowx_open(None, C.byref(own)) < 0 and lib.ftn_rowx_open(handle, None) < 0
    assert lib.ftn_rowx_close(None) == 0 and lib.ftn_rowx_free(None) == 0


def test_series_sharded_timesnet_is_exported(ftn):
    assert callable(ftn.dist.SeriesShardedTimesNet) and callable(ftn.dist.IpcRowExchange)
    assert callable(ftn.dist.series_row_exchanges)
    for name in ("rowx_push", "rowx_reduce", "rowx_gather"):
        assert callable(getattr(ftn.runtime, name))
