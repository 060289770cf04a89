"""The capturable mode of the multi-GPU exchange (FtnExchange.mode, include/flowtimes.h) on the host side: the ctypes
mirror of the struct, the argument checks of the C ABI for the new mode, the unchanged buffer size and the
``ShardedTimesNet(exchange=)`` signature.  No GPU: every call here is refused before anything is enqueued."""
import ctypes as C
import re

import pytest
import torch

from conftest import ROOT


def _header():
    return (ROOT / "include" / "flowtimes.h").read_text()


def test_ctypes_exchange_matches_header(ftn):
    X = ftn.lib.FtnExchange
    body = re.search(r"typedef struct FtnExchange \{(.*?)\} FtnExchange;", _header(), re.S).group(1)
    # the header's fields, in order, with their C types
    fields = []
    for ctype, names in re.findall(r"^\s*([a-z0-9_]+\*?)\s+([^;]+);", body, re.M):
        for n in names.split(","):
            fields.append((ctype, n.strip()))
    assert fields == [("void*", "slots[FTN_XCHG_MAXWORLD]"), ("int32_t", "world"), ("int32_t", "rank"),
                      ("int32_t", "F_cap"), ("uint64_t", "seq"), ("int32_t", "mode")]
    assert [f[0] for f in X._fields_] == ["slots", "world", "rank", "F_cap", "seq", "mode"]
    want = {"slots": C.c_void_p * ftn.lib.FTN_XCHG_MAXWORLD, "world": C.c_int32, "rank": C.c_int32,
            "F_cap": C.c_int32, "seq": C.c_uint64, "mode": C.c_int32}
    for name, ctype in X._fields_:
        assert C.sizeof(ctype) == C.sizeof(want[name]), name
    # C layout on LP64: 16 pointers, three int32, the uint64 aligned to 8, the new int32, tail padding to 8
    assert X.slots.offset == 0 and X.world.offset == 128 and X.rank.offset == 132 and X.F_cap.offset == 136
    assert X.seq.offset == 144 and X.mode.offset == 152 and C.sizeof(X) == 160
    assert int(re.search(r"FTN_XCHG_MAXWORLD (\d+)", _header()).group(1)) == ftn.lib.FTN_XCHG_MAXWORLD
    assert X().mode == 0                                          # a zeroed struct is today's protocol


def _spectrum(lib, xch):
    fake = C.c_void_p(256)
    return lib.ftn_period_spectrum(fake, 2, 48, 16, fake, fake, fake, None, C.byref(xch), None)


def test_mode1_needs_no_host_sequence_number(ftn):
    lib = ftn.lib.load()
    xch = ftn.lib.FtnExchange()
    xch.world, xch.rank, xch.F_cap, xch.seq, xch.mode = 2, 0, 64, 0, 1
    xch.slots[0] = 256
    # seq == 0 passes in mode 1 (the device counter is the sequence); the unmapped peer slot is what is refused
    assert _spectrum(lib, xch) < 0 and b"not mapped" in lib.ftn_last_error()
    # the same struct in mode 0 is refused for its sequence number, as before
    xch.mode = 0
    assert _spectrum(lib, xch) < 0 and b"bad exchange" in lib.ftn_last_error()


@pytest.mark.parametrize("mode", [2, -1])
def test_unknown_mode_is_refused(ftn, mode):
    lib = ftn.lib.load()
    fake = C.c_void_p(256)
    xch = ftn.lib.FtnExchange()
    xch.world, xch.rank, xch.F_cap, xch.seq, xch.mode = 1, 0, 64, 1, mode
    xch.slots[0] = 256
    assert _spectrum(lib, xch) < 0 and b"exchange" in lib.ftn_last_error()
    rc = lib.ftn_period_finalize(fake, 1, 2, fake, 2, 48, 2, 48, 1, 0, 0, 0.0, fake, fake, fake, None, C.byref(xch))
    assert rc < 0 and b"exchange" in lib.ftn_last_error()
    sd = ftn.synth.make_inception_params(16, 32, [(3, 3)], 2.0, 0)
    _, plan = ftn.pack.pack_inception(sd, 16, 32, [(3, 3)], 2.0, "gelu", "f16x2")
    rc = lib.ftn_period_finalize_stage_a(None, 1, 2, fake, 2, 48, 2, 48, 1, 0, 0, 0.0, fake, fake, fake, fake,
                                         C.byref(plan), fake, 1, 0, fake, 0, None, None, C.byref(xch))
    assert rc < 0 and b"exchange" in lib.ftn_last_error()
    assert lib.ftn_exchange_calls(C.byref(xch), None) < 0     # the counter read is for mode 1 only


def test_stage_a_check_accepts_mode1_without_seq(ftn):
    lib = ftn.lib.load()
    fake = C.c_void_p(256)
    sd = ftn.synth.make_inception_params(16, 32, [(3, 3)], 2.0, 0)
    _, plan = ftn.pack.pack_inception(sd, 16, 32, [(3, 3)], 2.0, "gelu", "f16x2")
    xch = ftn.lib.FtnExchange()
    xch.world, xch.rank, xch.F_cap, xch.seq, xch.mode = 1, 0, 64, 0, 1
    xch.slots[0] = 256
    # the exchange passes; the (deliberately empty) workspace is the next check to refuse the call
    rc = lib.ftn_period_finalize_stage_a(None, 1, 2, fake, 2, 48, 2, 48, 1, 0, 0, 0.0, fake, fake, fake, fake,
                                         C.byref(plan), fake, 1, 0, fake, 0, None, None, C.byref(xch))
    assert rc < 0 and b"workspace" in lib.ftn_last_error()
    xch.mode = 0
    rc = lib.ftn_period_finalize_stage_a(None, 1, 2, fake, 2, 48, 2, 48, 1, 0, 0, 0.0, fake, fake, fake, fake,
                                         C.byref(plan), fake, 1, 0, fake, 0, None, None, C.byref(xch))
    assert rc < 0 and b"exchange" in lib.ftn_last_error()


def test_exchange_bytes_unchanged_and_counter_in_error_line(ftn):
    lib = ftn.lib.load()
    # two halves of [world][F_cap] doubles + [world][32] sequence words, each rounded up to 256 bytes, + one line
    assert lib.ftn_exchange_bytes(2, 1024) == 34048
    assert lib.ftn_exchange_bytes(16, 1024) == 270592
    assert lib.ftn_exchange_bytes(2, 64) == 2 * 1536 + 256
    for world, f_cap in ((1, 64), (2, 1024), (16, 1024), (3, 169)):
        n = lib.ftn_exchange_bytes(world, f_cap)
        off = lib.ftn_exchange_counter_offset(world, f_cap)
        assert off == n - 256 + 8 and off % 8 == 0 and off + 8 <= n
    assert lib.ftn_exchange_counter_offset(99, 64) == 0


def test_sharded_timesnet_accepts_exchange(ftn):
    model = ftn.models.TimesNet(input_len=48, pred_len=8, d_model=16, n_layers=1, k_periods=2, kernel_set=[(3, 3)],
                                dropout=0.0, activation="gelu", mode="direct")

    class _X:                                                     # stands in for an IpcExchange (needs a GPU)
        capturable = True

    x = _X()
    runner = ftn.dist.ShardedTimesNet(model, exchange=x)
    assert runner.exchange is x and runner.group is None
    assert ftn.dist.ShardedTimesNet(model).exchange is None
    # GraphedForward's deferred-check attributes reach the wrapped model
    runner._defer_checks = True
    assert model._defer_checks is True
    runner._defer_checks = False
    flag = torch.zeros(1, dtype=torch.int32)
    runner._pending_bad = flag
    assert model._pending_bad is flag and runner._pending_bad is flag
    runner.check_outputs()                                        # a zero flag: nothing to raise
    assert model._pending_bad is None
