"""``tests/ws_poison.py`` on CPU tensors, so that the helper cannot pass silently on the GPU: the interior it hands out
is aligned and exactly as long as asked, ``check_guards`` notices one byte written on either side, each pattern decodes
as the helper's docstring says, and the case tables of ``test_gpu_workspace_hygiene.py`` name every block form."""
import math

import pytest
import torch

import ws_poison
from ws_poison import GUARD, PATTERNS, SENTINEL, check_guards, pattern_tensor, poisoned_workspace

CPU = torch.device("cpu")


@pytest.mark.parametrize("need", [1, 255, 256, 1024 + 7, 3 * 4096, 1 << 20])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_interior_is_aligned_exact_and_filled(pattern, need):
    log = []
    ws = poisoned_workspace(pattern, log)(CPU, need)
    assert ws.dtype == torch.uint8 and ws.numel() == need and ws.is_contiguous()
    assert ws.data_ptr() % 256 == 0
    assert bool((ws == pattern).all())
    assert len(log) == 1 and log[0][1] == need
    outer = log[0][0]
    assert outer.numel() == need + 2 * GUARD and outer.data_ptr() + GUARD == ws.data_ptr()
    assert bool((outer[:GUARD] == SENTINEL).all()) and bool((outer[GUARD + need:] == SENTINEL).all())
    assert check_guards(log) == 1
    ws.fill_(0x11)                                               # the whole interior is the caller's to write
    ws[0], ws[-1] = 0x22, 0x33
    check_guards(log)


def test_guard_bytes_and_patterns_are_distinct_and_a_multiple_of_the_alignment():
    assert GUARD == 4096 and GUARD % ws_poison.ALIGN == 0 and ws_poison.ALIGN == 256
    assert PATTERNS == (0x00, 0xFF, 0x7B) and SENTINEL not in PATTERNS


@pytest.mark.parametrize("where", ["one past the last byte", "one before the first byte", "last guard byte",
                                   "first guard byte"])
def test_check_guards_fails_on_one_byte_outside(where):
    log = []
    alloc = poisoned_workspace(0xFF, log)
    first, ws, last = alloc(CPU, 512), alloc(CPU, 1000), alloc(CPU, 256)
    check_guards(log)
    outer, need = log[1]
    assert outer.data_ptr() + GUARD == ws.data_ptr() and need == 1000
    at = {"one past the last byte": GUARD + need, "one before the first byte": GUARD - 1,
          "last guard byte": 2 * GUARD + need - 1, "first guard byte": 0}[where]
    outer[at] = 0
    with pytest.raises(AssertionError, match="workspace 1 "):
        check_guards(log)
    outer[at] = SENTINEL
    check_guards(log)
    del first, last


def test_a_write_of_the_guard_byte_value_inside_is_no_violation_but_any_other_value_outside_is():
    log = []
    ws = poisoned_workspace(0x00, log)(CPU, 64)
    ws.fill_(SENTINEL)
    check_guards(log)
    log[0][0][GUARD + 64] = SENTINEL ^ 1                         # one bit of the first byte behind the interior
    with pytest.raises(AssertionError):
        check_guards(log)


def _views(pattern, n=64):
    raw = pattern_tensor(pattern, (n,), torch.uint8, CPU)
    return raw.view(torch.float32), raw.view(torch.bfloat16), raw.view(torch.float16), raw.view(torch.int32)


def test_pattern_zero_decodes_as_zero():
    for v in _views(0x00):
        assert bool((v == 0).all())


def test_pattern_ff_is_nan_in_every_float_format_and_minus_one_as_int32():
    f32, bf16, f16, i32 = _views(0xFF)
    assert bool(f32.isnan().all()) and bool(bf16.isnan().all()) and bool(f16.isnan().all())
    assert bool((i32 == -1).all())
    # NaN times 0 is NaN: a reader that masks by multiplying cannot hide it
    assert bool((f32 * 0.0).isnan().all()) and bool((f16 * 0.0).isnan().all())


def test_pattern_7b_is_huge_as_fp32_and_bf16_and_inside_the_fp16_range():
    f32, bf16, f16, i32 = _views(0x7B)
    assert bool(torch.isfinite(f32).all()) and bool(torch.isfinite(bf16).all()) and bool(torch.isfinite(f16).all())
    assert math.isclose(float(f32[0]), 1.3e36, rel_tol=0.02) and math.isclose(float(bf16[0]), 1.3e36, rel_tol=0.02)
    assert float(f32[0]) > 65504.0 and float(bf16[0]) > 65504.0       # ... so as a piece source it is out of range
    # 0x7B7B as fp16: exponent 30, mantissa 0x37B = 2^15 (1 + 891 / 1024)
    assert float(f16[0]) == 32768.0 + 32.0 * 0x37B == 61280.0 and float(f16[0]) < 65504.0
    assert bool((f16 == f16[0]).all()) and bool((i32 == 0x7B7B7B7B).all())


def test_pattern_tensor_fills_every_byte_of_any_dtype():
    for dtype, shape in ((torch.int32, (103,)), (torch.float32, (5, 16)), (torch.float64, (3,))):
        t = pattern_tensor(0x7B, shape, dtype, CPU)
        assert t.shape == shape and t.dtype == dtype and t.is_contiguous()
        assert bool((t.view(torch.uint8) == 0x7B).all())


def test_hygiene_cases_name_every_block_form():
    """Each GPU case asserts ``_last_forms`` against these tables, so a form named here is a form that ran."""
    import test_gpu_forms as wide
    import test_gpu_forms_small as small
    import test_gpu_workspace_hygiene as hyg

    seen = set()
    for C, d_ff, ratio, ks, engine, selector in hyg.HYGIENE_SMALL:
        for fused in (False, True) if selector == "native" else (False,):
            f = small.expected_forms_small(C, d_ff, ratio, ks, engine, "gelu", 0, True, fused)
            seen |= {f["A"], f["conv"], f["C"], f["E"]}
    for C, engine, selector in hyg.HYGIENE_WIDE:
        f = wide.expected_forms(C, engine, "gelu", 0, True, selector == "native")
        seen |= {f["A"], f["conv"], f["C"], f["E"]}
    for C, d_ff, ratio, ks, engine, dtype in hyg.HYGIENE_HALF:
        f = small.expected_forms_small(C, d_ff, ratio, ks, engine, "gelu", 1, True, True)
        seen |= {f["A"].replace("k_finalize_pw<", "k_pw<1,"), f["conv"], f["C"], f["E"]}
    named = {n for row in small.SMALL_FORMS.values() for n in (row[0], row[1], row[2], row[5])}
    named |= {n for row in wide.TABLE_FORMS.values() for n in row}
    assert named <= seen, sorted(named - seen)
    # every fp32 row of SMALL_FORMS under both selectors, the four engines at both widths, every half row per dtype
    assert len(hyg.HYGIENE_SMALL) == 2 * len(small.SMALL_BASE) + len(small.TILED_ROWS)
    assert {(c[0], c[1]) for c in hyg.HYGIENE_WIDE} == {(C, e) for C in (64, 128) for e in ("f32", "bf16x3", "f16x2", "bf16")}
    assert len(hyg.HYGIENE_HALF) == 2 * len(small.SMALL_HALF)
