"""The instruction census of the position-major stage C at the bench form (f16x2, d_model 64: DESIGN §4 "Round 3:
what bounds stage C now").  Its group loop is bound by instruction issue, so what the compiler emits there is pinned:
no ``v_perm_b32`` (the fragment repacks that a ``__bf16`` vector crossing a block boundary costs), the MFMA count of
the algorithm, and no more spills than the prefetch form was tuned to.  Needs ``hipcc``, not a GPU."""
import importlib.util
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
UNIT = ROOT / "flow-timesnet_amd" / "csrc" / "stagec_pos.hip"
# k_mlp_pos<ACT, XVEC, NS, SKM, SCP, NOA, NOR, NWV, GB, PF>: GELU, both x alignments, f16x2, d_model 64, prefetch
BENCH_FORMS = ["k_mlp_pos<0, true, 2, 2, 2, 3, 4, 4, 5, 1>", "k_mlp_pos<0, false, 2, 2, 2, 3, 4, 4, 5, 1>"]


def _tool():
    spec = importlib.util.spec_from_file_location("isa_census", ROOT / "tools" / "isa_census.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_classify_and_parse():
    t = _tool()
    assert [t.classify(m) for m in ("v_mfma_f32_16x16x32_f16", "v_perm_b32", "ds_read_b128", "global_load_dwordx4",
                                    "scratch_load_dword", "s_waitcnt", "foo")] == ["mfma", "valu", "lds", "vmem", "vmem",
                                                                                   "salu", None]
    asm = """
	.amdhsa_kernel kern
	.end_amdhsa_kernel
kern:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_lshrrev_b32_e32 v1, 16, v0            ; a comment
.LBB0_1:
	ds_read_b128 v[0:3], v4
	v_mfma_f32_16x16x32_f16 v[0:3], v[4:7], v[8:11], v[0:3]
	v_perm_b32 v1, v2, v3, s0
	global_store_dword v0, v1, s[0:1]
	s_cbranch_scc1 .LBB0_1
	s_endpgm
.Lfunc_end0:
other:
	v_perm_b32 v1, v2, v3, s0
amdhsa.kernels:
  - .agpr_count:     0
    .name:           kern
    .sgpr_spill_count: 0
    .vgpr_count:     12
    .vgpr_spill_count: 3
"""
    k = t.parse_asm(asm)
    assert list(k) == ["kern"]
    k = k["kern"]
    assert [b["label"] for b in k["blocks"]] == ["entry", ".LBB0_1"]
    assert (k["blocks"][0]["salu"], k["blocks"][0]["valu"]) == (1, 1)
    assert {c: k["blocks"][1][c] for c in t.CLASSES} == {"mfma": 1, "valu": 1, "lds": 1, "vmem": 1, "salu": 2}
    assert k["mnemonics"]["v_lshrrev_b32"] == 1 and k["mnemonics"]["v_perm_b32"] == 1
    assert (k["vgpr_count"], k["vgpr_spill_count"], k["mfma"]) == (12, 3, 1)


def test_bench_form_census():
    t = _tool()
    hipcc = t.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    kernels = t.census(UNIT, ["-DFTN_POS_DEV=1"], hipcc)
    for form in BENCH_FORMS:
        assert form in kernels, sorted(kernels)
        k = kernels[form]
        t.report({form: k}, min_mfma=4, count=["v_perm_b32", "v_lshrrev_b32"])
        assert k["mnemonics"].get("v_perm_b32", 0) == 0
        assert k["mfma"] == 129
        assert k["vgpr_spill_count"] <= 13
