"""Closure of the block's form table outside the d_model 64 / 128 pipeline slice (host-only: no GPU needed): the
dispatch query ``ftn_timesblock_forms`` against the literal table of ``test_gpu_forms_small.py`` at every tuple the GPU
tests run, and every form that DESIGN's sweep table ("Block forms reachable without switches") lists against the two
matrices that own the forms."""
import functools
import re

from conftest import ROOT
from test_gpu_forms import FORMS_MATRIX, expected_forms
from test_gpu_forms_small import KSETS, NATIVE, SMALL_MATRIX, STUB, WIDE, expected_forms_small


@functools.lru_cache(maxsize=None)
def _plan(C, d_ff, ratio, ks, engine, act):
    import __graft_entry__ as ge
    ftn = ge.load_package()
    sd = ftn.synth.make_inception_params(C, d_ff, KSETS[ks], ratio, seed=0)
    return ftn.pack.pack_inception(sd, C, d_ff, KSETS[ks], ratio, act, engine)[1]


def test_forms_of_every_small_gpu_case(ftn):
    for C, d_ff, ratio, ks, engine, act, adt, aligned in SMALL_MATRIX:
        plan = _plan(C, d_ff, ratio, ks, engine, act)
        want = expected_forms_small(C, d_ff, ratio, ks, engine, act, adt, aligned)
        # the window lengths of the GPU cases, and the benchmark's
        for B, L in ((NATIVE[C >= WIDE]["B"], NATIVE[C >= WIDE]["L"]), (STUB[C >= WIDE]["B"], STUB[C >= WIDE]["L"]), (3, 336)):
            got = ftn.runtime.timesblock_forms(plan, B, L, adt, 0 if aligned else 4)
            assert got == want, (C, d_ff, ratio, ks, engine, act, adt, aligned, L)


def _design_rows():
    """The rows of DESIGN's sweep table: (stage A, conv, stage C, stage E) of every line between its two markers."""
    text = (ROOT / "DESIGN.md").read_text()
    body = text.split("<!-- block-forms-table -->")[1].split("<!-- /block-forms-table -->")[0]
    rows = []
    for line in body.splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        names = [re.fullmatch(r"`([^`]+)`", c) for c in cells]
        if len(cells) >= 5 and names[0] and names[1] and names[2] and names[4]:
            rows.append((names[0].group(1), names[1].group(1), names[2].group(1), cells[3], names[4].group(1)))
    return rows


def test_every_reachable_form_has_an_owner():
    """DESIGN's table is the authority for "every": each conv, stage C and stage E form it lists, and each whole
    row, is produced by an entry of ``FORMS_MATRIX`` or of ``SMALL_MATRIX`` (whose GPU tests assert that it ran)."""
    owned = []
    for C, engine, act, adt, aligned in FORMS_MATRIX:
        owned.append(expected_forms(C, engine, act, adt, aligned))
    for C, d_ff, ratio, ks, engine, act, adt, aligned in SMALL_MATRIX:
        owned.append(expected_forms_small(C, d_ff, ratio, ks, engine, act, adt, aligned))
    rows = _design_rows()
    assert len(rows) >= 80, len(rows)
    for stage in ("conv", "C", "E"):
        have = {f[stage] for f in owned}
        col = {"conv": 1, "C": 2, "E": 4}[stage]
        for r in rows:
            assert r[col] in have, (stage, r[col])
    tuples = {(f["A"], f["conv"], f["C"], f"{int(f['r_keeps_x'])} / {int(f['r_summed'])}", f["E"]) for f in owned}
    for r in rows:
        assert r in tuples, r
    # and nothing is owned that the sweep did not find: a literal edited to a form no shape reaches fails here
    assert tuples == set(rows)
