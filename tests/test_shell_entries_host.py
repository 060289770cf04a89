"""The argument checks of the narrow model-shell entries (d_model <= 128: ``ftn_head_forward``, ``ftn_embed_forward``,
``ftn_embed_rows_strided``, ``ftn_embed_ring``, ``ftn_timeproj_forward`` and the three form queries; csrc/shell_api.hip):
every bad argument is reported with the entry's name before anything touches a device.  The wide and ``_rms`` entries
have their tables in test_shell_wide_host.py and test_embed_rms_host.py.  Every call here is one the checks reject:
the pointers are stand-ins, so a call that passed would launch with them.  No GPU needed."""
import pytest

A, M = 0x10000, 0x10004          # stand-ins for device addresses: 16-byte aligned / 4 bytes past a boundary
BAD_D = {"D = 0": dict(D=0), "D = 6": dict(D=6), "D = 132": dict(D=132)}


def _head(lib, a):
    return lib.ftn_head_forward(a["hidden"], a["rows"], a["S"], a["D"], a["N"], a["wmu"], a["bmu"], a["wsg"], a["bsg"],
                                a["tail"], 0, a["hist"], a["late"], 0, None, 1e-3, a["rate"], a["disp"], a["bad"], None)


def _embed_forward(lib, a):
    return lib.ftn_embed_forward(a["x"], a["x_bs"], a["B"], a["L"], a["N"], a["w"], a["D"], a["add"], a["add_bs"],
                                 a["g"], a["b"], 1e-5, a["out"], None)


def _embed_rows(lib, a):
    return lib.ftn_embed_rows_strided(a["x"], a["x_bs"], a["B"], a["L"], a["N"], a["w"], a["D"], a["out"], a["out_bs"],
                                      None)


def _embed_ring(lib, a):
    return lib.ftn_embed_ring(a["V"], a["B"], a["L"], a["D"], a["head"], a["add"], a["add_bs"], a["g"], a["b"], 1e-5,
                              a["out"], None)


def _timeproj(lib, a):
    return lib.ftn_timeproj_forward(a["seq"], a["B"], a["L"], a["D"], a["wt"], a["bt"], a["S"], a["hid"], None)


def _head_form(lib, a):
    return lib.ftn_head_form(a["N"], a["D"], 0, 0, a["mis"])


def _embed_form(lib, a):
    return lib.ftn_embed_form(a["N"], a["D"], 0, a["x_mis"], a["w_mis"])


def _timeproj_form(lib, a):
    return lib.ftn_timeproj_form(a["L"], a["S"], a["D"], a["mis"])


ENTRIES = {
    "ftn_head_forward": (_head, dict(hidden=A, rows=12, S=4, D=64, N=8, wmu=A, bmu=A, wsg=A, bsg=A, tail=A, hist=4,
                                     late=None, rate=A, disp=A, bad=A), {
        **BAD_D, "null hidden": dict(hidden=None), "null w_mu": dict(wmu=None), "null b_mu": dict(bmu=None),
        "null w_sigma": dict(wsg=None), "null b_sigma": dict(bsg=None), "null tail": dict(tail=None),
        "null rate": dict(rate=None), "null disp": dict(disp=None), "null flag": dict(bad=None),
        "rows = 0": dict(rows=0), "S = 0": dict(S=0), "N = 0": dict(N=0), "rows % S": dict(rows=13),
        "hist = 0": dict(hist=0), "hist > S": dict(hist=5), "hidden misaligned": dict(hidden=M),
        "w_mu misaligned": dict(wmu=M), "w_sigma misaligned": dict(wsg=A + 8)}),
    "ftn_embed_forward": (_embed_forward, dict(x=A, x_bs=24 * 8, B=2, L=24, N=8, w=A, D=64, add=A, add_bs=0, g=A, b=A,
                                               out=A), {
        **BAD_D, "null x": dict(x=None), "null W": dict(w=None), "null out": dict(out=None), "B = 0": dict(B=0),
        "L = 0": dict(L=0), "N = 0": dict(N=0), "out misaligned": dict(out=M), "add misaligned": dict(add=M),
        "gamma misaligned": dict(g=M), "beta misaligned": dict(b=A + 8), "add stride": dict(add_bs=6),
        "gamma without beta": dict(b=None), "beta without gamma": dict(g=None)}),
    "ftn_embed_rows_strided": (_embed_rows, dict(x=A, x_bs=24 * 8, B=2, L=24, N=8, w=A, D=64, out=A, out_bs=24 * 64), {
        **BAD_D, "null x": dict(x=None), "null W": dict(w=None), "null out": dict(out=None), "B = 0": dict(B=0),
        "L = 0": dict(L=0), "N = 0": dict(N=0), "out misaligned": dict(out=M), "out off by 8": dict(out=A + 8),
        "rows overlap": dict(out_bs=23 * 64), "out stride": dict(out_bs=24 * 64 + 2)}),
    "ftn_embed_ring": (_embed_ring, dict(V=A, B=2, L=24, D=64, head=3, add=A, add_bs=0, g=A, b=A, out=A), {
        **BAD_D, "null V": dict(V=None), "null out": dict(out=None), "B = 0": dict(B=0), "L = 0": dict(L=0),
        "head = -1": dict(head=-1), "head = L": dict(head=24), "V misaligned": dict(V=M),
        "out misaligned": dict(out=M), "add misaligned": dict(add=M), "add stride": dict(add_bs=6),
        "gamma without beta": dict(b=None), "beta without gamma": dict(g=None)}),
    "ftn_timeproj_forward": (_timeproj, dict(seq=A, B=2, L=24, D=64, wt=A, bt=A, S=4, hid=A), {
        **BAD_D, "null seq": dict(seq=None), "null wt": dict(wt=None), "null bt": dict(bt=None),
        "null hidden": dict(hid=None), "B = 0": dict(B=0), "L = 0": dict(L=0), "S = 0": dict(S=0),
        "seq misaligned": dict(seq=M), "hidden misaligned": dict(hid=M), "hidden off by 8": dict(hid=A + 8)}),
    "ftn_head_form": (_head_form, dict(N=8, D=64, mis=0), {
        **BAD_D, "N = 0": dict(N=0), "misalign = 5": dict(mis=5), "misalign = 16": dict(mis=16),
        "misalign < 0": dict(mis=-4)}),
    "ftn_embed_form": (_embed_form, dict(N=8, D=64, x_mis=0, w_mis=0), {
        **BAD_D, "N = 0": dict(N=0), "x misalign = 3": dict(x_mis=3), "x misalign = 16": dict(x_mis=16),
        "w misalign < 0": dict(w_mis=-4)}),
    "ftn_timeproj_form": (_timeproj_form, dict(L=24, S=4, D=64, mis=0), {
        **BAD_D, "L = 0": dict(L=0), "S = 0": dict(S=0), "misalign = 2": dict(mis=2), "misalign = 16": dict(mis=16)}),
}
CASES = [(entry, name) for entry, (_, _, bad) in ENTRIES.items() for name in bad]


@pytest.mark.parametrize("entry,name", CASES, ids=[f"{e[4:]}-{n}" for e, n in CASES])
def test_narrow_entries_reject_bad_arguments_before_any_launch(entry, name, ftn):
    """None of these reaches a launch (this test runs without a device): a negative return (no form and no HIP error
    is negative), and the last error starts with the entry's name."""
    lib = ftn.lib.load()
    call, good, bad = ENTRIES[entry]
    assert lib.ftn_timeproj_wide_form(0, 0, 0, 0) < 0                    # another entry's message: none of ours is left
    assert lib.ftn_last_error().decode().startswith("ftn_timeproj_wide_form:")
    rc = call(lib, {**good, **bad[name]})
    assert rc < 0
    msg = lib.ftn_last_error().decode()
    assert msg.startswith(entry + ":"), msg
    with pytest.raises(ValueError, match=entry):
        ftn.lib.check(rc, entry)
