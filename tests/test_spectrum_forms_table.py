"""The shapes of the selector front end's time-axis sweep (``tests/test_gpu_spectrum_sweep.py``) and the kernel form
``runtime.spectrum_form`` must report for each (host-only: no GPU needed).  ``SWEEP`` is a literal table, so a change of
``spectrum_geom()`` that moves a shape to another form fails here first; the coverage conditions below keep a later
edit from dropping a length, a pairing or one side of a fit limit of ``csrc/spectrum.hip``."""
from collections import Counter

P, R, Q, T = "k_spectrum", "k_spectrum_row", "k_spectrum_rowq", "k_spectrum_rowq_tiled"
FORMS = (P, R, Q, T)

# (B, L, C, form, float4 loads): every length with (3, 1), (9, 33) and (65, 5); L % 4 == 0 also with (3, 100) and
# (64, 64); then what a form, a load width or an edge of k_median_rows needs
SWEEP = (
    (3, 2, 1, P, 0), (9, 2, 33, P, 0), (65, 2, 5, P, 0),
    (3, 3, 1, P, 0), (9, 3, 33, P, 0), (65, 3, 5, R, 0),
    (3, 4, 1, P, 0), (9, 4, 33, P, 0), (65, 4, 5, R, 0), (3, 4, 100, P, 0), (64, 4, 64, R, 1),
    (3, 5, 1, P, 0), (9, 5, 33, P, 0), (65, 5, 5, R, 0),
    (3, 7, 1, P, 0), (9, 7, 33, P, 0), (65, 7, 5, R, 0), (1, 7, 5, P, 0),
    (3, 8, 1, P, 0), (9, 8, 33, P, 0), (65, 8, 5, Q, 0), (3, 8, 100, T, 1), (64, 8, 64, Q, 1), (64, 8, 5, Q, 0),
    (3, 12, 1, P, 0), (9, 12, 33, P, 0), (65, 12, 5, Q, 0), (3, 12, 100, T, 1), (64, 12, 64, Q, 1), (3, 12, 130, P, 0),
    (3, 28, 1, P, 0), (9, 28, 33, P, 0), (65, 28, 5, Q, 0), (3, 28, 100, T, 1), (64, 28, 64, Q, 1), (1, 28, 64, P, 0),
    (3, 30, 1, P, 0), (9, 30, 33, P, 0), (65, 30, 5, R, 0),
    (3, 31, 1, P, 0), (9, 31, 33, P, 0), (65, 31, 5, R, 0),
    (3, 32, 1, P, 0), (9, 32, 33, P, 0), (65, 32, 5, Q, 0), (3, 32, 100, T, 1), (64, 32, 64, Q, 1),
    (3, 33, 1, P, 0), (9, 33, 33, P, 0), (65, 33, 5, R, 0), (65, 33, 130, P, 0),
    (3, 62, 1, P, 0), (9, 62, 33, P, 0), (65, 62, 5, R, 0),
    (3, 63, 1, P, 0), (9, 63, 33, P, 0), (65, 63, 5, R, 0), (64, 63, 8, R, 1),
    (3, 64, 1, P, 0), (9, 64, 33, P, 0), (65, 64, 5, Q, 0), (3, 64, 100, T, 1), (64, 64, 64, Q, 1), (3, 64, 127, T, 0),
    (1, 64, 100, T, 1),
    (3, 65, 1, P, 0), (9, 65, 33, P, 0), (65, 65, 5, R, 0), (64, 65, 64, R, 1), (3, 65, 130, P, 0),
    (3, 66, 1, P, 0), (9, 66, 33, P, 0), (65, 66, 5, R, 0),
    (3, 124, 1, P, 0), (9, 124, 33, P, 0), (65, 124, 5, Q, 0), (3, 124, 100, T, 1), (64, 124, 64, Q, 1),
    (3, 126, 1, P, 0), (9, 126, 33, P, 0), (65, 126, 5, R, 0),
    (3, 127, 1, P, 0), (9, 127, 33, P, 0), (65, 127, 5, R, 0),
    (3, 128, 1, P, 0), (9, 128, 33, P, 0), (65, 128, 5, Q, 0), (3, 128, 100, T, 1), (64, 128, 64, Q, 1),
    (9, 128, 130, P, 0),
    (3, 129, 1, P, 0), (9, 129, 33, P, 0), (65, 129, 5, R, 0), (1, 129, 33, P, 0),
    (3, 130, 1, P, 0), (9, 130, 33, P, 0), (65, 130, 5, R, 0),
    (3, 250, 1, P, 0), (9, 250, 33, P, 0), (65, 250, 5, R, 0), (64, 250, 64, R, 1),
    (3, 255, 1, P, 0), (9, 255, 33, P, 0), (65, 255, 5, R, 0), (70, 255, 24, R, 1),
    (3, 256, 1, P, 0), (9, 256, 33, P, 0), (65, 256, 5, Q, 0), (3, 256, 100, T, 1), (64, 256, 64, Q, 1),
    (3, 257, 1, P, 0), (9, 257, 33, P, 0), (65, 257, 5, R, 0),
    (3, 336, 1, P, 0), (9, 336, 33, P, 0), (65, 336, 5, Q, 0), (3, 336, 100, T, 1), (64, 336, 64, Q, 1),
    (1, 336, 100, T, 1), (9, 336, 70, T, 0),
    # C = 64 at the LDS limit: the four quarter-fold planes no longer fit at L = 400, where k_spectrum_row still does;
    # neither at 500
    (3, 400, 1, P, 0), (9, 400, 33, P, 0), (65, 400, 5, Q, 0), (3, 400, 100, T, 1), (64, 400, 64, R, 1),
    (3, 500, 1, P, 0), (9, 500, 33, P, 0), (65, 500, 5, Q, 0), (3, 500, 100, T, 1), (64, 500, 64, P, 0),
    (3, 500, 130, P, 0),
    (3, 720, 1, P, 0), (9, 720, 33, P, 0), (65, 720, 5, Q, 0), (3, 720, 100, T, 1), (64, 720, 64, P, 0),
    # the wave limit: 16 blocks of 32 bins (L = 1023, F = 512) | 17 (1026); 2 x 8 blocks per parity (1020) | 2 x 9
    # (1024).  (65, 1020, 100): B F = 33215 rows, so k_median_rows' last workgroup is ragged
    (3, 1020, 1, P, 0), (9, 1020, 33, P, 0), (65, 1020, 5, Q, 0), (3, 1020, 100, T, 1), (64, 1020, 64, P, 0),
    (65, 1020, 100, T, 1),
    (3, 1023, 1, P, 0), (9, 1023, 33, P, 0), (65, 1023, 5, R, 0), (64, 1023, 64, P, 0),
    (3, 1024, 1, P, 0), (9, 1024, 33, P, 0), (65, 1024, 5, P, 0), (3, 1024, 100, P, 0), (64, 1024, 64, P, 0),
    (64, 1024, 100, P, 0), (1, 1024, 130, P, 0),
    (3, 1026, 1, P, 0), (9, 1026, 33, P, 0), (65, 1026, 5, P, 0), (1, 1026, 1, P, 0),
)

LENGTHS = (2, 3, 4, 5, 7, 8, 12, 28, 30, 31, 32, 33, 62, 63, 64, 65, 66, 124, 126, 127, 128, 129, 130, 250, 255, 256,
           257, 336, 400, 500, 720, 1020, 1023, 1024, 1026)


def test_every_sweep_shape_reports_its_pinned_form(ftn):
    for B, L, C, form, vec in SWEEP:
        assert ftn.runtime.spectrum_form(B, L, C) == (form, bool(vec)), (B, L, C)


def test_sweep_has_no_duplicates_and_stays_small():
    shapes = [s[:3] for s in SWEEP]
    assert max(Counter(shapes).values()) == 1
    assert len(SWEEP) < 200, len(SWEEP)


def test_every_form_and_load_width_occurs():
    have = {(f, bool(v)) for _, _, _, f, v in SWEEP}
    assert (P, False) in have and (P, True) not in have          # k_spectrum has only scalar loads
    for form in (R, Q, T):
        assert (form, True) in have and (form, False) in have, form


def test_both_sides_of_every_fit_limit():
    """With B >= 64 a shape leaves the row-resident forms where the workgroup would need more than 16 waves or more
    LDS than it can be given; the channel-tiled form has a wave limit of its own."""
    table = {s[:3]: s[3] for s in SWEEP}
    at = lambda L, C: {f for (B, l, c), f in table.items() if B >= 64 and (l, c) == (L, C)}
    assert at(1023, 5) == {R} and at(1026, 5) == {P}             # nfb = 16 | 17 waves
    assert at(1020, 5) == {Q} and at(1024, 5) == {P}             # 2 nfq = 16 | 18 waves
    assert at(400, 64) <= {R, Q} and at(400, 64) and at(500, 64) == {P}      # LDS
    assert at(1020, 100) == {T} and at(1024, 100) == {P}         # tiled: 2 nfq = 16 | 18 waves


def test_lengths_and_pairings():
    shapes = {s[:3] for s in SWEEP}
    assert set(LENGTHS) <= {L for _, L, _ in shapes}
    for L in LENGTHS:
        for B, C in ((3, 1), (9, 33), (65, 5)) + (((3, 100), (64, 64)) if L % 4 == 0 else ()):
            assert (B, L, C) in shapes, (B, L, C)
    for which, sel in (("B = 1", lambda s: s[0] == 1), ("C = 130", lambda s: s[2] == 130)):
        ls = {s[1] for s in shapes if sel(s)}
        assert len(ls) >= 4 and min(ls) < 32 and max(ls) > 256, (which, sorted(ls))
