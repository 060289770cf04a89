"""The TimesBlock call path, host side (no GPU): the first error of bad calls to ``ftn_period_finalize``,
``ftn_period_finalize_stage_a``, ``ftn_timesblock_forms`` and the four forwards, ``ftn_selector_px_bound`` under the
constructor clamps, and the ``runtime.StageA`` record.

Every call of the message table fails in argument checking, before anything is enqueued, so the "device pointers" are
never dereferenced.  ``EXPECT`` holds ``ftn_last_error()`` of each call as the commit before the shared prologue,
argument fill and plan check returned it (recorded from a build of that commit): the text and, for a call with two
faults, which check speaks first are part of the C ABI's behaviour."""
import copy
import ctypes as C

import pytest
import torch

FAKE = 1 << 20            # a non-null, 256-aligned "device pointer": never dereferenced
L = 48
B = 2
LONG = 8192               # F = 4097 bins: one 16-bin step beyond the finalize workgroup's 48 KiB of LDS (L = 8190 fits)


@pytest.fixture(scope="module")
def env(ftn):
    lib = ftn.lib.load()
    sd = ftn.synth.make_inception_params(16, 32, [(3, 3)], 2.0, 0)
    _, plan = ftn.pack.pack_inception(sd, 16, 32, [(3, 3)], 2.0, "gelu", "f16x2")
    sd1 = ftn.synth.make_inception_params(16, 16, [(3, 3)], 1.0, 0)
    _, single = ftn.pack.pack_inception(sd1, 16, 16, [(3, 3)], 1.0, "gelu", "f32")      # single-conv block (mode 1)

    def variant(**fields):
        p = copy.copy(plan)                     # ctypes structures copy by value
        for name, v in fields.items():
            setattr(p, name, v)
        return p

    plans = {"ok": plan, "single": single, "nbr0": variant(nbr=0), "mp8": variant(MP=8), "pad": variant(CP=plan.CP + 8),
             None: None}
    xch = ftn.lib.FtnExchange()                 # sequence number 0: refused
    xch.world, xch.rank, xch.F_cap, xch.seq = 2, 0, 64, 0
    xch.slots[0] = FAKE
    return lib, plans, xch


def _bounds(lib, length):
    mg = C.c_int(0)
    pxb = lib.ftn_selector_px_bound(length, 2, length, 1, C.byref(mg))
    assert pxb > 0 and mg.value >= 1
    return mg.value, pxb


def _ref(p):
    return None if p is None else C.byref(p)


def _call(env, ftn, entry, kw):
    """One call of ``entry`` whose arguments are those of a good call except for ``kw``; returns (rc, message)."""
    lib, plans, bad_xch = env
    a = dict(psum=FAKE, nparts=1, Btotal=None, med=FAKE, B=B, L=L, k=2, act=0, desc=FAKE, amps=FAKE, wts=FAKE, x=FAKE,
             y=FAKE, plan="ok", wblob=FAKE, mg=None, pxb=None, ws=FAKE, short=0, xch=None, flags=0, rows=None,
             gamma=FAKE, misalign=0, out=True)
    a.update(kw)
    plan = plans[a["plan"]]
    mg, pxb = _bounds(lib, max(2, a["L"]))
    mg = mg if a["mg"] is None else a["mg"]
    pxb = pxb if a["pxb"] is None else a["pxb"]
    btotal = a["B"] if a["Btotal"] is None else a["Btotal"]
    xch = C.byref(bad_xch) if a["xch"] else None
    n = a["B"] if not a["rows"] or a["rows"] < 0 else min(a["B"], a["rows"])             # rows of a pass
    need = lib.ftn_timesblock_workspace_bytes(_ref(plans["ok"]), max(1, min(n, 65535)), max(2, a["L"]), min(16, max(1, mg)), max(0, pxb))
    assert need > 0
    ws_bytes = need - a["short"]
    fin = (a["psum"], a["nparts"], btotal, a["med"], a["B"], a["L"], a["k"], a["L"], 1, a["act"], 0, 0.0, a["desc"],
           a["amps"], a["wts"])
    if entry == "finalize":
        rc = lib.ftn_period_finalize(*fin, None, xch)
    elif entry == "fused":
        rc = lib.ftn_period_finalize_stage_a(*fin, a["x"], _ref(plan), a["wblob"], mg, pxb, a["ws"], ws_bytes, None, None, xch)
    elif entry == "forms":
        rc = lib.ftn_timesblock_forms(_ref(plan), a["B"], a["L"], a["act"], a["misalign"],
                                      C.byref(ftn.lib.FtnForms()) if a["out"] else None)
    else:
        head = (a["x"], a["y"], a["B"], a["L"], _ref(plan), a["wblob"], a["desc"], a["wts"], mg, pxb)
        tail = (a["ws"], ws_bytes, None, None) + (() if a["rows"] is None else (a["rows"],))
        mid = (a["flags"], a["gamma"], FAKE, 1e-5) if "norm" in entry else (a["act"], a["flags"])
        rc = getattr(lib, "ftn_timesblock_" + entry)(*head, *mid, *tail)
    return rc, lib.ftn_last_error().decode()


FORWARDS = ("forward", "forward_norm", "forward_rows", "forward_norm_rows")

# (name, entry, what differs from a good call)
CASES = [
    ("fin-null-med", "finalize", dict(med=None)),
    ("fin-null-psum", "finalize", dict(psum=None)),
    ("fin-misaligned-amps", "finalize", dict(amps=FAKE + 4)),
    ("fin-shape", "finalize", dict(B=0)),
    ("fin-btotal", "finalize", dict(Btotal=1)),
    ("fin-k17", "finalize", dict(k=17)),
    ("fin-act3", "finalize", dict(act=3)),
    ("fin-xch", "finalize", dict(xch=True)),
    ("fin-long", "finalize", dict(L=LONG)),
    ("fin-null+xch", "finalize", dict(med=None, xch=True)),
    ("fin-xch+misaligned", "finalize", dict(xch=True, wts=FAKE + 8)),
    ("fin-misaligned+shape", "finalize", dict(amps=FAKE + 4, B=0)),
    ("fin-shape+k17", "finalize", dict(Btotal=1, k=17)),
    ("fin-k17+act3", "finalize", dict(k=17, act=3)),
    ("fin-act3+long", "finalize", dict(act=3, L=LONG)),
    ("fused-nothing", "fused", dict(psum=None, x=None)),
    ("fused-null-plan", "fused", dict(plan=None)),
    ("fused-null-ws", "fused", dict(ws=None)),
    ("fused-null-med", "fused", dict(med=None)),
    ("fused-misaligned-amps", "fused", dict(amps=FAKE + 4)),
    ("fused-btotal", "fused", dict(Btotal=1)),
    ("fused-shape", "fused", dict(B=0)),
    ("fused-rows-65536", "fused", dict(B=65536)),
    ("fused-k17", "fused", dict(k=17)),
    ("fused-act3", "fused", dict(act=3)),
    ("fused-single-conv", "fused", dict(plan="single")),
    ("fused-mp8", "fused", dict(plan="mp8")),
    ("fused-bounds", "fused", dict(mg=0)),
    ("fused-ws-short", "fused", dict(short=1)),
    ("fused-ws-misaligned", "fused", dict(ws=FAKE + 16)),
    ("fused-long", "fused", dict(L=LONG)),
    ("fused-xch", "fused", dict(psum=None, xch=True)),
    ("fused-xch+null-plan", "fused", dict(xch=True, plan=None)),
    ("fused-xch+null-med", "fused", dict(xch=True, med=None)),
    ("fused-nothing+null-plan", "fused", dict(psum=None, x=None, plan=None)),
    ("fused-null-med+misaligned", "fused", dict(med=None, amps=FAKE + 4)),
    ("fused-misaligned+shape", "fused", dict(wts=FAKE + 4, B=0)),
    ("fused-btotal+k17", "fused", dict(Btotal=1, k=17)),
    ("fused-k17+mp8", "fused", dict(k=17, plan="mp8")),
    ("fused-act3+ws-short", "fused", dict(act=3, short=1)),
    ("fused-mp8+bounds", "fused", dict(plan="mp8", mg=17)),
    ("fused-bounds+ws-short", "fused", dict(pxb=-1, short=1)),
    ("fused-ws-short+long", "fused", dict(short=1, L=LONG)),
    # stage A only (psum NULL, no exchange): the finalize operands are not looked at, the rest is
    ("fused-a-only-k17", "fused", dict(psum=None, med=None, amps=FAKE + 4, k=17)),
    ("fused-a-only-ws-short", "fused", dict(psum=None, med=None, desc=None, amps=FAKE + 4, short=1)),
    ("fused-a-only-long", "fused", dict(psum=None, L=LONG)),
    ("forms-null", "forms", dict(plan=None)),
    ("forms-null-out", "forms", dict(out=False)),
    ("forms-rows-65536", "forms", dict(B=65536)),
    ("forms-act3", "forms", dict(act=3)),
    ("forms-misalign", "forms", dict(misalign=16)),
    ("forms-nbr0", "forms", dict(plan="nbr0")),
    ("forms-mp8", "forms", dict(plan="mp8")),
    ("forms-shape+nbr0", "forms", dict(L=1, plan="nbr0")),
]
for _e in FORWARDS:
    _r = dict(rows=1) if "rows" in _e else {}
    CASES += [
        (f"{_e}-null-x", _e, dict(x=None, **_r)),
        (f"{_e}-shape", _e, dict(B=0, **_r)),
        (f"{_e}-groups", _e, dict(mg=0, **_r)),
        (f"{_e}-pad", _e, dict(plan="pad", **_r)),
        (f"{_e}-nbr0", _e, dict(plan="nbr0", **_r)),
        (f"{_e}-mp8", _e, dict(plan="mp8", **_r)),
        (f"{_e}-px-bound", _e, dict(pxb=-1, **_r)),
        (f"{_e}-flags", _e, dict(flags=2, **_r)),
        (f"{_e}-stage-a-done-single-conv", _e, dict(flags=1, plan="single", **_r)),
        (f"{_e}-ws-short", _e, dict(short=1, **_r)),
        (f"{_e}-ws-misaligned", _e, dict(ws=FAKE + 16, **_r)),
        (f"{_e}-shape+groups", _e, dict(L=1, mg=17, **_r)),
        (f"{_e}-groups+pad", _e, dict(mg=0, plan="pad", **_r)),
        (f"{_e}-pad+ws-short", _e, dict(plan="pad", short=1, **_r)),
        (f"{_e}-nbr0+ws-short", _e, dict(plan="nbr0", short=1, **_r)),
        (f"{_e}-flags+ws-short", _e, dict(flags=2, short=1, **_r)),
    ]
    if "norm" in _e:
        CASES += [(f"{_e}-null-gamma", _e, dict(gamma=None, **_r)), (f"{_e}-null-gamma+null-x", _e, dict(gamma=None, x=None, **_r))]
    else:
        CASES += [(f"{_e}-act3", _e, dict(act=3, **_r)), (f"{_e}-act3+ws-short", _e, dict(act=3, short=1, **_r))]
    if "rows" in _e:
        CASES += [
            (f"{_e}-rows0", _e, dict(rows=0)),
            (f"{_e}-rows65536", _e, dict(rows=65536)),
            (f"{_e}-rows-1", _e, dict(rows=-1)),
            (f"{_e}-stage-a-done-two-passes", _e, dict(B=100, rows=50, flags=1)),
            (f"{_e}-pass-ws-short", _e, dict(B=100, rows=40, short=1)),
            (f"{_e}-rows0+null-x", _e, dict(rows=0, x=None)),
            (f"{_e}-rows65536+shape", _e, dict(rows=65536, B=0)),
            (f"{_e}-two-passes+groups", _e, dict(B=100, rows=50, flags=1, mg=0)),
        ]
    else:
        CASES += [(f"{_e}-rows-65536", _e, dict(B=65536))]

EXPECT = {
    'fin-null-med': 'ftn_period_finalize: null pointer',
    'fin-null-psum': 'ftn_period_finalize: null pointer',
    'fin-misaligned-amps': 'ftn_period_finalize: amps / weights must be 16-byte aligned',
    'fin-shape': 'ftn_period_finalize: bad shape',
    'fin-btotal': 'ftn_period_finalize: bad shape',
    'fin-k17': 'ftn_period_finalize: k_periods=17 > FTN_KMAX=16',
    'fin-act3': 'ftn_period_finalize: act_dtype=3',
    'fin-xch': 'ftn_period_finalize: bad exchange (world / rank / seq / mode / F_cap)',
    'fin-long': 'ftn_period_finalize: L=8192 too long',
    'fin-null+xch': 'ftn_period_finalize: null pointer',
    'fin-xch+misaligned': 'ftn_period_finalize: bad exchange (world / rank / seq / mode / F_cap)',
    'fin-misaligned+shape': 'ftn_period_finalize: amps / weights must be 16-byte aligned',
    'fin-shape+k17': 'ftn_period_finalize: bad shape',
    'fin-k17+act3': 'ftn_period_finalize: k_periods=17 > FTN_KMAX=16',
    'fin-act3+long': 'ftn_period_finalize: act_dtype=3',
    'fused-nothing': 'ftn_period_finalize_stage_a: nothing to do (psum and x both null)',
    'fused-null-plan': 'ftn_period_finalize_stage_a: null pointer',
    'fused-null-ws': 'ftn_period_finalize_stage_a: null pointer',
    'fused-null-med': 'ftn_period_finalize_stage_a: null pointer',
    'fused-misaligned-amps': 'ftn_period_finalize_stage_a: amps / weights must be 16-byte aligned',
    'fused-btotal': 'ftn_period_finalize_stage_a: bad shape',
    'fused-shape': 'ftn_period_finalize_stage_a: bad shape',
    'fused-rows-65536': 'ftn_period_finalize_stage_a: bad shape',
    'fused-k17': 'ftn_period_finalize_stage_a: k=17 act_dtype=0',
    'fused-act3': 'ftn_period_finalize_stage_a: k=2 act_dtype=3',
    'fused-single-conv': 'ftn_period_finalize_stage_a: bottleneck blocks only',
    'fused-mp8': 'ftn_period_finalize_stage_a: bottleneck blocks only',
    'fused-bounds': 'ftn_period_finalize_stage_a: bounds',
    'fused-ws-short': 'ftn_period_finalize_stage_a: workspace 62719 < 62720 bytes or misaligned',
    'fused-ws-misaligned': 'ftn_period_finalize_stage_a: workspace 62720 < 62720 bytes or misaligned',
    'fused-long': 'ftn_period_finalize_stage_a: L=8192 too long',
    'fused-xch': 'ftn_period_finalize_stage_a: bad exchange (world / rank / seq / mode / F_cap)',
    'fused-xch+null-plan': 'ftn_period_finalize_stage_a: bad exchange (world / rank / seq / mode / F_cap)',
    'fused-xch+null-med': 'ftn_period_finalize_stage_a: bad exchange (world / rank / seq / mode / F_cap)',
    'fused-nothing+null-plan': 'ftn_period_finalize_stage_a: nothing to do (psum and x both null)',
    'fused-null-med+misaligned': 'ftn_period_finalize_stage_a: null pointer',
    'fused-misaligned+shape': 'ftn_period_finalize_stage_a: amps / weights must be 16-byte aligned',
    'fused-btotal+k17': 'ftn_period_finalize_stage_a: bad shape',
    'fused-k17+mp8': 'ftn_period_finalize_stage_a: k=17 act_dtype=0',
    'fused-act3+ws-short': 'ftn_period_finalize_stage_a: k=2 act_dtype=3',
    'fused-mp8+bounds': 'ftn_period_finalize_stage_a: bottleneck blocks only',
    'fused-bounds+ws-short': 'ftn_period_finalize_stage_a: bounds',
    'fused-ws-short+long': 'ftn_period_finalize_stage_a: workspace 10520831 < 10520832 bytes or misaligned',
    'fused-a-only-k17': 'ftn_period_finalize_stage_a: k=17 act_dtype=0',
    'fused-a-only-ws-short': 'ftn_period_finalize_stage_a: workspace 62719 < 62720 bytes or misaligned',
    'fused-a-only-long': 'ftn_period_finalize_stage_a: L=8192 too long',
    'forms-null': 'ftn_timesblock_forms: null pointer',
    'forms-null-out': 'ftn_timesblock_forms: null pointer',
    'forms-rows-65536': 'ftn_timesblock_forms: bad shape B=65536 L=48',
    'forms-act3': 'ftn_timesblock_forms: act_dtype=3 x_misalign=0',
    'forms-misalign': 'ftn_timesblock_forms: act_dtype=0 x_misalign=16',
    'forms-nbr0': 'ftn_timesblock_forms: bad plan',
    'forms-mp8': 'ftn_timesblock_forms: bad plan',
    'forms-shape+nbr0': 'ftn_timesblock_forms: bad shape B=2 L=1',
    'forward-null-x': 'ftn_timesblock_forward: null pointer',
    'forward-shape': 'ftn_timesblock_forward: bad shape B=0 L=48',
    'forward-groups': 'ftn_timesblock_forward: max_groups=0',
    'forward-pad': 'ftn_timesblock_forward: plan channel padding is inconsistent',
    'forward-nbr0': 'ftn_timesblock_forward: nbr=0',
    'forward-mp8': 'ftn_timesblock_forward: bad MP',
    'forward-px-bound': 'ftn_timesblock_forward: px_bound=-1',
    'forward-flags': 'ftn_timesblock_forward: flags=2',
    'forward-stage-a-done-single-conv': 'ftn_timesblock_forward: flags=1',
    'forward-ws-short': 'ftn_timesblock_forward: workspace 62719 < 62720 bytes',
    'forward-ws-misaligned': 'ftn_timesblock_forward: workspace/weights must be 256/16-byte aligned',
    'forward-shape+groups': 'ftn_timesblock_forward: bad shape B=2 L=1',
    'forward-groups+pad': 'ftn_timesblock_forward: max_groups=0',
    'forward-pad+ws-short': 'ftn_timesblock_forward: plan channel padding is inconsistent',
    'forward-nbr0+ws-short': 'ftn_timesblock_forward: nbr=0',
    'forward-flags+ws-short': 'ftn_timesblock_forward: flags=2',
    'forward-act3': 'ftn_timesblock_forward: act_dtype=3 (the fused LayerNorm epilogue is fp32 only)',
    'forward-act3+ws-short': 'ftn_timesblock_forward: act_dtype=3 (the fused LayerNorm epilogue is fp32 only)',
    'forward-rows-65536': 'ftn_timesblock_forward: bad shape B=65536 L=48',
    'forward_norm-null-x': 'ftn_timesblock_forward: null pointer',
    'forward_norm-shape': 'ftn_timesblock_forward: bad shape B=0 L=48',
    'forward_norm-groups': 'ftn_timesblock_forward: max_groups=0',
    'forward_norm-pad': 'ftn_timesblock_forward: plan channel padding is inconsistent',
    'forward_norm-nbr0': 'ftn_timesblock_forward: nbr=0',
    'forward_norm-mp8': 'ftn_timesblock_forward: bad MP',
    'forward_norm-px-bound': 'ftn_timesblock_forward: px_bound=-1',
    'forward_norm-flags': 'ftn_timesblock_forward: flags=2',
    'forward_norm-stage-a-done-single-conv': 'ftn_timesblock_forward: flags=1',
    'forward_norm-ws-short': 'ftn_timesblock_forward: workspace 62719 < 62720 bytes',
    'forward_norm-ws-misaligned': 'ftn_timesblock_forward: workspace/weights must be 256/16-byte aligned',
    'forward_norm-shape+groups': 'ftn_timesblock_forward: bad shape B=2 L=1',
    'forward_norm-groups+pad': 'ftn_timesblock_forward: max_groups=0',
    'forward_norm-pad+ws-short': 'ftn_timesblock_forward: plan channel padding is inconsistent',
    'forward_norm-nbr0+ws-short': 'ftn_timesblock_forward: nbr=0',
    'forward_norm-flags+ws-short': 'ftn_timesblock_forward: flags=2',
    'forward_norm-null-gamma': 'ftn_timesblock_forward_norm: LayerNorm parameters',
    'forward_norm-null-gamma+null-x': 'ftn_timesblock_forward_norm: LayerNorm parameters',
    'forward_norm-rows-65536': 'ftn_timesblock_forward: bad shape B=65536 L=48',
    'forward_rows-null-x': 'ftn_timesblock_forward: null pointer',
    'forward_rows-shape': 'ftn_timesblock_forward_rows: bad shape B=0 L=48',
    'forward_rows-groups': 'ftn_timesblock_forward: max_groups=0',
    'forward_rows-pad': 'ftn_timesblock_forward: plan channel padding is inconsistent',
    'forward_rows-nbr0': 'ftn_timesblock_forward: nbr=0',
    'forward_rows-mp8': 'ftn_timesblock_forward: bad MP',
    'forward_rows-px-bound': 'ftn_timesblock_forward: px_bound=-1',
    'forward_rows-flags': 'ftn_timesblock_forward: flags=2',
    'forward_rows-stage-a-done-single-conv': 'ftn_timesblock_forward_rows: FTN_FWD_STAGE_A_DONE needs a single pass (B=2 rows_per_pass=1)',
    'forward_rows-ws-short': 'ftn_timesblock_forward: workspace 31999 < 32000 bytes',
    'forward_rows-ws-misaligned': 'ftn_timesblock_forward: workspace/weights must be 256/16-byte aligned',
    'forward_rows-shape+groups': 'ftn_timesblock_forward_rows: bad shape B=2 L=1',
    'forward_rows-groups+pad': 'ftn_timesblock_forward: max_groups=0',
    'forward_rows-pad+ws-short': 'ftn_timesblock_forward: plan channel padding is inconsistent',
    'forward_rows-nbr0+ws-short': 'ftn_timesblock_forward: nbr=0',
    'forward_rows-flags+ws-short': 'ftn_timesblock_forward: flags=2',
    'forward_rows-act3': 'ftn_timesblock_forward: act_dtype=3 (the fused LayerNorm epilogue is fp32 only)',
    'forward_rows-act3+ws-short': 'ftn_timesblock_forward: act_dtype=3 (the fused LayerNorm epilogue is fp32 only)',
    'forward_rows-rows0': 'ftn_timesblock_forward_rows: rows_per_pass=0 outside [1, 65535]',
    'forward_rows-rows65536': 'ftn_timesblock_forward_rows: rows_per_pass=65536 outside [1, 65535]',
    'forward_rows-rows-1': 'ftn_timesblock_forward_rows: rows_per_pass=-1 outside [1, 65535]',
    'forward_rows-stage-a-done-two-passes': 'ftn_timesblock_forward_rows: FTN_FWD_STAGE_A_DONE needs a single pass (B=100 rows_per_pass=50)',
    'forward_rows-pass-ws-short': 'ftn_timesblock_forward: workspace 1230079 < 1230080 bytes',
    'forward_rows-rows0+null-x': 'ftn_timesblock_forward_rows: rows_per_pass=0 outside [1, 65535]',
    'forward_rows-rows65536+shape': 'ftn_timesblock_forward_rows: bad shape B=0 L=48',
    'forward_rows-two-passes+groups': 'ftn_timesblock_forward_rows: FTN_FWD_STAGE_A_DONE needs a single pass (B=100 rows_per_pass=50)',
    'forward_norm_rows-null-x': 'ftn_timesblock_forward: null pointer',
    'forward_norm_rows-shape': 'ftn_timesblock_forward_rows: bad shape B=0 L=48',
    'forward_norm_rows-groups': 'ftn_timesblock_forward: max_groups=0',
    'forward_norm_rows-pad': 'ftn_timesblock_forward: plan channel padding is inconsistent',
    'forward_norm_rows-nbr0': 'ftn_timesblock_forward: nbr=0',
    'forward_norm_rows-mp8': 'ftn_timesblock_forward: bad MP',
    'forward_norm_rows-px-bound': 'ftn_timesblock_forward: px_bound=-1',
    'forward_norm_rows-flags': 'ftn_timesblock_forward: flags=2',
    'forward_norm_rows-stage-a-done-single-conv': 'ftn_timesblock_forward_rows: FTN_FWD_STAGE_A_DONE needs a single pass (B=2 rows_per_pass=1)',
    'forward_norm_rows-ws-short': 'ftn_timesblock_forward: workspace 31999 < 32000 bytes',
    'forward_norm_rows-ws-misaligned': 'ftn_timesblock_forward: workspace/weights must be 256/16-byte aligned',
    'forward_norm_rows-shape+groups': 'ftn_timesblock_forward_rows: bad shape B=2 L=1',
    'forward_norm_rows-groups+pad': 'ftn_timesblock_forward: max_groups=0',
    'forward_norm_rows-pad+ws-short': 'ftn_timesblock_forward: plan channel padding is inconsistent',
    'forward_norm_rows-nbr0+ws-short': 'ftn_timesblock_forward: nbr=0',
    'forward_norm_rows-flags+ws-short': 'ftn_timesblock_forward: flags=2',
    'forward_norm_rows-null-gamma': 'ftn_timesblock_forward_norm_rows: LayerNorm parameters',
    'forward_norm_rows-null-gamma+null-x': 'ftn_timesblock_forward_norm_rows: LayerNorm parameters',
    'forward_norm_rows-rows0': 'ftn_timesblock_forward_norm_rows: rows_per_pass=0 outside [1, 65535]',
    'forward_norm_rows-rows65536': 'ftn_timesblock_forward_rows: rows_per_pass=65536 outside [1, 65535]',
    'forward_norm_rows-rows-1': 'ftn_timesblock_forward_rows: rows_per_pass=-1 outside [1, 65535]',
    'forward_norm_rows-stage-a-done-two-passes': 'ftn_timesblock_forward_rows: FTN_FWD_STAGE_A_DONE needs a single pass (B=100 rows_per_pass=50)',
    'forward_norm_rows-pass-ws-short': 'ftn_timesblock_forward: workspace 1230079 < 1230080 bytes',
    'forward_norm_rows-rows0+null-x': 'ftn_timesblock_forward_norm_rows: rows_per_pass=0 outside [1, 65535]',
    'forward_norm_rows-rows65536+shape': 'ftn_timesblock_forward_rows: bad shape B=0 L=48',
    'forward_norm_rows-two-passes+groups': 'ftn_timesblock_forward_rows: FTN_FWD_STAGE_A_DONE needs a single pass (B=100 rows_per_pass=50)',
}


@pytest.mark.parametrize("name,entry,kw", CASES, ids=[c[0] for c in CASES])
def test_first_error_is_the_parents(env, ftn, name, entry, kw):
    rc, msg = _call(env, ftn, entry, kw)
    assert rc == -1 and msg == EXPECT[name]


def test_table_covers_every_entry_and_fault():
    assert len({c[0] for c in CASES}) == len(CASES) == len(EXPECT)
    assert {c[1] for c in CASES} == {"finalize", "fused", "forms", *FORWARDS}
    text = "\n".join(EXPECT.values())
    for piece in ("null pointer", "16-byte aligned", "> FTN_KMAX=16", "act_dtype=3", "bad exchange", "too long", "nbr=0", "bad MP",
                  "channel padding is inconsistent", "rows_per_pass=0 outside", "rows_per_pass=65536 outside", "needs a single pass",
                  "workspace", "bottleneck blocks only", "bad plan", "nothing to do"):
        assert piece in text, piece


def test_plan_check_is_shared(env, ftn):
    """The forms query and the fused stage A make the forwards' plan check: a plan ``ftn_timesblock_forward`` refuses
    (inconsistent channel padding, no branches) is refused by them too, each in its own words."""
    assert _call(env, ftn, "forward", dict(plan="pad"))[1] == "ftn_timesblock_forward: plan channel padding is inconsistent"
    assert _call(env, ftn, "forms", dict(plan="pad")) == (-1, "ftn_timesblock_forms: bad plan")
    for plan in ("pad", "nbr0"):
        assert _call(env, ftn, "fused", dict(plan=plan)) == (-1, "ftn_period_finalize_stage_a: bottleneck blocks only")


# (L, k, pmax, min_thr) -> (max_groups, px_bound): the constructor clamps (k < 0 -> 0, pmax < 1 -> 1, the threshold into
# [1, pmax]) as the same commit applied them
PX_BOUND = {
    (48, -3, 48, 1): (1, 48),
    (48, 3, 0, 1): (1, 48),
    (48, 3, 12, 40): (1, 48),
    (48, 3, 12, 0): (3, 149),
    (48, 3, -5, -5): (1, 48),
    (48, 0, 48, 1): (1, 48),
    (48, 3, 48, 1): (3, 194),
    (48, 16, 48, 57): (1, 48),
    (97, -3, 97, 1): (1, 97),
    (97, 3, 0, 1): (1, 97),
    (97, 3, 12, 40): (1, 108),
    (97, 3, 12, 0): (3, 314),
    (97, 3, -5, -5): (1, 97),
    (97, 0, 97, 1): (1, 97),
    (97, 3, 97, 1): (3, 400),
    (97, 16, 97, 106): (1, 97),
}


@pytest.mark.parametrize("args", sorted(PX_BOUND), ids=str)
def test_selector_px_bound_under_the_clamps(ftn, args):
    lib = ftn.lib.load()
    mg = C.c_int(-1)
    pxb = lib.ftn_selector_px_bound(*args, C.byref(mg))
    assert (mg.value, pxb) == PX_BOUND[args]


def test_selector_px_bound_cases():
    got = set(PX_BOUND)
    for length in (48, 97):
        assert {(length, -3, length, 1), (length, 3, 0, 1), (length, 3, 12, 40), (length, 3, 12, 0)} <= got


# ---- the StageA record ------------------------------------------------------------------------------------------
def test_selection_declares_stage_a(ftn):
    rt = ftn.runtime
    z = torch.zeros(1)
    assert rt.Selection(z, z, z, 1).stage_a is None
    call = rt.StageA(z, "plan", "wblob")
    assert (call.x, call.plan, call.wblob, call.range_flag, call.ws) == (z, "plan", "wblob", None, None)


def test_tuples_are_refused(ftn):
    rt, T = ftn.runtime, ftn.models.timesnet
    x = torch.zeros(2, L, 4)
    med = torch.zeros(2, L // 2 + 1)
    with pytest.raises((TypeError, ValueError), match="StageA"):
        rt.finalize(med.double().sum(0), 2, med, L, 2, L, 1, stage_a=(x, None, None))
    with pytest.raises((TypeError, ValueError), match="StageA"):
        T.FFTPeriodSelector(2, L).select_device(x, stage_a=(None, None))


def test_select_device_refuses_a_record_of_another_tensor(ftn):
    rt, T = ftn.runtime, ftn.models.timesnet
    x = torch.randn(2, L, 4)
    sm = T.FFTPeriodSelector(2, L)
    for other in (x.clone(), x[:1], x.double()):
        with pytest.raises(ValueError, match="StageA"):
            sm.select_device(x, stage_a=rt.StageA(other, None, None))
