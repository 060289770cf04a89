"""One TimesBlock call from the selector's finalize to stages A-F, over every route the host path offers: the fused
finalize + stage A, ``stage_a_only`` then ``finalize``, the unfused finalize, and the unfused finalize in row passes,
each with and without the LayerNorm epilogue.  The routes launch the same kernels on the same operands, so descriptor,
amplitudes, weights and y are equal bit for bit.

The two blocks are the smallest that reach both stage-A epilogues (fp32 and f16x2 pieces), at the shapes of
``test_gpu_workspace_hygiene.test_selection_buffers_ignore_their_old_content``."""
import pytest
import torch

from test_gpu_forms_small import _block
from ws_poison import check_guards, poisoned_workspace

pytestmark = pytest.mark.gpu

BLOCKS = [(5, 97, 24, 3, 96, "f32"), (3, 96, 64, 5, 256, "f16x2")]          # B, L, C, K, d_ff, engine
ROUTES = ("fused", "apart", "unfused", "unfused-rows")
ROWS = 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


class _Call:
    """One block, its input, and a selection + forward by any route."""

    def __init__(self, ftn, dev, B, L, C, K, d_ff, engine):
        self.rt, self.engine, self.B, self.L = ftn.runtime, engine, B, L
        blk = _block(ftn, C, d_ff, 4.0, "k357", engine, "gelu", dev)
        self.wblob, self.plan = blk._packed(dev)
        assert self.rt.fuse_stage_a(self.plan)
        sm = ftn.models.timesnet.FFTPeriodSelector(K, L)
        self.ctor = (int(sm.k), int(sm.pmax), int(sm.min_period_threshold))
        self.x = torch.from_numpy(ftn.synth.make_input(B, L, C, seed=57)).to(dev)
        self.norm = (torch.linspace(0.5, 1.5, C, device=dev), torch.linspace(-0.2, 0.2, C, device=dev), 1e-5)
        self.flags = []

    def flag(self):
        """A fresh range word for the f16x2 block (every one of them must stay 0), None for the fp32 block."""
        if self.engine != "f16x2":
            return None
        self.flags.append(torch.zeros(1, dtype=torch.int32, device=self.x.device))
        return self.flags[-1]

    def select(self, route, monkeypatch):
        rt = self.rt
        med, psum = rt.spectrum(self.x)
        call = rt.StageA(self.x, self.plan, self.wblob, self.flag())
        with monkeypatch.context() as m:
            m.setenv("FTN_FUSE_STAGE_A", "0" if route.startswith("unfused") else "1")
            if route == "apart":
                rt.stage_a_only(call, *self.ctor)
                assert call.ws is not None
            sel = rt.finalize(psum, self.B, med, self.L, *self.ctor, stage_a=call)
        assert (sel.stage_a is call) if not route.startswith("unfused") else (sel.stage_a is None and call.ws is None)
        return sel

    def forward(self, sel, norm, rows=None):
        y = self.rt.timesblock_forward(self.x, self.plan, self.wblob, sel, norm=self.norm if norm else None,
                                       range_flag=self.flag(), rows_per_pass=rows)
        assert sel.stage_a is None
        return y

    def run(self, route, norm, monkeypatch):
        sel = self.select(route, monkeypatch)
        y = self.forward(sel, norm, ROWS if route.endswith("rows") else None)
        return sel, y

    def range_words_clear(self):
        torch.cuda.synchronize()
        return all(int(f.item()) == 0 for f in self.flags)


@pytest.mark.parametrize("B,L,C,K,d_ff,engine", BLOCKS)
def test_every_route_gives_the_same_bits(B, L, C, K, d_ff, engine, ftn, dev, monkeypatch):
    c = _Call(ftn, dev, B, L, C, K, d_ff, engine)
    got = {(route, norm): c.run(route, norm, monkeypatch) for route in ROUTES for norm in (False, True)}
    sel0, _ = got[("fused", False)]
    for (route, norm), (sel, y) in got.items():
        for name in ("desc", "amps", "weights"):
            assert torch.equal(getattr(sel, name), getattr(sel0, name)), (route, norm, name)
        assert torch.equal(y, got[("fused", norm)][1]), (route, norm)
        assert bool(torch.isfinite(y).all()) and not torch.equal(y, c.x)
    assert not torch.equal(got[("fused", False)][1], got[("fused", True)][1])
    d = sel0.host()
    assert 1 <= d.n_groups <= d.n_sel == K
    assert c.range_words_clear()


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("B,L,C,K,d_ff,engine", BLOCKS)
def test_a_consumed_selection_serves_a_second_forward(B, L, C, K, d_ff, engine, norm, ftn, dev, monkeypatch):
    """The fused stage A serves one forward; the next one on the same selection finds no record, allocates its own
    workspace (exactly one, here full of NaN bytes between guards) and runs stage A itself: the same bits."""
    c = _Call(ftn, dev, B, L, C, K, d_ff, engine)
    sel, y = c.run("fused", norm, monkeypatch)
    assert sel.stage_a is None
    log = []
    with monkeypatch.context() as m:
        m.setattr(c.rt, "_workspace", poisoned_workspace(0xFF, log))
        y2 = c.forward(sel, norm)
    assert check_guards(log) == 1
    assert torch.equal(y2, y)
    assert c.range_words_clear()


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("B,L,C,K,d_ff,engine", BLOCKS)
def test_a_fused_selection_refuses_row_passes(B, L, C, K, d_ff, engine, norm, ftn, dev, monkeypatch):
    """Stage A of a fused selection fills a workspace of all B rows: more than one pass over it is refused on the host,
    before a workspace is allocated or an entry point is called."""
    c = _Call(ftn, dev, B, L, C, K, d_ff, engine)
    sel = c.select("fused", monkeypatch)
    lib, log, calls = ftn.lib.load(), [], []
    for entry in ("ftn_timesblock_forward", "ftn_timesblock_forward_norm", "ftn_timesblock_forward_rows",
                  "ftn_timesblock_forward_norm_rows"):
        monkeypatch.setattr(lib, entry, lambda *a, _e=entry: calls.append(_e) or 0)
    monkeypatch.setattr(c.rt, "_workspace", poisoned_workspace(0xFF, log))
    with pytest.raises(RuntimeError, match="single pass only"):
        c.forward(sel, norm, ROWS)
    assert not log and not calls
