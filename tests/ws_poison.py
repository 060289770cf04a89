"""A TimesBlock workspace whose old content is known to be hostile, between two guards (``include/flowtimes.h`` at
``ftn_timesblock_workspace_bytes``, DESIGN section 1 "Workspaces"): the result of a block call does not depend on the
bytes the workspace held before it, and the call writes nothing outside it.

``poisoned_workspace(pattern, log)`` replaces ``runtime._workspace(device, need)``, the single allocation point of
``runtime.timesblock_forward``, ``runtime.finalize`` (the fused stage A) and ``runtime.stage_a_only``; tests install it
with ``monkeypatch.setattr(ftn.runtime, "_workspace", ...)``.  The fills are ordinary torch ops on the current stream,
so they are ordered before the kernels.  Works on CPU tensors too (``test_ws_poison_host.py``).

Patterns, as repeated bytes:
  0x00  zeros
  0xFF  NaN as fp32, as bf16 and as fp16 (so in both halves of the P3 / H2 piece layouts), -1 as an int32 of the
        descriptor head
  0x7B  about 1.3e36 as fp32 and as bf16; 61280 as fp16: finite and inside the fp16 range, so by itself it must not
        trip the f16x2 range guard
"""
import torch

GUARD = 4096              # bytes on either side: a multiple of the 256-byte alignment the block's entry points demand
ALIGN = 256
SENTINEL = 0xA5           # guard byte: none of the patterns
PATTERNS = (0x00, 0xFF, 0x7B)


def poisoned_workspace(pattern, log):
    """A replacement for ``runtime._workspace``: ``need`` bytes of ``pattern`` between two guards of ``SENTINEL``.
    Appends ``(outer, need)`` to ``log`` (``outer``: front guard, interior, back guard) and returns the interior,
    ``numel() == need`` exactly and 256-byte aligned.  The allocation carries up to 255 bytes of slack in front of
    ``outer``, because host memory from ``torch.empty`` is only 64-byte aligned."""
    assert 0 <= int(pattern) <= 255 and int(pattern) != SENTINEL

    def _workspace(device, need):
        need = int(need)
        span = need + 2 * GUARD
        raw = torch.empty(span + ALIGN, dtype=torch.uint8, device=device)
        off = (-raw.data_ptr()) % ALIGN
        outer = raw[off:off + span]
        outer[:GUARD].fill_(SENTINEL)
        outer[GUARD + need:].fill_(SENTINEL)
        inner = outer[GUARD:GUARD + need]
        inner.fill_(int(pattern))
        assert inner.numel() == need and inner.data_ptr() % ALIGN == 0 and inner.is_contiguous()
        log.append((outer, need))
        return inner

    return _workspace


def pattern_tensor(pattern, shape, dtype, device):
    """A tensor of ``shape`` / ``dtype`` whose every byte is ``pattern`` (the selection buffers of the finalize tests)."""
    n = 1
    for s in shape:
        n *= int(s)
    raw = torch.full((n * torch.empty(0, dtype=dtype).element_size(),), int(pattern), dtype=torch.uint8, device=device)
    return raw.view(dtype).view(*shape)


def _first_bad(guard):
    bad = (guard != SENTINEL).nonzero()
    return None if bad.numel() == 0 else int(bad[0])


def check_guards(log):
    """Synchronise, then assert that both guards of every logged workspace are untouched."""
    if any(outer.is_cuda for outer, _ in log):
        torch.cuda.synchronize()
    for i, (outer, need) in enumerate(log):
        assert outer.numel() == need + 2 * GUARD
        front = _first_bad(outer[:GUARD])
        assert front is None, f"workspace {i} ({need} bytes): byte {front - GUARD} in front of the workspace was written"
        back = _first_bad(outer[GUARD + need:])
        assert back is None, f"workspace {i} ({need} bytes): byte {need + (back or 0)} past the workspace's start was written"
    return len(log)
