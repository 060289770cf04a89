"""The f16x2 range guard (DESIGN §4 "Range", ``include/flowtimes.h`` ABI 9): engine f16x2 stores 1 to a caller-owned
int32 word when a value does not fit its fp16 pieces, and the call must be repeated on bf16x3.  A bare ``TimesBlock``
repairs its own eager calls (``check_range``).  A composite forward has already fed a block's output onwards, so it runs
again with every block on bf16x3 (``repeat_on_trip``; ``device_flags``, ``tripped`` and ``fall_back`` are its pieces).
"""
from __future__ import annotations

import contextlib
import warnings
from typing import Callable, Sequence

import torch

MESSAGE = ("a value left the fp16 range of engine f16x2 (|v| >= 65504 or not finite); the forward was repeated with "
           "every block on engine bf16x3")


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def arm(block, device: torch.device):
    """``(word, event)`` for one f16x2 call of ``block``.  An eager call gets a word from the block's pool and an event
    to record behind it: the block reads the word itself.  In a capture or in device-flag mode the block's calls store
    into one word until it is taken away (``device_flags``), and the event is None.  Made in a capture, that word is in
    device memory and the captured fill zeroes it at every replay; outside one, it is the block's own and is reused.
    Eager words are pinned host memory that the device writes directly (``runtime.new_range_flag``)."""
    from . import runtime

    capturing = _capturing()
    if not (capturing or block.range_flag_on_device):
        block._range_dev_flag = None
        return block._range_slots.pop() if block._range_slots else (runtime.new_range_flag(device), torch.cuda.Event())
    if block._range_dev_flag is None:
        if capturing:
            block._range_dev_flag = torch.zeros(1, dtype=torch.int32, device=device)
        else:
            word = block._range_word
            if word is None or (word.is_cuda and word.device != device):
                block._range_word = runtime.new_range_flag(device)
            block._range_dev_flag = block._range_word
    return block._range_dev_flag, None


@contextlib.contextmanager
def device_flags(blocks: Sequence):
    """Device-flag mode for ``blocks`` over one composite forward; restores the previous mode on exit.  Yields a list
    that holds the words the blocks stored into once the context has ended.  Outside a capture they then leave the
    blocks; a captured forward leaves them there, for ``check_range()`` to read after a replay."""
    blocks = list(blocks)
    saved = [b.range_flag_on_device for b in blocks]
    words = []
    for b in blocks:
        b.range_flag_on_device, b._range_dev_flag = True, None
    finished = False
    try:
        yield words
        finished = True
    finally:
        keep = _capturing()
        for b, on in zip(blocks, saved):
            b.range_flag_on_device = on
            if b._range_dev_flag is not None:
                words.append(b._range_dev_flag)
                if not keep:
                    b._range_dev_flag = None
        if not (finished or keep):
            for w in words:                     # reused words: a forward that did not finish must not trip the next
                w.zero_()


def tripped(flags: Sequence[torch.Tensor], group=None) -> bool:
    """Whether any of ``flags`` is set, read at one synchronisation of the current stream (pinned host words need no
    copy), and all-reduced (MAX) over ``group`` when one is given so that every rank gets the same answer (gloo:
    through the host).  Clears what it read."""
    flags = list(flags)
    if any(not f.is_cuda for f in flags):
        torch.cuda.current_stream().synchronize()
    hit = any(int(f.item()) != 0 for f in flags)
    if group is not None:
        import torch.distributed as dist

        v = torch.tensor([int(hit)], dtype=torch.int32)
        v = v if dist.get_backend(group) == "gloo" else v.cuda()
        dist.all_reduce(v, op=dist.ReduceOp.MAX, group=group)
        hit = int(v.item()) != 0
    for f in flags if hit else ():
        f.zero_()
    return hit


def fall_back(blocks: Sequence, message: str = MESSAGE) -> None:
    """One ``RuntimeWarning``, every block on bf16x3 from now on, one ``_range_fallbacks`` count per block on f16x2."""
    warnings.warn(message, RuntimeWarning, stacklevel=3)
    for b in blocks:
        b._range_fallbacks += int(b._engine_name() == "f16x2")
        b.engine = "bf16x3"


def repeat_on_trip(blocks: Sequence, run: Callable, group=None, message: str = MESSAGE):
    """``run()`` in device-flag mode; if a word tripped (on any rank of ``group``), ``fall_back`` and ``run()`` again.
    In a capture nothing is read: a replay that trips raises ``FloatingPointError`` from ``check_range()``."""
    blocks = list(blocks)
    with device_flags(blocks) as flags:
        out = run()
    if _capturing() or not tripped(flags, group):
        return out
    fall_back(blocks, message)
    return run()
