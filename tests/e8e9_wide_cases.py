"""TEST INFRASTRUCTURE shared by the tests of the device's decoder for long LZ77 streams with the inverse E8E9 filter behind it
(test_emu_e8e9_decode_wide.py, test_gpu_e8e9_decode_wide.py): the methods, and one ragged batch of blocks in a fixed order.
Nothing of the machine is read.  What a stream must decode to is always what the host makes of it (zpq_postprocess_block, the
method's own PCOMP program)."""
from __future__ import annotations

import functools

import e8e9_cases as ec

# level 1, level 2, and level 1 with rb = 1 at 2^25 bytes of M: each behind E8E9
METHODS = ("x0,5,6,0,3,20", "x0,6,4,0,3,20", "x5,5,4,0,3,24")


def e8_of(xm: str) -> str:
    """The E8E9 form of a plain LZ77 method (args[1] 1 / 2 -> 5 / 6): the stream's format is the same."""
    a = xm[1:].split(",")
    assert a[1] in ("1", "2"), xm
    a[1] = str(int(a[1]) + 4)
    return "x" + ",".join(a)


def _framed(n: int) -> bytes:
    """n bytes that begin with a hit at 0 and end with an e9 whose address bytes never arrive."""
    head, tail = bytes([0xe8, 0x10, 0x20, 0x30, 0x00]), bytes([0xe9, 0xff, 0xff, 0xff, 0xff])
    return head + bytes((37 * k + 11) & 255 for k in range(n - 10)) + tail


@functools.lru_cache(maxsize=None)
def blocks():
    """e8e9_cases.blocks() in its order -- the first twenty have 0 .. 9 bytes and an e8 / e9 at byte 0, and the lengths around 4 096
    and 8 192 are no multiples of 16, so packed and aligned offsets differ from the second block on and a misplaced byte lands on
    an opcode --, then three consecutive blocks of 17, 31 and 33 bytes, x86_like(70001, 7) twice in a row, and 300 000 bytes of
    x86_like, whose stream spans many pieces of 4 096 bytes."""
    out = list(ec.blocks())
    out += [_framed(17), _framed(31), _framed(33)]
    out += [ec.x86_like(70001, 7), ec.x86_like(70001, 7)]
    out.append(ec.x86_like(300000, 19))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def streams(xm: str):
    """The stream of every block under method xm (zpq_preprocess_block), once."""
    return tuple(ec.stream_of(xm, b) for b in blocks())


@functools.lru_cache(maxsize=None)
def expected(xm: str):
    """zpq_postprocess_block over every stream of streams(xm): what the device must deliver."""
    import zpaq_amd as z
    out = []
    for s in streams(xm):
        rc, data, _ = z.postprocess_block(xm, s)
        assert rc == 0, (xm, len(s), rc)
        out.append(data)
    return tuple(out)
