"""TEST INFRASTRUCTURE shared by the tests of the device's forward E8E9 filter (test_emu_e8e9_forward.py,
test_gpu_e8e9_forward.py): the sequential scan in Python, the decomposition of device/e8e9_forward_kernel.h written out, and the
blocks around every edge of that kernel.  Nothing of the machine is read.  What a block must be filtered to is always what the
host makes of it (zpq_e8e9); model() is its readable copy."""
from __future__ import annotations

import bisect
import functools

from e8e9_cases import ALPHABETS, TILE, _over, x86_like

__all__ = ["ALPHABETS", "TILE", "x86_like", "model", "chains_model", "blocks", "WORST", "MANY_CHAINS", "SKIPPING", "skipping_block"]


def model(block: bytes) -> bytes:
    """The forward filter as the sequential scan (host/preproc.cpp e8e9_forward, libzpaq.cpp:6450-6459): from the end down."""
    b = bytearray(block)
    n = len(b)
    for i in range(n - 5, -1, -1):
        if (b[i] & 254) == 0xe8 and ((b[i + 4] + 1) & 254) == 0:
            a = ((b[i + 1] | b[i + 2] << 8 | b[i + 3] << 16) + i) & 0xffffff
            b[i + 1], b[i + 2], b[i + 3] = a & 255, (a >> 8) & 255, a >> 16
    return bytes(b)


def chains_model(o: bytes):
    """What device/e8e9_forward_kernel.h does, written out: candidates, seeds and breaks from the original bytes, then one walk
    downward per head.  Returns (the filtered block, the longest walk in steps)."""
    n = len(o)
    b = bytearray(o)
    cand = [i + 4 < n and (o[i] & 254) == 0xe8 for i in range(n)]
    seeds = [i for i in range(n) if cand[i] and ((o[i + 4] + 1) & 254) == 0]
    breaks = [i for i in range(n) if cand[i] and not any(cand[j] for j in range(i + 1, min(n, i + 4)))]
    longest = 0
    for k, s in enumerate(seeds):
        j = bisect.bisect_left(breaks, s)                         # the chain's break: the first at or above s (there is one)
        if k + 1 < len(seeds) and seeds[k + 1] <= breaks[j]:
            continue                                              # the seed above belongs to the same chain: not a head
        floor = breaks[j - 1] + 4 if j else 0                     # the three positions above the lower chain's break are its own
        i, lasthit, steps = s, None, 0
        while True:
            steps += 1
            if cand[i] and ((b[i + 4] + 1) & 254) == 0:
                a = ((b[i + 1] | b[i + 2] << 8 | b[i + 3] << 16) + i) & 0xffffff
                b[i + 1], b[i + 2], b[i + 3] = a & 255, (a >> 8) & 255, a >> 16
                lasthit = i
            if i <= floor:
                break
            i -= 1
            if lasthit is None or lasthit - i > 3:
                lasthit = None
                kk = bisect.bisect_right(seeds, i) - 1
                if kk < 0 or seeds[kk] < floor:
                    break
                i = seeds[kk]
        longest = max(longest, steps)
    return bytes(b), longest


def _with(b: bytes, at, value: int) -> bytes:
    b = bytearray(b)
    for a in at:
        b[a] = value
    return bytes(b)


WORST = b"\xe8\xff\xff" * 3000                                      # one chain of 9 000 bytes, walked by one head
MANY_CHAINS = b"\xe8\xff\xff\xff\xff" * 2000                        # 2 000 chains of 2 steps each (the inverse's worst case)
SKIPPING = _with(b"\xe8\x11\x11" * 4000, (6004, 11999), 0xff)       # one chain of 4 000 candidates, the seeds far apart


def skipping_block() -> bytes:
    """1 MiB that is one chain of candidates with ff in two tails: a walk over every candidate would take 350 000 steps."""
    n = (1 << 20) // 3
    return _with(b"\xe8\x11\x11" * n + b"\x11", (3 * (n // 2) + 4, 3 * (n - 2) + 4), 0xff)


def _straddle(length: int, edge: int, seed: int, head_above: bool = False) -> bytes:
    """`length` bytes over the second alphabet with a hit laid across `edge`: the opcode up to 4 positions below it.  head_above:
    a second hit three positions above the edge, whose walk comes down across it."""
    b = bytearray(_over(ALPHABETS[1], length, seed))
    at = edge - 1 - length % 5
    if at + 4 < length:
        b[at] = 0xe8 + length % 2
        b[at + 1:at + 4] = bytes([0x12, 0x34, 0x56])
        b[at + 4] = 0xff if length % 3 else 0x00
    if head_above and edge + 8 < length:
        b[edge - 1:edge + 8] = bytes([0xe8, 0xff, 0xff, 0xe8, 0xff, 0xff, 0xe9, 0xff, 0x00])
    return bytes(b)


@functools.lru_cache(maxsize=None)
def blocks():
    """The blocks, in one fixed order."""
    out = []
    # around i + 4 < n: a block of 5 bytes visits i = 0 only
    for n in range(10):
        out.append(bytes([0xe8, 0x10, 0x20, 0x30, 0x00, 0xe9, 0xff, 0xff, 0xff][:n]))
        out.append(bytes([0xe9] + [0xff] * 8)[:n])
        out.append(bytes([0x11] * 4 + [0xe8, 0x01, 0x02, 0x03, 0xff])[:n])
    # around the tile's edge, with a hit across it
    for n in list(range(TILE - 5, TILE + 6)) + list(range(2 * TILE - 3, 2 * TILE + 4)):
        out.append(_straddle(n, TILE if n < 2 * TILE - 3 else 2 * TILE, 100 + n))
    out.append(_straddle(TILE + 700, TILE, 99, head_above=True))     # the head lies in the upper tile and walks into the lower
    # random bytes over each alphabet
    for k, alphabet in enumerate(ALPHABETS):
        for j, n in enumerate((64, 65, 255, 333, 700)):
            out.append(_over(alphabet, n, 1000 + 10 * k + j))
    out.append(WORST)
    out.append(MANY_CHAINS)
    out.append(SKIPPING)
    out.append(x86_like(70001, 7))                                 # positions above 2^16: the carry reaches the third address byte
    out.append(skipping_block())
    return tuple(out)
