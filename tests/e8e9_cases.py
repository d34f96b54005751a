"""TEST INFRASTRUCTURE shared by the tests of the device's inverse E8E9 filter (test_emu_e8e9.py, test_gpu_e8e9_decode.py): the
methods, a seeded generator of x86-like bytes, the blocks around every edge of device/e8e9_kernel.h, and the sequential scan in
Python.  Nothing of the machine is read.  What a stream must decode to is always what the host makes of it
(zpq_postprocess_block, the method's own PCOMP program); model() is its readable copy for the filter alone."""
from __future__ import annotations

import bisect
import functools
import random

import numpy as np

import lz77_hash_cases as hc

TILE = 4096                                  # kE8Tile: bytes per workgroup of the mark pass (16 per lane)
# E8E9 alone, in front of LZ77 level 1 and level 2, in front of the BWT (without and with a model behind it)
METHODS = ("x0,4", "x0,5,6,0,3,20", "x0,6,4,0,3,20", "x0,7", "x0,7ci1")
OTHER_METHODS = ("x0,1,4,0,3,20", "x0,3", "x5,7", "x0,0")
ALPHABETS = (
    (0x00, 0xff, 0xe8, 0xe9),
    (0x00, 0xff, 0xe8, 0xe9, 0x01, 0x17, 0xe7, 0xea),
    (0x00,) * 12 + (0xff, 0xe8, 0xe9, 0x05),
    tuple(range(256)),
)


def model(block: bytes) -> bytes:
    """The inverse filter as the sequential scan (host/preproc.cpp e8e9_inverse, kE8Loop of host/method.cpp)."""
    b = bytearray(block)
    n = len(b)
    for i in range(0, n - 4):
        if (b[i] & 254) == 0xe8 and ((b[i + 4] + 1) & 254) == 0:
            a = ((b[i + 1] | b[i + 2] << 8 | b[i + 3] << 16) - i) & 0xffffff
            b[i + 1], b[i + 2], b[i + 3] = a & 255, (a >> 8) & 255, a >> 16
    return bytes(b)


def chains_model(o: bytes):
    """What device/e8e9_kernel.h does, written out: candidates, seeds and breaks from the original bytes, then one walk per head.
    Returns (the filtered block, the longest walk in steps)."""
    n = len(o)
    b = bytearray(o)
    cand = [i + 4 < n and ((o[i + 4] + 1) & 254) == 0 for i in range(n)]
    seeds = [i for i in range(n) if cand[i] and (o[i] & 254) == 0xe8]
    breaks = [i for i in range(n) if cand[i] and not any(cand[j] for j in range(max(0, i - 3), i))]
    longest = 0
    for k, s in enumerate(seeds):
        p = seeds[k - 1] if k else -1
        j = bisect.bisect_right(breaks, s) - 1
        if not (j >= 0 and breaks[j] > p):
            continue                                              # not a head
        j = bisect.bisect_right(breaks, s)
        end = breaks[j] if j < len(breaks) else n
        i, lasthit, steps = s, None, 0
        while True:
            steps += 1
            if cand[i] and (b[i] & 254) == 0xe8:
                a = ((b[i + 1] | b[i + 2] << 8 | b[i + 3] << 16) - i) & 0xffffff
                b[i + 1], b[i + 2], b[i + 3] = a & 255, (a >> 8) & 255, a >> 16
                lasthit = i
            i += 1
            if lasthit is None or i - lasthit > 3:
                lasthit = None
                kk = bisect.bisect_left(seeds, i)
                if kk == len(seeds) or seeds[kk] >= end:
                    break
                i = seeds[kk]
            if i + 4 >= n or i + 3 >= end:
                break
        longest = max(longest, steps)
    return bytes(b), longest


def x86_like(n: int, seed: int) -> bytes:
    """About 2 % e8 / e9 opcodes, each followed by a little-endian displacement whose top byte is 00 or ff, between other bytes
    and padding runs of 00, cc and ff."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < n:
        r = int(rng.integers(0, 100))
        if r < 10:
            out.append(0xe8 + int(rng.integers(0, 2)))
            d = int(rng.integers(-(1 << 20), 1 << 20))
            out += (d & 0xffffffff).to_bytes(4, "little")
        elif r < 13:
            out += bytes([(0x00, 0xcc, 0xff)[int(rng.integers(0, 3))]]) * int(rng.integers(1, 40))
        else:
            out += rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
    return bytes(out[:n])


def _over(alphabet, n: int, seed: int) -> bytes:
    rng = random.Random(seed)
    return bytes(rng.choice(alphabet) for _ in range(n))


def _straddle(length: int, edge: int, seed: int) -> bytes:
    """`length` bytes over the second alphabet with a hit laid across `edge`: the opcode up to 4 positions in front of it."""
    b = bytearray(_over(ALPHABETS[1], length, seed))
    at = edge - 1 - length % 5
    if at + 4 < length:
        b[at] = 0xe8 + length % 2
        b[at + 1:at + 4] = bytes([0x12, 0x34, 0x56])
        b[at + 4] = 0xff if length % 3 else 0x00
    return bytes(b)


@functools.lru_cache(maxsize=None)
def blocks():
    """The blocks, in one fixed order (the inputs of the filter in the emulator, the blocks to compress on the GPU)."""
    out = []
    # around i + 4 < n: a block of 5 bytes visits i = 0 only
    for n in range(10):
        out.append(bytes([0xe8, 0x10, 0x20, 0x30, 0x00, 0xe9, 0xff, 0xff, 0xff][:n]))
        out.append(bytes([0xe9] + [0xff] * 8)[:n])
    # around the tile's edge, with a hit across it
    for n in list(range(TILE - 5, TILE + 6)) + list(range(2 * TILE - 3, 2 * TILE + 4)):
        out.append(_straddle(n, TILE if n < 2 * TILE - 3 else 2 * TILE, 100 + n))
    # random bytes over each alphabet
    for k, alphabet in enumerate(ALPHABETS):
        for j, n in enumerate((64, 65, 255, 333, 700)):
            out.append(_over(alphabet, n, 1000 + 10 * k + j))
    out.append(b"\xe8" + bytes(5000) + b"\xe9" + bytes(300))       # one chain of 5 302 candidates, two seeds: the walk skips
    out.append(ADVERSARIAL)                                        # one chain of 2 000 seeds, every position walked
    out.append(x86_like(70001, 7))                                 # positions above 2^16: the borrow reaches the third address byte
    return tuple(out)


ADVERSARIAL = b"\xe8\xff\xff\xff\xff" * 2000


def skipping_block() -> bytes:
    """1 MiB that is one chain: e8, zeros, one e9 in the middle."""
    b = bytearray(1 << 20)
    b[0] = 0xe8
    b[1 << 19] = 0xe9
    return bytes(b)


def stream_of(xm: str, block: bytes) -> bytes:
    """The stream the method's coder sees for a block (zpq_preprocess_block)."""
    return hc.preprocess(xm, block)[0]
