"""TEST INFRASTRUCTURE shared by the tests of the device's LZ77 coder (test_emu_lz77_codes.py, test_gpu_lz77_codes.py): hand-made
and random token lists.  The coder never looks at whether a match matches, so lists no parse makes at small sizes reach every
branch of it; what the stream must be is always what the host's coder (zpq_lz77_serialize) writes for the same list."""
from __future__ import annotations

import functools
import struct

import numpy as np

# level 1, level 2, and level 1 with rb = 2 (the offset split); min_match 4 everywhere
METHODS = ("x0,1,4,0,3,20", "x0,2,4,0,3,20", "x6,1,4,0,3,24")
MM = 4
GAPS = (0, 1, 4095, 4096, 4097, 8192, 8193)
LENS = (MM, MM + 63, MM + 64, 2 * MM + 63, 2 * MM + 64, 49152)


def tok(i, off, length, blit=0) -> bytes:
    return struct.pack("<4I", i, off, length, blit)


def _bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _list(steps, tail: int, seed: int):
    """steps = (gap in front, blit, len, off or None for off = i) per token, then `tail` literals: (block, token list)."""
    pos, toks = 0, b""
    for gap, blit, length, off in steps:
        i = pos + gap
        toks += tok(i, i if off is None else off, length, blit)
        pos = i + blit + length
    return _bytes(pos + tail, seed), toks


@functools.lru_cache(maxsize=None)
def synthetic():
    """(name, block, token list) of every hand-made case; valid for each of METHODS."""
    cases = []
    # every gap in front of a token (the first token cannot stand at 0: its offset would be 0) and behind the last one
    for k, tail in enumerate(GAPS):
        steps = [(1, 0, 5, 1)] + [(g, 0, 4 + j, 1 + j) for j, g in enumerate(GAPS)]
        cases.append((f"gaps, tail {tail}",) + _list(steps, tail, 100 + k))
    # literals that belong to the match on top of a remainder of 4095: one run of 4095 / 4350, behind none or one flush
    for k, (gap, blit) in enumerate([(4095, 0), (4095, 255), (4096 + 4095, 0), (4096 + 4095, 255), (1, 255), (4096, 255)]):
        cases.append((f"gap {gap} blit {blit}",) + _list([(gap, blit, 9, 1), (0, blit, 4, 3)], 2, 120 + k))
    # lengths around the places where level 2 splits a match
    for k, length in enumerate(LENS):
        cases.append((f"len {length}",) + _list([(3, 0, length, 2), (2, 1, length, 1)], 1, 140 + k))
    # offsets around the place where level 2 widens them; off = i
    far = [(65540, 0, 7, 1), (5, 0, 6, 65536), (0, 2, 8, 65537), (7, 0, 5, None), (0, 0, 4, 65535)]
    cases.append(("offsets",) + _list(far, 3, 160))
    # level 1: literal(1) match(4, 1) literal(2) is 11 + 8 + 21 = 40 bits, a whole number of bytes; one literal is 11 bits
    cases.append(("ends on a byte",) + _list([(1, 0, 4, 1)], 2, 170))
    cases.append(("ends inside a byte", _bytes(1, 171), b""))
    cases.append(("9000 literals", _bytes(9000, 172), b""))
    cases.append(("empty", b"", b""))
    return tuple(cases)


def refusals():
    """(name, block, token list): one per check of the host's coder."""
    data = _bytes(300, 180)
    return (
        ("out of order", data, tok(50, 1, 10) + tok(55, 1, 4)),
        ("offset 0", data, tok(50, 0, 10)),
        ("offset beyond the position", data, tok(50, 51, 10)),
        ("length 0", data, tok(50, 1, 0)),
        ("span past the end", data, tok(50, 1, 4) + tok(290, 1, 8, 3)),
        ("position past the end", data, tok(301, 1, 1)),
        ("span that wraps 32 bits", data, tok(50, 1, 0xFFFFFFF0, 0x20)),
        ("a list over an empty block", b"", tok(0, 1, 1)),
    )


def random_list(rng, n: int):
    """A random valid list over n bytes: gaps of every class, literals in front, lengths and offsets of every width."""
    pos, toks = 0, b""
    while True:
        gap = rng.choice([0, 0, 1, 2, 7, 63, 64, 65, 300, 4095, 4096, 4097, rng.randrange(0, 9000)])
        blit = rng.choice([0, 0, 0, 1, 3, 255, rng.randrange(0, 256)])
        length = rng.choice([1, 3, 4, 5, 67, 68, 71, 72, 200, rng.randrange(1, 3000)])
        i = max(pos + gap, 1)                         # (a match at 0 would need offset 0)
        if i + blit + length > n:
            break
        off = rng.choice([1, i, rng.randrange(1, i + 1), min(i, 65536), min(i, 65537)])
        toks += tok(i, off, length, blit)
        pos = i + blit + length
    return toks


def random_batch(rng):
    ns = [rng.choice([0, 1, 2, 5, 64, 65, 300, 4096, 4097, 9000, 20000]) for _ in range(6)]
    if rng.random() < 0.3:
        ns.append(rng.randrange(66000, 90000))
    return [(_bytes(n, rng.randrange(1 << 30)), random_list(rng, n)) for n in ns]
