"""TEST INFRASTRUCTURE shared by the tests of the device's LZ77 decoder (test_emu_lz77_decode.py, test_gpu_lz77_decode.py):
the methods, hand-made streams -- written here code by code, in the formats of DESIGN 4.5.2 -- and damaged ones.  What a stream
must decode to is always what the host makes of it: zpq_postprocess_block, the method's own PCOMP program."""
from __future__ import annotations

import functools

import lz77_codes_cases as cc
import lz77_hash_cases as hc

E8E9 = "x0,5,6,0,3,20"
METHODS = tuple(m for m in hc.METHODS if m != E8E9) + ("x6,1,4,0,3,24",)          # the last one: rb = 2
L1, L2, RB = cc.METHODS                                                          # level 1, level 2, level 1 with rb = 2 (min_match 4)


def args_of(xm: str):
    a = [int(x) for x in xm[1:].split(",")]
    return a + [0] * (9 - len(a))


class _Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value: int, nbits: int):
        self.v |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits

    def bytes(self) -> bytes:
        return self.v.to_bytes((self.n + 7) // 8, "little")


def encode(xm: str, codes) -> bytes:
    """codes: ("lit", bytes) or ("match", len, off), written one code each -- no splitting, no merging, no checks."""
    a = args_of(xm)
    level, rb, mm = a[1] & 3, max(a[0] - 4, 0), a[2]
    if level == 2:
        out = bytearray()
        for c in codes:
            if c[0] == "lit":
                assert 1 <= len(c[1]) <= 64
                out.append(len(c[1]) - 1)
                out += c[1]
            else:
                _, length, off = c
                assert 0 <= length - mm < 64 and off >= 1
                nb = 2 if off - 1 < 1 << 16 else (3 if off - 1 < 1 << 24 else 4)
                out.append(64 * (nb - 1) + length - mm)
                out += (off - 1).to_bytes(nb, "big")
        return bytes(out)
    w = _Bits()
    for c in codes:
        if c[0] == "lit":
            n = len(c[1])
            w.put(0, 2)
            for ll in range(n.bit_length() - 2, -1, -1):
                w.put(1, 1)
                w.put(n >> ll, 1)
            w.put(0, 1)
            for byte in c[1]:
                w.put(byte, 8)
        else:
            _, length, off = c
            assert length >= 4 and off >= 1
            offp = off + (1 << rb) - 1
            lo = offp.bit_length() - 1 - rb
            w.put((lo + 8) >> 3, 2)
            w.put(lo & 7, 3)
            for ll in range(length.bit_length() - 2, 1, -1):
                w.put(1, 1)
                w.put(length >> ll, 1)
            w.put(0, 1)
            w.put(length & 3, 2)
            w.put(offp, rb + lo)
    return w.bytes()


def _lit(n: int, seed: int):
    return ("lit", cc._bytes(n, seed))


@functools.lru_cache(maxsize=None)
def handmade():
    """(name, method, stream, must be declined) around the copy kernel's group rule and its windows of 64 tokens."""
    cases = []
    for xm in (L1, L2, RB):
        # literals and matches in turn (nothing merges): 63, 64 and 65 codes, then enough for three windows
        for ncodes in (63, 64, 65, 150):
            codes = [_lit(5, 300)]
            for k in range(1, ncodes):
                codes.append(_lit(1 + k % 3, 300 + k) if k % 2 == 0 else ("match", 4 + k % 5, 1 + k % 4))
            cases.append((f"{ncodes} codes", xm, encode(xm, codes), False))
        # T0 literals [0, 8); T1 a match from [0, 4): starts a group at 8; T2 literals [12, 16); T3 a match at 16 whose source
        # ends exactly at 8 (off 12: it stays in the group) or one byte past it (off 11: it starts the next)
        for off in (12, 11):
            codes = [_lit(8, 310), ("match", 4, 8), _lit(4, 311), ("match", 4, off), _lit(3, 312)]
            cases.append((f"source ends at the group's start + {12 - off}", xm, encode(xm, codes), False))
        # each match needs the token right before it; runs (off < len) among them, one over a match that is itself a run
        codes = [_lit(4, 320), ("match", 4, 4), ("match", 6, 2), ("match", 9, 1), ("match", 7, 3), _lit(2, 321), ("match", 5, 2), ("match", 40, 7)]
        cases.append(("each match needs the one before", xm, encode(xm, codes), False))
        # the same offset twice in a row: one copy
        cases.append(("pieces at one offset", xm, encode(xm, [_lit(3, 330), ("match", 5, 3), ("match", 7, 3), ("match", 4, 2), _lit(1, 331)]), False))
        # a match at position 0 of a non-empty output reads in front of the start
        cases.append(("a first code that is a match", xm, encode(xm, [("match", 5, 1), _lit(3, 340)]), True))
        cases.append(("a match one byte too far back", xm, encode(xm, [_lit(3, 341), ("match", 5, 4)]), True))
    return tuple(cases)


def cuts(stream: bytes):
    """The stream cut at every length from 0 to its size."""
    return [stream[:k] for k in range(len(stream) + 1)]


def pad_variants(stream: bytes):
    """A level-1 stream with bits of its last byte set from the top: non-zero pad bits first, then damage to the last code."""
    if not stream:
        return []
    return [stream[:-1] + bytes([stream[-1] | m]) for m in (0x80, 0xC0, 0xE0, 0xF0, 0xF8, 0xFC, 0xFE, 0xFF)]


def damaged_batch(xm: str):
    """(streams, number of cuts): a valid stream, then each stream of a small valid batch cut at every length, with non-zero pad
    bits (level 1), the hand-made streams that must be declined, and a valid stream again."""
    from zpaq_amd import corpus
    small = [(k, n) for n in (257, 256, 255, 12, 9) for k in hc.KINDS]
    if xm == RB:
        small = [("zeros", 255), ("text", 12), ("pattern", 9)]     # (its program's M is 64 MiB on the host, per call)
    valid = [hc.preprocess(xm, corpus.block(k, n, 700 + i).tobytes())[0] for i, (k, n) in enumerate(small)]
    bad = []
    for s in valid:
        bad += cuts(s)
        if args_of(xm)[1] == 1:
            bad += pad_variants(s)
    bad += [c[2] for c in handmade() if c[1] == xm and c[3]]
    return [valid[0]] + bad + [valid[-1]], sum(len(s) + 1 for s in valid)
