"""TEST INFRASTRUCTURE shared by the tests of the device's LZ77 decoder for streams parsed in pieces
(test_emu_lz77_decode_wide.py, test_gpu_lz77_decode_wide.py): hand-made streams, written code by code with
lz77_decode_cases.encode, around what is new in that decoder -- the seams between pieces, the stitch, the jump rounds.  What a
stream must decode to is always what the host makes of it (zpq_postprocess_block)."""
from __future__ import annotations

import functools

import lz77_codes_cases as cc
import lz77_decode_cases as dc

L1, L2, RB = dc.L1, dc.L2, dc.RB
METHODS = (L1, L2, RB)
SEAM_PIECES = (64, 256)


def level_of(xm: str) -> int:
    return dc.args_of(xm)[1] & 3


def units(xm: str) -> int:
    """Positions per stream byte: a level-1 stream is addressed in bits, a level-2 stream in bytes."""
    return 8 if level_of(xm) == 1 else 1


def _lit(n: int, seed: int):
    return ("lit", cc._bytes(n, seed))


def size_of(xm: str, c) -> int:
    """Positions one code takes as lz77_decode_cases.encode writes it."""
    if level_of(xm) == 2:
        return len(dc.encode(xm, [c]))
    rb = max(dc.args_of(xm)[0] - 4, 0)
    if c[0] == "lit":
        n = len(c[1])
        return 2 + 2 * (n.bit_length() - 1) + 1 + 8 * n
    _, length, off = c
    offp = off + (1 << rb) - 1
    return 2 + 3 + 2 * (length.bit_length() - 3) + 1 + 2 + offp.bit_length() - 1


def literals_up_to(xm: str, target: int, seed: int):
    """Runs of 1 .. 8 literals whose codes end exactly at position `target` (every target from 200 on can be reached)."""
    sizes = {n: size_of(xm, _lit(n, 0)) for n in range(1, 9)}
    how = {0: None}
    for at in range(1, target + 1):
        for n, s in sizes.items():
            if at - s in how:
                how[at] = n
                break
    assert target in how, (xm, target)
    runs = []
    while target:
        runs.append(how[target])
        target -= sizes[how[target]]
    return [_lit(n, seed + i) for i, n in enumerate(runs)]


def _filler(xm: str, nbytes: int, seed: int):
    """Runs of literals whose stream is at least nbytes long."""
    codes = []
    while len(dc.encode(xm, codes)) < nbytes:
        codes.append(_lit(7 + (seed + len(codes)) % 9, seed + len(codes)))
    return codes


@functools.lru_cache(maxsize=None)
def seams():
    """(name, method, piece, stream): a match and a run of literals that start 0 .. 23 bits (level 1) or 0 .. 3 bytes (level 2) in
    front of the seam behind the second piece -- the seam at every bit of the code's header -- for pieces of 64 and 256 bytes."""
    cases = []
    for xm in METHODS:
        for piece in SEAM_PIECES:
            seam = 2 * piece * units(xm)
            for code in (("match", 9, 5), _lit(6, 77)):
                for back in range(24 if level_of(xm) == 1 else 4):
                    codes = literals_up_to(xm, seam - back, 500) + [code, _lit(5, 78), ("match", 6, 3)] + _filler(xm, piece, 600)
                    cases.append((f"{code[0]} {back} in front of the seam at {seam}", xm, piece, dc.encode(xm, codes)))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def long_literals():
    """(name, method, stream): a level-1 run of 4 096 literals in one code between short codes -- with pieces of 256 bytes the code
    leaps over whole pieces."""
    return tuple(("4096 literals in one code", xm, dc.encode(xm, [_lit(3, 90), _lit(4096, 91), ("match", 8, 2), _lit(4, 92)])) for xm in (L1, RB))


def parse_from(xm: str, stream: bytes, pos: int, stop: int):
    """The states (pos, t) of the code starts of a parse of `stream` begun at pos as if a code began there, up to the first start
    at or behind stop -- the parser of DESIGN 4.5.3 in plain Python, without its verdicts: where the stream ends or the parser
    refuses a field the list just stops."""
    a = dc.args_of(xm)
    rb, n = max(a[0] - 4, 0), len(stream)
    states = []
    if level_of(xm) == 2:
        while pos < stop and pos < n:
            states.append((pos, 0))
            c = stream[pos]
            pos += 2 + c if c < 64 else 2 + (c >> 6)
        return states + [(pos, 0)]
    v = int.from_bytes(stream, "little")
    t = (pos + 7) // 8
    while pos < stop:
        states.append((pos, t))
        if t >= n or 8 * t - pos > 24:
            return states
        t += 1
        mm = (v >> pos) & 3
        pos += 2
        length = 1
        if mm:
            r3 = (mm - 1) * 8 + ((v >> pos) & 7)
            pos += 3
            while True:
                t = max(t, (pos + 10) >> 3)
                if t > n or length >= 1 << 28:
                    return states
                if (v >> pos) & 1:
                    length = length * 2 + ((v >> (pos + 1)) & 1)
                    pos += 2
                else:
                    pos += 3
                    break
            if rb:
                t = max(t, (pos + rb + 7) >> 3)
                pos += rb
            t = max(t, (pos + r3 + 7) >> 3)
            if r3 > 24 or t > n:
                return states
            pos += r3
        else:
            while True:
                t = max(t, (pos + 9) >> 3)
                if t > n or length >= 1 << 28:
                    return states
                pos += 1
                if not (v >> (pos - 1)) & 1:
                    break
                length = length * 2 + ((v >> pos) & 1)
                pos += 1
            t = max(t, (pos + 15) >> 3)
            if t > n or length > n - t + 1:
                return states
            t += length - 1
            pos += 8 * length
    return states + [(pos, t)]


LATE_PIECE, LATE_K = 64, 2


@functools.lru_cache(maxsize=None)
def late_meet():
    """(method, stream): a level-1 stream whose piece LATE_K (pieces of LATE_PIECE bytes) never meets the true parse inside the
    piece.  The seam lies in a run of 8 literals whose bits, read from the seam on as a code, are a run of 128 literals: the
    provisional parse leaves the piece with its first code, while the true parse has several code starts in it.  Asserted here."""
    xm = L1
    seam = LATE_K * LATE_PIECE * 8
    as_code = 0
    for i in range(7):                                   # 00, then seven steps (1, 0) of the length, then 0: a run of 128
        as_code |= 1 << (2 + 2 * i)
    data = (cc._bytes(1, 70)[0] | as_code << 8 | 0x5A << 32 | int.from_bytes(cc._bytes(3, 71), "little") << 40).to_bytes(8, "little")
    head = size_of(xm, ("lit", data)) - 64
    codes = literals_up_to(xm, seam - head - 8, 700) + [("lit", data)]
    codes += [_lit(2, 72), ("match", 5, 3), _lit(3, 73), ("match", 4, 9), _lit(1, 74)] + _filler(xm, 5 * LATE_PIECE, 710)
    stream = dc.encode(xm, codes)
    true = parse_from(xm, stream, 0, 8 * len(stream))
    prov = parse_from(xm, stream, seam, seam + 8 * LATE_PIECE)
    inside = [s for s in true if seam <= s[0] < seam + 8 * LATE_PIECE]
    assert len(inside) >= 4 and prov[0] == (seam, seam // 8) and prov[0] not in true, (inside, prov)
    assert len(prov) == 2 and prov[1][0] >= seam + 8 * LATE_PIECE, prov       # one code, and it ends behind the piece
    return xm, stream


@functools.lru_cache(maxsize=None)
def chain(xm: str, depth: int = 1000):
    """8 literals, then `depth` matches of 8 at offset 8: every match reads exactly what the one before it wrote."""
    return dc.encode(xm, [_lit(8, 95)] + [("match", 8, 8)] * depth + [_lit(2, 96)])


@functools.lru_cache(maxsize=None)
def runs(xm: str):
    """Runs (off < len) at offsets 1, 2, 3 and 7 over a source that is itself a run."""
    codes = [_lit(7, 97), ("match", 40, 7)]
    for off in (1, 2, 3, 7):
        codes += [("match", 30 + off, off), _lit(1 + off % 3, 98 + off)]
    return dc.encode(xm, codes + [("match", 50, 3), ("match", 60, 1), ("match", 45, 2), ("match", 33, 7)])


@functools.lru_cache(maxsize=None)
def deferred(piece: int = 64):
    """(name, method, stream, must be declined): the two must-decline cases of lz77_decode_cases.handmade() -- a match that reaches
    one byte in front of the output's start, as a code of its own and behind three literals -- behind more than two pieces of
    literals, so that only the check against the absolute position can see them; and the same match one byte shorter, which is
    valid: the bound is exact."""
    cases = []
    for xm in METHODS:
        fill = _filler(xm, 2 * piece + 8, 5000)
        emitted = sum(len(c[1]) for c in fill)
        cases.append(("a match one byte too far back", xm, dc.encode(xm, fill + [("match", 5, emitted + 1), _lit(3, 341)]), True))
        cases.append(("a match one byte too far back behind literals", xm, dc.encode(xm, fill + [_lit(3, 342), ("match", 5, emitted + 4)]), True))
        cases.append(("a match that reaches the first byte", xm, dc.encode(xm, fill + [("match", 5, emitted), _lit(3, 343)]), False))
    return tuple(cases)
