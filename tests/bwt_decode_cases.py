"""TEST INFRASTRUCTURE shared by the tests of the device's BWT decoder (test_emu_bwt_decode.py, test_gpu_bwt_decode.py): the
methods, the valid inputs, streams that obey the rule 1 <= idx <= n, S[idx] == 255 without being a BWT, and streams outside it.
What a stream must decode to is always what the host makes of it: zpq_postprocess_block, the method's own PCOMP program;
model() is that program written out, for the streams under the rule."""
from __future__ import annotations

import functools
import random

import lz77_hash_cases as hc

METHOD, BIG_METHOD, HUGE_METHOD = "x0,3", "x1,3", "x2,3"      # x1,3 for blocks above 2^20 - 257, x2,3 above 2^21 - 257
TILE, CHUNK, STRIDE = 4096, 64, 256          # device/layout.h kBwtTile, kBwtChunk, kBwtStride
EMPTY = b"\xff\x00\x00\x00\x00"              # what the pre-processor writes for an empty block; it decodes to nothing


def mbits_of(xm: str) -> int:
    return int(xm[1:].split(",")[0]) + 20


def model(s):                       # None: outside the rule
    n = len(s) - 5
    if n < 1:
        return None
    idx = int.from_bytes(s[n + 1:], "little")
    if not (1 <= idx <= n) or s[idx] != 255:
        return None
    order = sorted((b for b in range(n + 1) if b != idx), key=lambda b: s[b])   # stable
    nxt = [0] * (n + 1)
    for r, b in enumerate(order):
        nxt[r + 1] = b
    out, d = bytearray(), idx
    while d != 0:
        d = nxt[d]
        out.append(s[d])
    return bytes(out)


@functools.lru_cache(maxsize=None)
def valid_inputs():
    """Blocks the library's BWT is given: every kind at every length of the LZ77 tests (the empty ones among them), real 255s
    beside the marker, every byte value, two symbols, lengths around the tile, the chunk and the splitter stride, several tiles,
    and text long enough for links beyond 16 bits."""
    from zpaq_amd import corpus
    blocks = list(hc.inputs())
    blocks.append(b"\xff" * 300)
    blocks.append(bytes(range(255, -1, -1)) * 2)
    blocks.append(b"ab" * 333)
    for i, size in enumerate((TILE, CHUNK, STRIDE)):
        for d in (-1, 0, 1):
            # the stream holds n + 1 positions: both n and n + 1 pass each boundary
            blocks.append(corpus.block(("text", "records", "lcg")[i], size + d, 5100 + 3 * i + d).tobytes())
            blocks.append(corpus.block(("text", "records", "lcg")[i], size + d - 1, 5200 + 3 * i + d).tobytes())
    blocks.append(corpus.block("records", 3 * TILE + 1, 5300).tobytes())
    blocks.append(corpus.block("text", 70000, 5301).tobytes())
    return tuple(blocks)


@functools.lru_cache(maxsize=None)
def valid_streams():
    """(stream, block) of every valid input, through the host's pre-processor."""
    out = []
    for d in valid_inputs():
        s, seen = hc.preprocess(METHOD, d)
        assert seen == d
        out.append((s, d))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rule_streams():
    """400 seeded streams that obey the rule: (stream, model's output).  Most are no BWT of anything: cycles beside the path."""
    rng = random.Random(7)
    out = []
    for _ in range(400):
        n = rng.choice([1, 2, 3, 5, 17, 64, 65, 255, 256, 257, 1000])
        alphabet = [rng.randrange(256) for _ in range(rng.choice([1, 2, 4, 256]))]
        body = bytearray(rng.choice(alphabet) for _ in range(n + 1))
        idx = rng.randrange(1, n + 1)
        body[idx] = 255
        stream = bytes(body) + idx.to_bytes(4, "little")
        out.append((stream, model(stream)))
    full = sum(1 for s, m in out if len(m) == len(s) - 5)
    assert full >= 20 and len(out) - full >= 20, (full, len(out))
    return tuple(out)


def _with_idx(stream: bytes, idx: int) -> bytes:
    return stream[:-4] + idx.to_bytes(4, "little")


@functools.lru_cache(maxsize=None)
def outside_batch():
    """Streams outside the rule between two valid ones: idx 0, n + 1 and 0x7fffffff, S[idx] changed to 7, streams of 0 to 4
    bytes, and every cut of the valid streams of 5 kinds x 5 small lengths (a cut may happen to obey the rule)."""
    from zpaq_amd import corpus
    small = [hc.preprocess(METHOD, corpus.block(k, n, 700 + i).tobytes())[0]
             for i, (k, n) in enumerate((k, n) for n in (9, 12, 255, 256, 257) for k in hc.KINDS)]
    bad = []
    for s in small[:5] + small[10:15]:
        n = len(s) - 5
        idx = int.from_bytes(s[n + 1:], "little")
        bad += [_with_idx(s, 0), _with_idx(s, n + 1), _with_idx(s, 0x7FFFFFFF)]
        hit = bytearray(s)
        hit[idx] = 7
        bad.append(bytes(hit))
    bad += [small[0][:k] for k in range(5)]
    for s in small:
        bad += [s[:k] for k in range(len(s))]
    return tuple([small[0]] + bad + [small[-1]])
