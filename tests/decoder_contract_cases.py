"""Damaged and capped streams for every device decoder of a modelled block, for tests/test_emu_decoder_contract.py (the
emulator) and tests/test_gpu_decoder_contract.py (MI355X).  zpq_decode_batch documents a status for every stream: 0 at the end
of the stream or at the capacity, 2 where the coder's value leaves its range, 6 where the input ends, 5 where HCOMP stops with
an error -- and the bytes decoded before it.  A damaged stream decodes garbage until one of these happens: contexts, hash rows
and MATCH pointers that no encoder produces.  The yardstick is Oracle.decode_limited (oracle/zpaq_oracle.c zo_decode_limit).

Per chain one deterministic catalogue of (name, stream, max_out, valid, source): two valid inputs of at most 1.5 KiB with the
post-processing byte 0 in front, coded by the oracle (never by the code under test); bit flips at full and at low capacity,
truncations, an extension, whole-stream garbage, capacities around the block's length.  The CPU test holds the catalogue to the
conditions it needs to mean anything (every status present, at least 8 garbage decodes stopped by a capacity) and the generator
to the record of which decoder takes which chain."""
from collections import namedtuple

import numpy as np

import model_edge_cases as mec
from zpaq_amd import corpus

ERROR_BYTE = 255

# HCOMP stops with an error when the byte is 255; otherwise three ordinary contexts
VM_ERROR_CFG = """
comp 2 0 0 0 3
  0 cm 9 255
  1 icm 6
  2 mix2 8 0 1 24 255
hcomp
  a== 255 if error endif
  d= 0 *d=a d++ hash *d=a d++ a=*d a<<= 3 *d=a halt
end
"""
# ... and the same program without the stop: H is the same up to the first 255, so the oracle codes with this header the
# streams that the chain above decodes up to that byte (its own coder refuses an input with the byte)
VM_TWIN_CFG = VM_ERROR_CFG.replace("if error endif", "")

CHAINS = ("m5_text", "m5_records", "deep_isse", "pipe_stress", "one_word", "vm_error")

# What the generator says about each chain: the dual decoder's verdict, the lockstep decoder's threads per workgroup
TAKES = {
    "m5_text": {"dual": True, "team": 384},
    "m5_records": {"dual": True, "team": 512},
    "deep_isse": {"dual": True, "team": 512},
    "pipe_stress": {"dual": True, "team": 384},
    "one_word": {"dual": True, "team": 384},
    "vm_error": {"dual": True, "team": 384},
}
DUAL_DECLINES = tuple(n for n in CHAINS if TAKES[n]["dual"] is not True)
TEAM_DECLINES = tuple(n for n in CHAINS if not isinstance(TAKES[n]["team"], int))

# chain -> (seed, coded bytes written through the shift): a 48-byte input (low_zero_input) on which a shift of the coder takes
# `low` to 0 -- its low 24 bits were zero -- so that `low += (low == 0)` (libzpaq.cpp:2118) makes it 1, with no further shift
# behind it.  The oracle's stream up to that byte followed by zeros is the number `low` itself: it decodes the same bits up
# to there, then `curr` is 0 below `low` = 1 and the next bit is status 2.  A decoder that leaves the increment out goes on
# decoding.  Found by a search over seeds with the oracle's coder; the CPU test holds the oracle to the verdict.
LOW_ZERO = {"deep_isse": (33310, 13), "one_word": (34833, 14), "pipe_stress": (5618, 22), "vm_error": (47571, 8)}


def low_zero_input(seed, n=48):
    x, out = (seed * 2654435761 + 12345) & 0xFFFFFFFF, bytearray()
    for k in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out.append(x >> 24 if k else 0)
    return bytes(out)


Case = namedtuple("Case", "name stream max_out valid src")      # valid: decodes exactly; src: index of the input it came from, or None


def header(z, name, twin=False):
    if name == "m5_text":
        return z.method_to_header(z.expand_method("5", corpus.block("text", 1 << 20, corpus.BASE_SEED)))[0]
    if name == "m5_records":
        return z.method_to_header(z.expand_method("5", corpus.block("records", 1 << 20, corpus.BASE_SEED)))[0]
    if name == "deep_isse":
        return z.method_to_header(mec.DEEP_ISSE)[0]
    if name == "vm_error":
        return z.assemble(VM_TWIN_CFG if twin else VM_ERROR_CFG)[0]
    return z.assemble({"pipe_stress": mec.PIPE_STRESS_CFG, "one_word": mec.ONE_WORD_CFG}[name])[0]


def _no_error_byte(d):
    return bytes(b if b != ERROR_BYTE else 254 for b in d)


def valid_inputs(name):
    """The two inputs whose streams are damaged: text-like of about 1.2 KiB, records of about 700 bytes."""
    ins = [b"\0" + corpus.block("text", 1200, 41).tobytes(), b"\0" + corpus.block("records", 700, 42).tobytes()]
    return [_no_error_byte(d) for d in ins] if name == "vm_error" else ins


def vm_error_inputs():
    """(input, index of the first ERROR_BYTE or None): none, at byte 0, 1, the last byte, 64 and 65 (around the encoder's
    chunk boundary), twice, and an empty block."""
    base = _no_error_byte(b"\0" + corpus.block("text", 299, 43).tobytes())

    def at(*pos):
        d = bytearray(base)
        for p in pos:
            d[p] = ERROR_BYTE
        return bytes(d), min(pos)

    return [(base, None), at(0), at(1), at(len(base) - 1), at(64), at(65), (b"", None), at(130, 131),
            (_no_error_byte(b"\0" + corpus.block("lcg", 150, 44).tobytes()), None)]


def _flip(good, pos, bit):
    b = bytearray(good)
    b[pos] ^= 1 << bit
    return bytes(b)


def catalogue(name, hdr, encode):
    """The cases of one chain.  encode(data) -> the oracle's coded stream for this chain (for vm_error: with the twin header)."""
    ins = valid_inputs(name)
    coded = [encode(d) for d in ins]
    cases = []
    for s, (d, c) in enumerate(zip(ins, coded)):
        good = c + b"\0\0\0\0"
        n, full = len(c), len(d) + 64
        assert n > 40
        mids = (n // 4, n // 2 + 1, (3 * n) // 4 + 2)
        early = [(0, 7), (3, 0), (4, 5 - s)]
        late = [(mids[0], 1), (mids[1], 6), (mids[2], 3), (n - 5, 2)] + [(n - 4 + k, (3 * k + s) & 7) for k in range(4)]
        marker = [(n + k, (5 * k + 1) & 7) for k in range(4)]
        for pos, bit in early + late + marker:
            cases.append(Case(f"in{s}.flip{pos}.{bit}", _flip(good, pos, bit), full, False, s))
        # the same flips at a low capacity: garbage decoded to the capacity.  Behind a flip near the stream's start everything
        # is garbage, so the capacity is small; behind one further on it lies 20 to 100 bytes behind the place in the block that
        # the flipped byte codes, taken as proportional (a flip of a marker byte is never reached at a capacity below the
        # block's length: left out)
        for k, (pos, bit) in enumerate(early):
            cases.append(Case(f"in{s}.flip{pos}.{bit}.cap", _flip(good, pos, bit), (1, 37, 100)[(k + s) % 3], False, s))
        for k, (pos, bit) in enumerate(late):
            cap = min(pos * len(d) // n + (20, 37, 100)[(k + s) % 3], len(d) - 1)
            cases.append(Case(f"in{s}.flip{pos}.{bit}.cap", _flip(good, pos, bit), cap, False, s))
        for ln in (0, 1, 2, 3, 4, 5, n // 2, n - 1, n, n + 1, n + 2, n + 3):
            cases.append(Case(f"in{s}.cut{ln}", good[:ln], full, False, s))
        tail = bytes(np.random.default_rng(50 + s).integers(1, 256, 50, dtype=np.uint8))
        cases.append(Case(f"in{s}.extended", good + tail, full, True, s))
        for cap in (0, 1, len(d) - 1, len(d), len(d) + 1):
            cases.append(Case(f"in{s}.cap{cap}", good, cap, True, s))
    g0, g1 = coded[0] + b"\0\0\0\0", coded[1] + b"\0\0\0\0"
    cases += [
        Case("random400", bytes(np.random.default_rng(5).integers(0, 256, 400, dtype=np.uint8)), 1564, False, None),
        Case("zeros600", bytes(600), 1564, False, None),
        # ff: every bit 0, and a model that has learnt it spends next to nothing per bit -- 600 bytes of ff yield more than
        # 2^24 zero bytes on every chain here (9 004 460 on deep_isse), 8 bytes already more than 2^16 on most.  So no capacity
        # a test can afford lies above what they yield: 600 bytes at two capacities below it, and 5 bytes, which run out of
        # input after 4 to 8 bytes of output on four chains and still reach the capacity on pipe_stress and one_word, and 4
        # bytes, which run out of input on every chain: after one byte of output, on one_word after 24 949
        Case("ff600.below", b"\xff" * 600, 20, False, None),
        Case("ff600.cap1500", b"\xff" * 600, 1500, False, None),
        Case("ff5", b"\xff" * 5, 1564, False, None),
        Case("ff4", b"\xff" * 4, 1 << 15, False, None),
        Case("empty_block", bytes([0, 0, 0, 1, 0, 0, 0, 0]), 64, True, None),
        Case("spliced", g0[:len(g0) // 2] + g1[len(g1) // 2:], 1564, False, None),
    ]
    if name in LOW_ZERO:
        seed, emitted = LOW_ZERO[name]
        d = low_zero_input(seed)
        cases.append(Case("low_zero", encode(d)[:emitted] + bytes(8), len(d) + 64, False, None))
    if name == "vm_error":
        # the inputs on which HCOMP stops, coded with the twin header: status 5 with as many bytes as lie in front of the byte
        # (none when it is the first, all but one when it is the last); the clean ones decode exactly
        for i, (d, at) in enumerate(vm_error_inputs()):
            stream = encode(d) + b"\0\0\0\0"
            if at is None and d:
                ins.append(d)
                coded.append(stream[:-4])
            cases.append(Case(f"hcomp{i}", stream, len(d) + 8, at is None, len(ins) - 1 if at is None and d else None))
    return ins, coded, cases


def interleave(cases, ins, coded, every=2, rotate=0):
    """The cases in an order in which valid and damaged streams alternate in slots of `every` (2: every pair of consecutive
    blocks -- a dual wavefront -- and so every group of 8 -- a lockstep workgroup -- holds one of each); where the catalogue
    runs out of valid cases, the two good streams at full capacity fill in.  rotate: the same order, begun `rotate` blocks
    later, so that every stream sits in another slot of its workgroup and, for an odd rotate, in the other half of its
    wavefront.  The length is a multiple of `every`."""
    valid = [c for c in cases if c.valid]
    bad = [c for c in cases if not c.valid]
    fill = [Case(f"in{s}.good", coded[s] + b"\0\0\0\0", len(ins[s]) + 64, True, s) for s in range(len(ins))]
    out, v, k = [], 0, 0
    while bad or v < len(valid) or len(out) % every:
        if len(out) % every == 0 or not bad:
            if v < len(valid):
                out.append(valid[v])
                v += 1
            else:
                out.append(fill[k % len(fill)])
                k += 1
        else:
            out.append(bad.pop(0))
    rotate %= len(out)
    return out[rotate:] + out[:rotate]


def classify(case, ins, want):
    """The outcome class of a case given decode_limited's (status, bytes, consumed)."""
    st, out, used = want
    if st == 0 and used > 0:
        return "end of stream"
    if st == 0:
        garbage = not case.valid and (case.src is None or out != ins[case.src][:len(out)])
        return "capacity, garbage" if garbage else "capacity"
    return {2: "corrupt", 5: "hcomp error", 6: "end of input"}[st]
