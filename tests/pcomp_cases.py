"""TEST INFRASTRUCTURE shared by the tests of the device's generic post-processor -- the archive's own PCOMP program translated to
HIP by host/codegen.cpp and run a lane per stream by device/pcomp_kernel.h through engine_pcomp (test_emu_pcomp.py,
test_gpu_pcomp.py, fuzz_pcomp.py): hand-written ZPAQL programs, the standard methods' programs with valid and damaged streams,
seeded stream batches and size hints.  Nothing of the machine is read.  What a stream must become is always what the host's
interpreter makes of it (zpq_pcomp_host); on the CPU that interpreter is held to the reference's (test_emu_pcomp.py).

Every loop of every program here is bounded by its input, except NO_EXIT, which never goes to a GPU."""
from __future__ import annotations

import functools
import random
import re
from typing import NamedTuple, Optional, Tuple

import lz77_decode_cases as dc
import lz77_hash_cases as hc

EOS_GUARD = "a> 255 if halt endif "            # a program that ignores the end-of-segment call (a = 0xFFFFFFFF)


class Program(NamedTuple):
    name: str
    ph: int
    pm: int
    text: str                 # ZPAQL between "pcomp x ;" and "end"; "@name:" defines a byte address, "lj @name" jumps there
    gpu: bool = True          # among the (at most ten) programs the GPU test compiles


# ---- the control-flow forms: sections that read the input byte from c, write with out and fall through to what follows ----
FLOW_SECTIONS = (
    ("if", "a=c a> 100 if a= 1 out else a= 2 out endif a=c a< 50 ifnot a= 3 out endif a=c a== 7 ifnot a= 4 out else a= 5 out endif "
           "a=c a> 200 ifl a= 6 out elsel a= 7 out endif a=c a< 20 ifnotl a= 8 out endif a=c a== 0 ifl a= 9 out else a= 10 out endif "
           "a=c a== 1 if a= 11 out elsel a= 12 out endif a=c a< 128 ifnotl a= 13 out elsel a= 14 out endif "),
    ("until", "a=c a&= 7 a++ d=a do a=d out d-- a=d a== 0 until "),
    # forward over code, backward as a loop of at most four rounds, forward out of an if
    ("lj", "a=c a> 127 if lj @fwd endif a= 20 out @fwd: a= 21 out a=c a&= 3 d=a @top: a=d out a== 0 ifnot d-- lj @top endif "
           "a=c a&= 1 a== 1 if lj @odd endif a= 22 out @odd: "),
    # a jump into the operand of "a= 57" (57 = out): the instruction at its pc + 1 is decoded too, so "a= 57" must `goto` its successor
    ("overlap", "a=c a> 99 if jmp 1 endif a= 57 out "),
    # (last: its halt ends the call)
    ("forever", "a=c a&= 3 d=a do a=d out a== 0 if halt endif d-- forever "),
)


def _flow(names) -> str:
    return EOS_GUARD + "c=a " + "".join(t for n, t in FLOW_SECTIONS if n in names) + "halt"


PROGRAMS: Tuple[Program, ...] = (
    Program("cat", 0, 0, "a> 255 ifnot out endif halt"),
    Program("plus_one", 0, 0, "a> 255 ifnot a++ out endif halt"),
    # the running sum in r 0, the count of bytes in r 255, written low byte first at the end-of-segment call
    Program("delta", 0, 0, "a> 255 ifnot b=a a=r 0 a+=b r=a 0 out a=r 255 a++ r=a 255 else a=r 255 out a>>= 8 out a>>= 8 out a>>= 8 out endif halt"),
    # (count, byte) pairs; c = 1 when the count is in d
    Program("rle", 0, 0, "a> 255 if c=0 halt endif b=a a=c a== 0 if d=b c++ else c=0 a=d a> 0 if do a=b out d-- a=d a> 0 while endif endif halt"),
    # everything is kept in M and leaves backwards at the end-of-segment call (M wraps beyond 2^16 bytes)
    Program("reverse", 0, 16, "a> 255 ifnot *b=a b++ halt endif a=b a== 0 if halt endif do b-- a=*b out a=b a> 0 while halt"),
    # H and M of one element each: every index is masked to 0
    Program("ph0_pm0", 0, 0, EOS_GUARD + "b=a c=a c++ d=a d-- *b=a a+=*c *d=a a=*d hashd a=*d out a>>= 8 out a=*b hash out b<>a a=*c out a=b out halt"),
    # b down from 0, c down in threes, d up in threes past H's four elements; reads come back through other indices than the writes
    Program("walk", 2, 3, EOS_GUARD + "b-- *b=a a=c a-= 3 c=a *c++ a=d a+= 3 d=a a=*b *d=a hashd a=*c out a=*d out a>>= 16 out a=b a>>= 24 out "
                                      "d-- d-- a=*d out d++ d++ halt"),
    Program("arith", 3, 4, EOS_GUARD + "b=a c=a *b=a hash d=a hashd a=*d out a>>= 13 out a=c a/= 0 out a=c a%= 0 out a=c a+= 7 a/= 3 out a=c a%= 7 out "
                                       "a=c a<<= 33 out a=c a*= 251 a*= 251 a*= 251 a*= 251 a>>= 255 out d=c a=c a<<=d out a>>= 8 out a= 255 a*= 255 a*= 255 a>>=d out "
                                       "a=c a*= 13 *b<>a out a=*b out a>>= 8 out a=c b<>a b<>a out a=b out a=c a*= 199 a<<= 8 a+=c c<>a *c<>a out a>>= 8 out "
                                       "a=c a&~ 15 out a=c a|= 129 a^=c out a=c a-= 200 a>>= 24 out halt"),
    Program("flow_all", 0, 0, _flow([n for n, _ in FLOW_SECTIONS])),
    # `error` on the input byte ee only
    Program("error_on_ee", 0, 0, "a== 238 if error endif a> 255 ifnot out endif halt"),
    # ---- the emulator only (the GPU compiles ten programs): every control-flow form on its own, a path that leaves the program ----
    *(Program("flow_" + n, 0, 0, _flow([n]), False) for n, _ in FLOW_SECTIONS),
    Program("leaves_on_fd", 0, 0, "a== 253 if jmp 100 endif a> 255 ifnot out endif halt", False),
)
GPU_PROGRAMS = tuple(p for p in PROGRAMS if p.gpu)
assert len(GPU_PROGRAMS) == 10
# a loop without an exit through a backward lj: the device's answer is status 5 when its budget of backward jumps is spent, the
# host's is its step limit.  CPU ONLY.
NO_EXIT = Program("no_exit", 0, 0, "@top: b++ lj @top", False)


# the input byte on which a program stops with an error (the device: a status, and the whole batch goes back to the host)
STOP_BYTE = {"error_on_ee": 0xEE, "leaves_on_fd": 0xFD}


def by_name(name: str) -> Program:
    return next(p for p in PROGRAMS + (NO_EXIT,) if p.name == name)


def _config(ph: int, pm: int, text: str) -> str:
    return "comp 0 0 %d %d 0 hcomp halt pcomp x ; %s end" % (ph, pm, text)


def config(p: Program) -> str:
    """The whole ZPAQL source of a stored block that carries the program (labels resolved)."""
    return _config(p.ph, p.pm, _resolved(p))


@functools.lru_cache(maxsize=None)
def _resolved(p: Program) -> str:
    """"@name:" / "lj @name" -> byte addresses: an address is the length of what is assembled in front of it (every lj is three
    bytes whatever its operand; an if that is still open there assembles all the same)."""
    import zpaq_amd as z
    words = p.text.split()
    at = {}
    for i, w in enumerate(words):
        if w.startswith("@") and w.endswith(":"):
            prefix = " ".join("0" if x.startswith("@") else x for x in words[:i] if not x.endswith(":"))
            at[w[:-1]] = len(z.assemble(_config(p.ph, p.pm, prefix))[1]) - 3           # less the length bytes and the closing 0
    return " ".join(str(at[w]) if w.startswith("@") else w for w in words if not w.endswith(":"))


@functools.lru_cache(maxsize=None)
def code(p: Program) -> bytes:
    """The program's bytes without the two length bytes (what zpq_pcomp_device / zpq_pcomp_host / zpq_pcomp_source take)."""
    import zpaq_amd as z
    return z.assemble(config(p))[1][2:]


# ---- streams ----
LENGTHS = (1000, 0, 70000, 1, 2, 63, 64, 65)         # the order of a batch: its first four hold the longest, the empty and a one-byte stream
BATCHES = (1, 4, 64, 65, 130)


def _bytes(n: int, seed: int) -> bytes:
    return random.Random(seed).randbytes(n)


@functools.lru_cache(maxsize=None)
def batch(n: int, seed: int = 1, avoid: Optional[int] = None) -> Tuple[bytes, ...]:
    """n streams of the lengths 0, 1, 2, 63, 64, 65, 1 000 and 70 000 in turn -- 70 000 twice per batch at most, then a few hundred
    -- of seeded bytes without the byte `avoid`."""
    out = []
    for i in range(n):
        ln = LENGTHS[i % 8]
        if ln == 70000 and i >= 16:
            ln = 300 + i
        s = _bytes(ln, 1000 * seed + i)
        if avoid is not None:
            s = s.replace(bytes([avoid]), bytes([avoid ^ 1]))
        out.append(s)
    return tuple(out)


def rle_forcing_a_retry() -> bytes:
    """1 000 pairs of count 255: 255 000 bytes from 2 000, more than the 8 * 2 000 + 65 536 of a first attempt without a hint."""
    return b"".join(bytes([255, k & 255]) for k in range(1000))


def hints_for(wants, kind: str):
    """Size hints for outputs of the sizes of `wants`: exact, zero (unknown), too small by half, or the three in turn."""
    n = [len(w) for w in wants]
    if kind == "exact":
        return n
    if kind == "zero":
        return [0] * len(n)
    if kind == "half":
        return [x // 2 for x in n]
    assert kind == "mixed"
    return [(x, 0, x // 2)[i % 3] for i, x in enumerate(n)]


HINT_BEYOND_32_BITS = 1 << 32


def engine_cap(hint: int, in_len: int) -> int:
    """The output capacity engine_pcomp gives a lane on its first attempt."""
    return (hint if hint else 8 * in_len) + 65536


def engine_declines_cap(cap: int) -> bool:
    return cap > 0xFFFFFFF0


def expected(p: Program, stream: bytes):
    """(return code, bytes) of the host's interpreter."""
    import zpaq_amd as z
    rc, out, _ = z.pcomp_host(code(p), p.ph, p.pm, stream, cap=max(1 << 20, 300 * len(stream)))
    return rc, out


# ---- the standard methods' programs ----
STD_METHODS = ("1", "2", "3", "3,128,1", "x0,7ci1", "x0,4")


@functools.lru_cache(maxsize=None)
def std_blocks():
    from zpaq_amd import corpus
    import e8e9_cases as ec
    return (corpus.block("text", 3000, 41).tobytes(), ec.x86_like(2500, 42), corpus.block("records", 1, 43).tobytes(), b"",
            corpus.block("zeros", 700, 44).tobytes(), corpus.block("text", 65, 45).tobytes())


@functools.lru_cache(maxsize=None)
def std_program(method: str):
    """(xmethod, Program-like tuple) of a standard method: its PCOMP program as zpq_method_to_header gives it."""
    import zpaq_amd as z
    xm = method if method[0] == "x" else z.expand_method(method, std_blocks()[0])
    h, pc, _ = z.method_to_header(xm)
    assert len(pc) > 3 and len(pc) - 2 == pc[0] + 256 * pc[1]
    return xm, h[4], h[5], pc[2:]


@functools.lru_cache(maxsize=None)
def std_valid(method: str):
    """(streams of zpq_preprocess_block, the blocks they were made from)."""
    xm = std_program(method)[0]
    return tuple(hc.preprocess(xm, b)[0] for b in std_blocks()), std_blocks()


@functools.lru_cache(maxsize=None)
def std_damaged(method: str):
    """(name, stream, gpu) -- the valid streams' damaged relatives.  gpu: the device program ends them by itself within the input's
    own bounds (status 0 under guard pages, test_emu_pcomp.py holds the flag to that); the others spend the budget of backward
    jumps or stop with a status and stay on the CPU."""
    xm = re.match(r"x[0-9,]*[0-9]", std_program(method)[0]).group(0)          # the pre-processor's arguments, without the model
    args = dc.args_of(xm)
    streams, _ = std_valid(method)
    s0 = streams[0]
    bwt = args[1] in (3, 7)                     # (what is left of a BWT stream's idx sends the program counting to 2^32: the budget)
    out = [("truncated tail", s0[:len(s0) - 7], not bwt), ("random bytes", _bytes(600, 77), not bwt)]
    if not bwt:
        out.append(("truncated to one byte", s0[:1], True))
    if args[1] in (1, 2, 5, 6):                 # LZ77: a match that reaches in front of the start
        ln = max(5, args[2] + 1)                # (level 2 codes lengths from its minimum match)
        out.append(("offset before the start", dc.encode(xm, [("match", ln, 1), dc._lit(3, 340)]), True))
        out.append(("offset one byte too far", dc.encode(xm, [dc._lit(3, 341), ("match", ln, 4)]), True))
    if bwt:                                     # S[0 .. n] and idx, low byte first
        body, n = s0[:-4], len(s0) - 5
        out.append(("idx 0", body + (0).to_bytes(4, "little"), True))
        out.append(("idx n + 1", body + (n + 1).to_bytes(4, "little"), True))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def std_expected(method: str, name: str):
    """(return code, bytes) of the host's interpreter for a damaged stream, and of zpq_postprocess_block: each computed once (a
    stream that spends the step limit takes the host a second or two)."""
    import zpaq_amd as z
    xm, ph, pm, pcode = std_program(method)
    s = next(s for n, s, _ in std_damaged(method) if n == name)
    return z.pcomp_host(pcode, ph, pm, s, cap=1 << 22)[:2], z.postprocess_block(xm, s)[:2]


# ---- archives of stored blocks (no model: the decoded bytes are the PP header and the stream), written here byte by byte ----
BLOCK_TAG = bytes([0x37, 0x6B, 0x53, 0x74, 0xA0, 0x31, 0x83, 0xD3, 0x8C, 0xB2, 0x28, 0xB0, 0xD3])


def stored_block(p: Optional[Program], segments, sha1: bool = True) -> bytes:
    """One ZPAQ level-2 block without components that carries program p (None: no program, PP byte 0).  segments: (name, comment,
    stream, the data the segment decodes to -- for its SHA-1) each; only the first carries the PP header."""
    import hashlib
    import zpaq_amd as z
    header, pcomp = z.assemble(config(p)) if p is not None else (z.assemble("comp 0 0 0 0 0 hcomp end")[0], b"")
    out = BLOCK_TAG + b"zPQ" + bytes([2, 1]) + header
    for k, (name, comment, stream, data) in enumerate(segments):
        out += b"\x01" + name + b"\0" + comment + b"\0\0"
        payload = (((b"\x01" + pcomp) if p is not None else b"\0") if k == 0 else b"") + stream
        for at in range(0, len(payload), 65536):
            chunk = payload[at:at + 65536]
            out += len(chunk).to_bytes(4, "big") + chunk
        out += b"\0\0\0\0" + ((b"\xfd" + hashlib.sha1(data).digest()) if sha1 else b"\xfe")
    return out + b"\xff"


# counts the bytes of the block in H[0] -- across its segments -- and writes the count's low byte at every end of segment
COUNTER = Program("counter_in_h", 0, 0, "d=0 a> 255 if a=*d out halt endif *d++ out halt", False)


@functools.lru_cache(maxsize=None)
def routing_archive(qualifying: int = 9):
    """(archive, the data it decodes to, single-segment blocks with a program): blocks of one segment with program A (delta) and B
    (plus_one) -- 5 + 4, or 2 + 1 --, one block of two segments whose program keeps a counter in H across the segment boundary, and
    two stored blocks without a program, interleaved; sizes in some comments, none in others; far below 256 KiB."""
    a, b = by_name("delta"), by_name("plus_one")
    na, nb = (5, 4) if qualifying == 9 else (2, 1)
    assert na + nb == qualifying
    s = [_bytes(200 + 317 * k, 500 + k) for k in range(14)]
    blocks = []

    def one(p, k):
        want = expected(p, s[k])[1] if p is not None else s[k]
        comment = (b"%d" % len(want)) if k % 2 else b""
        return stored_block(p, [(b"f%d" % k, comment, s[k], want)]), want

    two = (s[12] + bytes([len(s[12]) & 255]), s[13] + bytes([(len(s[12]) + len(s[13])) & 255]))
    shared = (stored_block(COUNTER, [(b"c0", b"", s[12], two[0]), (b"", b"", s[13], two[1])]), two[0] + two[1])
    order = [(a, 0), (b, 1), (None, 2), (a, 3), "shared", (b, 4), (a, 5), (None, 6), (b, 7), (a, 8), (b, 9), (a, 10)]
    left = {a.name: na, b.name: nb}
    for it in order:
        if it == "shared":
            blocks.append(shared)
            continue
        p, k = it
        if p is not None:
            if not left[p.name]:
                continue
            left[p.name] -= 1
        blocks.append(one(p, k))
    arch = b"".join(x for x, _ in blocks)
    assert len(arch) < (200 << 10)
    return arch, b"".join(w for _, w in blocks), qualifying


@functools.lru_cache(maxsize=None)
def stopping_archive(with_stop: bool):
    """Five blocks of one segment with error_on_ee; with_stop: the byte ee in the middle of the fourth (no checksums: what the call
    gives is the program's verdict)."""
    p = by_name("error_on_ee")
    streams = [_bytes(300 + 41 * k, 600 + k).replace(b"\xee", b"\xef") for k in range(5)]
    if with_stop:
        streams[3] = streams[3][:100] + b"\xee" + streams[3][100:]
    return b"".join(stored_block(p, [(b"e%d" % k, b"", st, b"")], sha1=False) for k, st in enumerate(streams)), b"".join(streams)
