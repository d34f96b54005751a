"""TEST INFRASTRUCTURE shared by the tests of the batched suffix sort (test_emu_sa.py on the emulator, test_gpu_sort_cases.py on
the GPU): the strings prefix doubling finds hard, the lengths, the batch shapes, the host sorter as the reference side -- and the
check of that reference side itself (check_reference_side).  numpy only, deterministic; every case has a name that the
assertion messages carry.

Why these: device/sa_kernels.hip sorts every suffix of every block of a batch as one array, by the key
block << 48 | rank[i] << 24 | rank[i + h].  A block's tail must be compared with "past the end" (rank 0), not with the next
block's bytes; names restart at each block's first sorted element; the sort is asked for 48 + bits-of-the-block-count key bits;
the loop runs until every name is distinct -- log2(n) rounds for a run of one byte, 3-4 for random bytes, and both in one batch."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

CPU_LENGTHS = tuple(n for k in (6, 8, 12) for n in ((1 << k) - 1, 1 << k, (1 << k) + 1))
GPU_LENGTHS = CPU_LENGTHS + tuple(n for n in ((1 << 16) - 1, 1 << 16, (1 << 16) + 1))
PERIODS = (2, 3, 5, 255, 256, 257)
NAIVE_LIMIT = 3000              # the longest case check_reference_side sorts naively

_u8p = C.POINTER(C.c_ubyte)
_u32p = C.POINTER(C.c_uint32)


# ---- generators ----
def lcg(n: int, seed: int = 1) -> bytes:
    """n bytes of a 32-bit linear congruential generator (its high byte)."""
    x = np.empty(n, np.uint64)
    s = (seed * 2654435761 + 12345) & 0xFFFFFFFF
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        x[i] = s >> 24
    return x.astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def _lcg_pattern(period: int) -> bytes:
    """A pattern whose period is exactly `period`: LCG bytes, the first one made unique."""
    p = bytearray(lcg(period, 100 + period))
    for i in range(1, period):
        if p[i] == p[0]:
            p[i] ^= 0x80
    return bytes(p)


def repeat(pattern: bytes, n: int) -> bytes:
    return (pattern * (n // len(pattern) + 1))[:n]


def fibonacci(n: int, a: int, b: int) -> bytes:
    """The Fibonacci word (a -> ab, b -> a): repeats of every length, none of them periodic."""
    x, y = bytes([a]), bytes([a, b])
    while len(y) < n:
        x, y = y, y + x
    return y[:n]


def thue_morse(n: int, a: int, b: int) -> bytes:
    """The Thue-Morse word: overlap-free, squares of every power of two."""
    i = np.arange(n, dtype=np.uint64)
    par = np.zeros(n, np.uint8)
    for s in range(40):
        par ^= ((i >> np.uint64(s)) & np.uint64(1)).astype(np.uint8)
    return np.where(par == 0, a, b).astype(np.uint8).tobytes()


def two_letters(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0x61, 0x63, n, dtype=np.uint8).tobytes()


def random_bytes(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def zipf_text(n: int, seed: int) -> bytes:
    """Words of a 200-word vocabulary drawn with Zipf's weights (1 / rank), single spaces between."""
    r = np.random.default_rng(seed)
    vocab = [bytes(r.integers(0x61, 0x7B, int(r.integers(1, 10)), dtype=np.uint8)) for _ in range(200)]
    w = 1.0 / np.arange(1, 201)
    out, size = [], 0
    picks = r.choice(200, size=n // 2 + 2, p=w / w.sum())
    for k in picks:
        out.append(vocab[k])
        size += len(vocab[k]) + 1
        if size >= n:
            break
    return b" ".join(out)[:n].ljust(n, b" ")


def _changed(s: bytes, at: int) -> bytes:
    b = bytearray(s)
    b[at] = (b[at] + 1) & 255
    return bytes(b)


@functools.lru_cache(maxsize=None)
def strings(n: int):
    """The hard strings at length n: a tuple of (name, bytes), every one exactly n bytes long.

    The periodic ones are repeats of a pattern cut at n bytes.  Where the period divides n the cut falls on a period's end
    (named "...whole"); the lengths come in threes (2^k - 1, 2^k, 2^k + 1) and no period of 2 or more divides two neighbours,
    so every period is met with a cut last repeat at two of each three lengths."""
    assert n >= 4
    A, B = 0x61, 0x62
    out = [("run00", bytes(n)), ("runFF", b"\xff" * n),
           ("a^(n-1)b,b>a", bytes([A]) * (n - 1) + bytes([B])), ("a^(n-1)b,b<a", bytes([B]) * (n - 1) + bytes([A])),
           ("ba^(n-1),b>a", bytes([B]) + bytes([A]) * (n - 1)), ("ba^(n-1),b<a", bytes([A]) + bytes([B]) * (n - 1))]
    for p in PERIODS:
        s = repeat(_lcg_pattern(p), n)
        tag = f"period{p}" + ("whole" if n % p == 0 else "")
        out += [(tag, s), (tag + "+middle", _changed(s, n // 2)), (tag + "+last", _changed(s, n - 1))]
    out += [("fibonacci_ab", fibonacci(n, A, B)), ("fibonacci_00FF", fibonacci(n, 0x00, 0xFF)),
            ("thue_morse_ab", thue_morse(n, A, B)), ("thue_morse_00FF", thue_morse(n, 0x00, 0xFF)),
            ("two_letters", two_letters(n, 7000 + n)),
            ("counting_up", repeat(bytes(range(256)), n)), ("counting_down", repeat(bytes(range(255, -1, -1)), n))]
    s = random_bytes((n + 1) // 2, 8000 + n)
    out.append(("s+s", (s + s)[:n]))
    s = random_bytes((n + 3) // 3, 9000 + n)
    out.append(("s+s+s[:-1]", (s + s + s[:-1])[:n]))
    t = zipf_text((n + 1) // 2, 10000 + n)
    out.append(("zipf+zipf", (t + t)[:n]))
    assert all(len(d) == n for _, d in out), [(k, len(d)) for k, d in out if len(d) != n]
    assert len({k for k, _ in out}) == len(out)
    return tuple(out)


def string(n: int, name: str) -> bytes:
    """One hard string by its name (the "whole" suffix of a periodic name may be left out)."""
    for k, d in strings(n):
        if k == name or k.replace("whole", "") == name:
            return d
    raise KeyError(name)


# ---- batch shapes: (name, ((block name, bytes), ...)) ----
def alone(lengths):
    """Every hard string at every length as a batch of one block."""
    return [(f"alone/{k}/{n}", ((f"{k}/{n}", d),)) for n in lengths for k, d in strings(n)]


def small_batches(lengths):
    """Two and three blocks: a run beside the same run (the tail of the first meets bytes that sort like "past the end"), blocks
    that need log2(n) rounds beside blocks that need three, the same string twice."""
    out = []
    for n in lengths:
        def blocks(*names):
            return tuple((f"{k}/{n}", string(n, k)) for k in names)
        out += [(f"two/run00,run00/{n}", blocks("run00", "run00")),
                (f"two/runFF,run00/{n}", blocks("runFF", "run00")),
                (f"two/period3,fibonacci_00FF/{n}", blocks("period3", "fibonacci_00FF")),
                (f"two/two_letters,period256+middle/{n}", blocks("two_letters", "period256+middle")),
                (f"three/run00,a^(n-1)b,run00/{n}", blocks("run00", "a^(n-1)b,b<a", "run00")),
                (f"three/fibonacci_ab,fibonacci_ab,thue_morse_ab/{n}", blocks("fibonacci_ab", "fibonacci_ab", "thue_morse_ab")),
                (f"three/s+s,run00,counting_up/{n}", blocks("s+s", "run00", "counting_up"))]
    return out


def many(nblocks: int, hard_len: int = 257):
    """256 or 257 blocks (either side of a power of two: 8 or 9 bits of block id in the key): mostly 1 to 40 bytes of zeros, two
    letters or random bytes, hard strings among them -- the first and the last block are runs of zeros, so a key sorted one
    bit short files the last block's suffixes among the first's."""
    r = np.random.default_rng(nblocks)
    hard = {0: "run00", 1: "run00", nblocks // 2 - 1: "fibonacci_00FF", nblocks // 2: "period2", nblocks - 2: "thue_morse_ab", nblocks - 1: "run00"}
    out = []
    for b in range(nblocks):
        if b in hard:
            n = hard_len - (b % 3)
            out.append((f"{hard[b]}/{n}", string(n, hard[b])))
            continue
        n = int(r.integers(1, 41))
        kind = b % 3
        d = bytes(n) if kind == 0 else (two_letters(n, 20000 + b) if kind == 1 else random_bytes(n, 30000 + b))
        out.append((f"{('zeros', 'two_letters', 'random')[kind]}/{n}", d))
    return (f"many/{nblocks}", tuple(out))


def boundary(hard_len: int = 4097):
    """The batch edges in one batch: empty blocks first, in the middle and last; runs of zeros of 1000, 1001 (a 1 at the end) and
    999 bytes with 1-byte blocks between; one hard string three times in a row and once more without its last byte."""
    h = string(hard_len, "fibonacci_ab")
    return (f"boundary/{hard_len}", (("empty", b""), ("zeros/1000", bytes(1000)), ("byte00", b"\x00"), ("zeros+01/1001", bytes(1000) + b"\x01"),
                                      ("byte01", b"\x01"), ("zeros/999", bytes(999)), ("empty", b""),
                                      (f"fibonacci_ab/{hard_len}", h), (f"fibonacci_ab/{hard_len}", h), ("byteFF", b"\xff"),
                                      (f"fibonacci_ab/{hard_len}", h), (f"fibonacci_ab/{hard_len - 1}", h[:-1]), ("empty", b"")))


def batch_shapes(lengths, hard_len: int = 4097):
    """Every batch shape over these lengths."""
    return alone(lengths) + small_batches(lengths) + [many(256), many(257), boundary(hard_len)]


# ---- the reference side ----
def _lib():
    import zpaq_amd as z
    L = z.lib()
    L.zpq_suffix_array_host.argtypes = [_u8p, C.c_uint32, _u32p]
    return L


def host_suffix_array(data: bytes) -> np.ndarray:
    """zpq_suffix_array_host (SA-IS): the array every kernel is judged by."""
    L = _lib()
    n = len(data)
    buf = np.frombuffer(bytes(data), np.uint8).copy() if n else np.zeros(1, np.uint8)
    out = np.zeros(max(n, 1), np.uint32)
    assert L.zpq_suffix_array_host(buf.ctypes.data_as(_u8p), n, out.ctypes.data_as(_u32p)) == 0, (n, L.zpq_last_error())
    return out[:n]


@functools.lru_cache(maxsize=4096)
def _host_cached(data: bytes) -> np.ndarray:
    a = host_suffix_array(data)
    a.setflags(write=False)
    return a


def expected(data: bytes) -> np.ndarray:
    """The host sorter's array, computed once per distinct string (read-only)."""
    return _host_cached(bytes(data))


def naive_suffix_array(data: bytes) -> np.ndarray:
    s = bytes(data)
    return np.array(sorted(range(len(s)), key=lambda i: s[i:]), np.uint32).reshape(-1)


def check_reference_side(shapes, ref=None) -> int:
    """For every distinct block of these shapes of at most NAIVE_LIMIT bytes: the host sorter equals Python's sort of the
    suffixes -- and, with the compiled reference at hand, its divsufsort (then for the longer blocks too).  Returns the number
    of blocks checked."""
    seen = set()
    for shape, blocks in shapes:
        for name, d in blocks:
            if d in seen:
                continue
            seen.add(d)
            host = expected(d)
            if len(d) <= NAIVE_LIMIT:
                assert (host == naive_suffix_array(d)).all(), ("host sorter against the naive sort", shape, name)
            if ref is not None and len(d):
                assert (host.astype(np.int64) == ref.divsufsort(d).astype(np.int64)).all(), ("host sorter against divsufsort", shape, name)
    return len(seen)
