"""TEST INFRASTRUCTURE shared by the tests of the hash-table LZ77 parse (test_lz77_hash_host.py, test_emu_lz77_hash.py,
test_gpu_lz77_hash.py): the parameter sets, the inputs, and thin ctypes calls of the library's parse / coder entries."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

# x<args[0]>,<level (+4: E8E9)>,<min_match>,<min_match2>,<bucket bits>,<table bits>[,<look-ahead>]: all with args[5] - args[0] < 21
METHODS = (
    "x0,1,4,0,1,15",
    "x0,1,4,0,2,16",
    "x0,1,5,0,3,20",
    "x0,5,6,0,3,20",        # E8E9 in front
    "x0,2,4,0,3,20",
    "x0,1,4,6,2,18",
    "x0,1,4,8,3,16,2",
    "x0,2,3,5,2,12,1",
    "x0,1,4,0,0,10",        # one slot per bucket, a small table: long slot lists
    "x4,1,4,0,3,24",        # checkbits 8, the largest table the device takes
)
FAR_METHODS = ("x0,2,4,0,3,20", "x0,2,4,6,3,20,1")      # level 2, tables that still hold an entry 70 000 positions later
KINDS = ("text", "lcg", "zeros", "records", "pattern")
LENGTHS = (0, 1, 3, 4, 7, 8, 9, 12, 255, 256, 257, 5000, 70000)

_u8p = C.POINTER(C.c_ubyte)
_u32p = C.POINTER(C.c_uint32)


@functools.lru_cache(maxsize=None)
def inputs():
    """Every kind at every length (65 blocks, the empty ones among them), generated once."""
    from zpaq_amd import corpus
    return tuple(corpus.block(k, n, 4000 + 17 * i + j).tobytes() for i, n in enumerate(LENGTHS) for j, k in enumerate(KINDS))


@functools.lru_cache(maxsize=None)
def far_repeat():
    """140 000 bytes whose second half repeats the first: offsets of 2^16 and more (level 2 asks a longer match of them)."""
    from zpaq_amd import corpus
    half = corpus.block("text", 50000, 91).tobytes() + corpus.block("lcg", 20000, 92).tobytes()
    return half + half


def _buf(data: bytes) -> np.ndarray:
    return np.frombuffer(bytearray(data), np.uint8).copy() if data else np.zeros(1, np.uint8)


def _lib():
    import zpaq_amd as z
    L = z.lib()
    L.zpq_lz77_tokens_host.argtypes = [C.c_char_p, _u8p, C.c_uint32, _u32p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.zpq_lz77_serialize.argtypes = [C.c_char_p, _u8p, C.c_uint32, _u32p, C.c_size_t, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.zpq_preprocess_block.argtypes = [C.c_char_p, _u8p, C.c_uint32, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    return L


def host_tokens_rc(xm: str, data: bytes):
    """zpq_lz77_tokens_host: (return code, token list as bytes, the block as the parse saw it -- E8E9 applied)."""
    L = _lib()
    buf = _buf(data)
    cap = len(data) + 4
    toks = np.zeros(4 * cap, np.uint32)
    cnt = C.c_size_t(0)
    rc = L.zpq_lz77_tokens_host(xm.encode(), buf.ctypes.data_as(_u8p), len(data), toks.ctypes.data_as(_u32p), cap, C.byref(cnt))
    return rc, toks[:4 * cnt.value].tobytes(), buf[:len(data)].tobytes()


def host_tokens(xm: str, data: bytes):
    rc, toks, seen = host_tokens_rc(xm, data)
    assert rc == 0, (xm, len(data), _lib().zpq_last_error())
    return toks, seen


def serialize(xm: str, seen: bytes, toks: bytes) -> bytes:
    """zpq_lz77_serialize: LZBuffer's codes for a token list over the (filtered) block."""
    L = _lib()
    e = _buf(seen)
    t = np.frombuffer(bytearray(toks), np.uint32).copy() if toks else np.zeros(4, np.uint32)
    out = np.empty(2 * len(seen) + 4096, np.uint8)
    ol = C.c_size_t(0)
    rc = L.zpq_lz77_serialize(xm.encode(), e.ctypes.data_as(_u8p), len(seen), t.ctypes.data_as(_u32p), len(toks) // 16, out.ctypes.data_as(_u8p), out.size, C.byref(ol))
    assert rc == 0, (xm, len(seen), L.zpq_last_error())
    return out[:ol.value].tobytes()


def preprocess(xm: str, data: bytes):
    """zpq_preprocess_block: (the stream the coder sees, the block afterwards)."""
    L = _lib()
    src = _buf(data)
    out = np.empty(2 * len(data) + 4096, np.uint8)
    ol = C.c_size_t(0)
    rc = L.zpq_preprocess_block(xm.encode(), src.ctypes.data_as(_u8p), len(data), out.ctypes.data_as(_u8p), out.size, C.byref(ol))
    assert rc == 0, (xm, len(data), L.zpq_last_error())
    return out[:ol.value].tobytes(), src[:len(data)].tobytes()
