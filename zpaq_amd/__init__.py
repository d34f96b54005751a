"""zpaq_amd -- MI355X-native ZPAQ context-mixing coder (hot path of libzpaq 7.15).

Python is plumbing here: this module is a ctypes mirror of the C ABI in
``include/zpaq_amd.h`` (same entry points, same argument meaning, same error
behaviour), used by the tests and by ``bench.py``.  The product is
``zpaq_amd/libzpaq_amd.so`` (HIP kernels for gfx950 + C++ host library, built
in-tree by ``zpaq_amd/csrc/Makefile``).

There is no CPU fallback: if the shared library is missing, or no gfx950 device
is present, the modelled path raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

__all__ = [
    "ZpaqError", "lib", "library_path", "version", "init", "device_count", "shutdown", "set_kernel",
    "set_state_budget", "Plan", "encode_batch", "decode_batch", "compress_blocks", "compress_block",
    "decompress", "sha1", "expand_method", "method_to_header", "assemble", "table", "selftest",
    "last_timing", "STATUS",
]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBNAME = "libzpaq_amd.so"
_u8p = C.POINTER(C.c_ubyte)

STATUS = {0: "OK", 1: "NOMEM", 2: "CORRUPT", 3: "OVERFLOW", 4: "HEADER", 5: "VM", 6: "EOF", 7: "DEVICE",
          8: "UNSUPPORTED", 9: "ARG"}


class ZpaqError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[{STATUS.get(code, code)}] {msg}")
        self.code = code


def library_path() -> str:
    # ZPAQ_AMD_LIB selects an alternative in-tree build (e.g. the cycle-profiling variant)
    return os.path.join(_HERE, os.environ.get("ZPAQ_AMD_LIB", _LIBNAME))


_lib = None


def lib():
    """The loaded C-ABI library; raises loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `make -C zpaq_amd/csrc` (or __graft_entry__.build()). "
            "zpaq_amd has no pure-Python or CPU fallback for the coder.")
    L = C.CDLL(path)
    L.zpq_last_error.restype = C.c_char_p
    L.zpq_version.restype = C.c_char_p
    L.zpq_plan_create.argtypes = [_u8p, C.c_size_t, C.POINTER(C.c_void_p)]
    L.zpq_plan_destroy.argtypes = [C.c_void_p]
    L.zpq_plan_ncomp.argtypes = [C.c_void_p]
    L.zpq_plan_memory.argtypes = [C.c_void_p]
    L.zpq_plan_memory.restype = C.c_double
    L.zpq_plan_state_bytes.argtypes = [C.c_void_p]
    L.zpq_plan_state_bytes.restype = C.c_uint64
    L.zpq_plan_algo_bytes_per_byte.argtypes = [C.c_void_p]
    L.zpq_plan_algo_bytes_per_byte.restype = C.c_double
    L.zpq_set_state_budget.argtypes = [C.c_uint64]
    L.zpq_sha1.argtypes = [_u8p, C.c_uint64, _u8p]
    L.zpq_sha1.restype = None
    L.zpq_table.restype = C.c_size_t
    L.zpq_table.argtypes = [C.c_int, C.c_void_p, C.c_size_t]
    L.zpq_decompress.argtypes = [_u8p, C.c_uint64, _u8p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.zpq_encode_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                    C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                    C.c_void_p, C.c_void_p, C.c_int]
    L.zpq_decode_device.argtypes = L.zpq_encode_device.argtypes
    L.zpq_last_hash_parse_blocks.restype = C.c_uint32
    L.zpq_last_hash_parse_blocks.argtypes = []
    L.zpq_last_device_coded_blocks.restype = C.c_uint32
    L.zpq_last_device_coded_blocks.argtypes = []
    L.zpq_lz77_serialize_device.argtypes = [C.c_char_p, C.POINTER(_u8p), C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_size_t),
                                            C.c_uint32, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.zpq_postprocess_block.argtypes = [C.c_char_p, _u8p, C.c_uint32, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.zpq_lz77_decode_device.argtypes = [C.c_char_p, C.POINTER(_u8p), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(_u8p), C.POINTER(C.c_size_t),
                                         C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    L.zpq_last_device_unlz_segments.restype = C.c_uint32
    L.zpq_last_device_unlz_segments.argtypes = []
    L.zpq_lz77_decode_device_wide.argtypes = L.zpq_lz77_decode_device.argtypes
    L.zpq_last_device_unlz_wide_segments.restype = C.c_uint32
    L.zpq_last_device_unlz_wide_segments.argtypes = []
    L.zpq_last_unlz_wide_pieces.restype = None
    L.zpq_last_unlz_wide_pieces.argtypes = [C.POINTER(C.c_uint32)]
    L.zpq_last_unlz_wide_rounds.restype = C.c_uint32
    L.zpq_last_unlz_wide_rounds.argtypes = []
    L.zpq_bwt_decode_device.argtypes = [C.c_char_p, C.POINTER(_u8p), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(_u8p), C.POINTER(C.c_size_t),
                                        C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    L.zpq_bwt_decode_device_wide.argtypes = L.zpq_bwt_decode_device.argtypes
    L.zpq_last_device_unbwt_segments.restype = C.c_uint32
    L.zpq_last_device_unbwt_segments.argtypes = []
    L.zpq_e8e9_decode_device.argtypes = [C.c_char_p, C.POINTER(_u8p), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(_u8p), C.POINTER(C.c_size_t),
                                         C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    L.zpq_last_device_une8_segments.restype = C.c_uint32
    L.zpq_last_device_une8_segments.argtypes = []
    L.zpq_e8e9.argtypes = [_u8p, C.c_uint32]
    L.zpq_e8e9.restype = None
    L.zpq_e8e9_device.argtypes = [C.POINTER(_u8p), C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(C.c_int32)]
    L.zpq_last_device_e8_blocks.argtypes = []
    L.zpq_last_device_e8_blocks.restype = C.c_uint32
    L.zpq_e8e9_decode_device_wide.argtypes = L.zpq_e8e9_decode_device.argtypes
    L.zpq_last_device_une8_wide_segments.restype = C.c_uint32
    L.zpq_last_device_une8_wide_segments.argtypes = []
    L.zpq_pcomp_device.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(_u8p), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint64),
                                   C.POINTER(_u8p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    L.zpq_pcomp_host.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, _u8p, C.c_uint32, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.zpq_last_device_pcomp_segments.restype = C.c_uint32
    L.zpq_last_device_pcomp_segments.argtypes = []
    _frag = [C.POINTER(_u8p), C.POINTER(C.c_uint64), C.c_uint32, C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
             C.POINTER(C.c_uint32), _u8p, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.zpq_fragment_host.argtypes = _frag
    L.zpq_fragment_device.argtypes = _frag
    L.zpq_fragment_limits.argtypes = [C.c_int, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.zpq_fragment_limits.restype = None
    L.zpq_suffix_array_device_wide.argtypes = [_u8p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.zpq_preprocess_block_device_wide.argtypes = [C.c_char_p, _u8p, C.c_uint32, _u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.zpq_last_wide_sort_blocks.restype = C.c_uint32
    L.zpq_last_wide_sort_blocks.argtypes = []
    L.zpq_last_wide_sort_rounds.restype = C.c_uint32
    L.zpq_last_wide_sort_rounds.argtypes = []
    L.zpq_lz77_parse_device_wide.argtypes = [C.c_char_p, _u8p, C.c_uint32, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]
    L.zpq_last_wide_parse_blocks.restype = C.c_uint32
    L.zpq_last_wide_parse_blocks.argtypes = []
    L.zpq_last_wide_parse_pieces.restype = None
    L.zpq_last_wide_parse_pieces.argtypes = [C.POINTER(C.c_uint32)]
    L.zpq_wide_stage_bytes.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.zpq_last_fragment_rounds.restype = C.c_uint32
    L.zpq_last_fragment_rounds.argtypes = []
    L.zpq_fragment_analyze.restype = C.c_uint32
    L.zpq_fragment_analyze.argtypes = [_u8p, C.c_uint64, C.c_uint32, _u8p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    _lib = L
    return L


def _check(rc: int):
    if rc != 0:
        raise ZpaqError(rc, lib().zpq_last_error().decode("latin1"))


def _arr(b) -> np.ndarray:
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
    b = bytes(b)
    return np.frombuffer(b, dtype=np.uint8).copy() if len(b) else np.zeros(0, np.uint8)


def _p(a: np.ndarray):
    return a.ctypes.data_as(_u8p)


def version() -> str:
    return lib().zpq_version().decode()


def device_count() -> int:
    return int(lib().zpq_device_count())


def init(device: Optional[int] = None):
    """zpq_init: bind to one GPU (default LOCAL_RANK, else 0)."""
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    _check(lib().zpq_init(int(device)))


def shutdown():
    lib().zpq_shutdown()


def set_kernel(which: int):
    """0 auto, 1 generic one-lane kernel, 2 generic wave-parallel kernel, 3 per-header specialised kernel."""
    _check(lib().zpq_set_kernel(int(which)))


def set_state_budget(nbytes: int):
    _check(lib().zpq_set_state_budget(int(nbytes)))


def selftest() -> List[int]:
    out = (C.c_int32 * 8)()
    _check(lib().zpq_selftest(out))
    return list(out)


def last_timing() -> Tuple[float, float, int]:
    a, b, n = C.c_float(0), C.c_float(0), C.c_uint32(0)
    lib().zpq_last_timing(C.byref(a), C.byref(b), C.byref(n))
    return a.value, b.value, n.value


class Plan:
    """zpq_plan: a parsed block header (ZPAQL::read + Predictor::init sizing)."""

    def __init__(self, header):
        h = _arr(header)
        self.header = h.tobytes()
        self._h = C.c_void_p()
        _check(lib().zpq_plan_create(_p(h), h.size, C.byref(self._h)))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().zpq_plan_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def ncomp(self) -> int:
        return int(lib().zpq_plan_ncomp(self._h))

    @property
    def memory(self) -> float:
        return float(lib().zpq_plan_memory(self._h))

    @property
    def state_bytes(self) -> int:
        return int(lib().zpq_plan_state_bytes(self._h))

    @property
    def algo_bytes_per_byte(self) -> float:
        return float(lib().zpq_plan_algo_bytes_per_byte(self._h))


def encode_batch(plans: Sequence[Plan], inputs: Sequence, out_cap: Optional[Sequence[int]] = None,
                 check: bool = True):
    """zpq_encode_batch -> list of coded byte strings (and statuses if check=False)."""
    n = len(inputs)
    if isinstance(plans, Plan):
        plans = [plans] * n
    ins = [_arr(x) for x in inputs]
    caps = [int(c) for c in out_cap] if out_cap is not None else [a.size + a.size // 4 + 4096 for a in ins]
    outs = [np.empty(max(c, 1), np.uint8) for c in caps]
    PA = (C.c_void_p * n)(*[p._h for p in plans])
    IA = (_u8p * n)(*[_p(a) for a in ins])
    OA = (_u8p * n)(*[_p(a) for a in outs])
    IL = (C.c_uint32 * n)(*[a.size for a in ins])
    OC = (C.c_uint32 * n)(*caps)
    OL = (C.c_uint32 * n)()
    ST = (C.c_int32 * n)()
    rc = lib().zpq_encode_batch(PA, IA, IL, n, OA, OC, OL, ST)
    if check:
        _check(rc)
        return [outs[i][:OL[i]].tobytes() for i in range(n)]
    return [outs[i][:min(OL[i], caps[i])].tobytes() for i in range(n)], list(ST), list(OL)


def decode_batch(plans: Sequence[Plan], payloads: Sequence, max_out: Sequence[int], check: bool = True):
    """zpq_decode_batch -> list of (decoded bytes incl. PP header, consumed)."""
    n = len(payloads)
    if isinstance(plans, Plan):
        plans = [plans] * n
    ins = [_arr(x) for x in payloads]
    caps = [int(c) for c in max_out]
    outs = [np.empty(max(c, 1), np.uint8) for c in caps]
    PA = (C.c_void_p * n)(*[p._h for p in plans])
    IA = (_u8p * n)(*[_p(a) for a in ins])
    OA = (_u8p * n)(*[_p(a) for a in outs])
    IL = (C.c_uint32 * n)(*[a.size for a in ins])
    OC = (C.c_uint32 * n)(*caps)
    OL = (C.c_uint32 * n)()
    CO = (C.c_uint32 * n)()
    ST = (C.c_int32 * n)()
    rc = lib().zpq_decode_batch(PA, IA, IL, n, OA, OC, OL, CO, ST)
    if check:
        _check(rc)
        return [(outs[i][:OL[i]].tobytes(), int(CO[i])) for i in range(n)]
    return [(outs[i][:OL[i]].tobytes(), int(CO[i])) for i in range(n)], list(ST)


def compress_blocks(blocks: Sequence, method: str, filenames: Optional[Sequence[Optional[str]]] = None,
                    comments: Optional[Sequence[Optional[str]]] = None, dosha1: bool = True,
                    inputs_after: Optional[list] = None) -> List[bytes]:
    """Batched libzpaq::compressBlock: one ZPAQ block (archive bytes) per input buffer.  inputs_after: a list that receives the
    input buffers as the call left them (E8E9 is applied in place, as the reference does)."""
    n = len(blocks)
    ins = [_arr(x).copy() for x in blocks]      # the call may modify inputs in place (E8E9)
    caps = [a.size + a.size // 4 + 8192 for a in ins]
    outs = [np.empty(c, np.uint8) for c in caps]

    def cstrs(v):
        if v is None:
            return None
        return (C.c_char_p * n)(*[None if s is None else (s if isinstance(s, bytes) else str(s).encode()) for s in v])

    IA = (_u8p * n)(*[_p(a) for a in ins])
    IL = (C.c_uint32 * n)(*[a.size for a in ins])
    OA = (_u8p * n)(*[_p(a) for a in outs])
    OC = (C.c_uint64 * n)(*caps)
    OL = (C.c_uint64 * n)()
    rc = lib().zpq_compress_blocks(method.encode(), IA, IL, n, cstrs(filenames), cstrs(comments), int(dosha1),
                                   OA, OC, OL)
    if rc == 3:   # OVERFLOW: sizes are in OL, retry once with exact capacities
        caps = [int(x) for x in OL]
        outs = [np.empty(max(c, 1), np.uint8) for c in caps]
        OA = (_u8p * n)(*[_p(a) for a in outs])
        OC = (C.c_uint64 * n)(*caps)
        ins = [_arr(x).copy() for x in blocks]
        IA = (_u8p * n)(*[_p(a) for a in ins])
        rc = lib().zpq_compress_blocks(method.encode(), IA, IL, n, cstrs(filenames), cstrs(comments), int(dosha1),
                                       OA, OC, OL)
    _check(rc)
    if inputs_after is not None:
        inputs_after[:] = [a.tobytes() for a in ins]
    return [outs[i][:OL[i]].tobytes() for i in range(n)]


def last_hash_parse_blocks() -> int:
    """Blocks of the last compress_blocks call whose hash-table LZ77 parse (method 1, ...) ran on the device."""
    return int(lib().zpq_last_hash_parse_blocks())


def last_device_coded_blocks() -> int:
    """Blocks of the last compress_blocks call whose LZ77 stream was written on the device (ZPAQ_AMD_DEVICE_CODES)."""
    return int(lib().zpq_last_device_coded_blocks())


def lz77_serialize_device(xmethod: str, blocks: Sequence, tokens: Sequence, caps: Optional[Sequence[int]] = None):
    """zpq_lz77_serialize_device: LZBuffer's codes of token lists (bytes, 16 per match: i, off, len, blit) over already
    filtered blocks, written on the device.  Returns (return code, streams, sizes); caps = the output capacities
    (default: room for any valid list)."""
    n = len(blocks)
    ins = [_arr(x) if len(x) else np.zeros(1, np.uint8) for x in blocks]
    tks = [np.frombuffer(bytes(t), np.uint32).copy() if len(t) else np.zeros(4, np.uint32) for t in tokens]
    caps = [2 * a.size + 4096 for a in ins] if caps is None else [int(c) for c in caps]
    outs = [np.zeros(max(c, 1), np.uint8) for c in caps]
    u32p = C.POINTER(C.c_uint32)
    IA = (_u8p * n)(*[_p(a) for a in ins])
    IL = (C.c_uint32 * n)(*[len(x) for x in blocks])
    TA = (u32p * n)(*[t.ctypes.data_as(u32p) for t in tks])
    TN = (C.c_size_t * n)(*[len(t) // 16 for t in tokens])
    OA = (_u8p * n)(*[_p(a) for a in outs])
    OC = (C.c_size_t * n)(*caps)
    OL = (C.c_size_t * n)()
    rc = lib().zpq_lz77_serialize_device(xmethod.encode(), IA, IL, TA, TN, n, OA, OC, OL)
    sizes = [int(x) for x in OL]
    return rc, [outs[i][:min(sizes[i], caps[i])].tobytes() for i in range(n)], sizes


def suffix_array_device_wide(data, spare: int = 0, fill: int = 0):
    """zpq_suffix_array_device_wide: the suffix array of one buffer of any length below 2^31 from the device's wide sorter.
    Returns (return code, array -- n + spare entries of uint32, pre-filled with `fill`, as the call left them)."""
    a = data if isinstance(data, np.ndarray) else _arr(data)
    n = int(a.size)
    src = a if n else np.zeros(1, np.uint8)
    out = np.full(max(n + spare, 1), fill, np.uint32)
    rc = lib().zpq_suffix_array_device_wide(_p(src), n, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return rc, out[:n + spare]


def preprocess_block_device_wide(xmethod: str, data, cap: int, guard: int = 0, fill: int = 0):
    """zpq_preprocess_block_device_wide: zpq_preprocess_block's stream of one buffer, the sort by the device's wide sorter.
    `data` (a writable uint8 array, or bytes that are copied) is E8E9-filtered in place where the method says so.  `guard` bytes of
    `fill` lie behind the `cap` bytes of output.  Returns (return code, the buffer -- cap + guard bytes, as the call left it --,
    size)."""
    a = data if isinstance(data, np.ndarray) else _arr(data)
    n = int(a.size)
    src = a if n else np.zeros(1, np.uint8)
    out = np.full(max(int(cap) + guard, 1), fill, np.uint8)
    ol = C.c_size_t(0)
    rc = lib().zpq_preprocess_block_device_wide(xmethod.encode(), _p(src), n, _p(out), int(cap), C.byref(ol))
    return rc, out[:int(cap) + guard].tobytes(), int(ol.value)


def lz77_parse_device_wide(xmethod: str, data, cap: int, spare: int = 0, fill: int = 0):
    """zpq_lz77_parse_device_wide: the LZ77 parse of one buffer of any length below 2^31 on the device, behind the wide sorter.
    `data` (a writable uint8 array, or bytes that are copied) is E8E9-filtered in place where the method says so.  `spare` token
    slots of `fill` words lie behind the `cap` slots of the list.  Returns (return code, the buffer -- 4 x (cap + spare) words of
    uint32, as the call left it --, count)."""
    a = data if isinstance(data, np.ndarray) else _arr(data)
    n = int(a.size)
    src = a if n else np.zeros(1, np.uint8)
    out = np.full(max(4 * (int(cap) + spare), 4), fill, np.uint32)
    cnt = C.c_size_t(0)
    rc = lib().zpq_lz77_parse_device_wide(xmethod.encode(), _p(src), n, out.ctypes.data_as(C.POINTER(C.c_uint32)), int(cap), C.byref(cnt))
    return rc, out[:4 * (int(cap) + spare)], int(cnt.value)


def last_wide_parse_blocks() -> int:
    """Blocks of the last compress_blocks call whose LZ77 parse ran on the device behind the wide sorter (ZPAQ_AMD_DEVICE_PARSE_WIDE)."""
    return int(lib().zpq_last_wide_parse_blocks())


def last_wide_parse_pieces() -> Tuple[int, int, int, int]:
    """Of this process's last wide parse: pieces, adopted whole, re-joined after a re-walk, own tokens only or nothing."""
    out = (C.c_uint32 * 4)()
    lib().zpq_last_wide_parse_pieces(out)
    return tuple(int(x) for x in out)


def wide_stage_bytes(xmethod: str, n: int) -> Tuple[int, int]:
    """zpq_wide_stage_bytes: what a wide call for n bytes holds on the device -- (the sort alone, the sort with parse and codes)."""
    out = (C.c_uint64 * 2)()
    _check(lib().zpq_wide_stage_bytes(xmethod.encode(), int(n), out))
    return int(out[0]), int(out[1])


def last_wide_sort_blocks() -> int:
    """Blocks of the last compress_blocks call that the device's wide sorter sorted (ZPAQ_AMD_DEVICE_SORT_WIDE)."""
    return int(lib().zpq_last_wide_sort_blocks())


def last_wide_sort_rounds() -> int:
    """Doubling rounds of this process's last wide sort."""
    return int(lib().zpq_last_wide_sort_rounds())


def postprocess_block(xmethod: str, stream, cap: Optional[int] = None):
    """zpq_postprocess_block: the method's own PCOMP program over one stream on the host, the inverse of zpq_preprocess_block.
    Returns (return code, output, size)."""
    a = _arr(stream)
    src = a if a.size else np.zeros(1, np.uint8)
    ol = C.c_size_t(0)
    if cap is None:                                   # ask for the size first
        probe = np.zeros(1, np.uint8)
        rc = lib().zpq_postprocess_block(xmethod.encode(), _p(src), a.size, _p(probe), 0, C.byref(ol))
        if rc not in (0, 3):
            return rc, b"", 0
        cap = int(ol.value)
    out = np.zeros(max(int(cap), 1), np.uint8)
    rc = lib().zpq_postprocess_block(xmethod.encode(), _p(src), a.size, _p(out), int(cap), C.byref(ol))
    size = int(ol.value)
    return rc, (out[:size].tobytes() if rc == 0 else b""), size


def lz77_decode_device(xmethod: str, streams: Sequence, caps: Sequence[int], guard: int = 0, fill: int = 0, wide: bool = False):
    """zpq_lz77_decode_device: a batch of LZ77 streams (level 1 / 2, no E8E9) back into their blocks on the device
    (wide: zpq_lz77_decode_device_wide, the decoder that parses a stream in pieces).
    caps = the output capacities; `guard` bytes of `fill` lie behind each.  Returns (return code, buffers -- cap + guard bytes each,
    as the call left them --, sizes, statuses: 0 decoded, 1 declined)."""
    n = len(streams)
    ins = [_arr(x) if len(x) else np.zeros(1, np.uint8) for x in streams]
    caps = [int(c) for c in caps]
    outs = [np.full(max(c + guard, 1), fill, np.uint8) for c in caps]
    IA = (_u8p * n)(*[_p(a) for a in ins])
    IL = (C.c_uint32 * n)(*[len(x) for x in streams])
    OA = (_u8p * n)(*[_p(a) for a in outs])
    OC = (C.c_size_t * n)(*caps)
    OL = (C.c_size_t * n)()
    ST = (C.c_int32 * n)()
    entry = lib().zpq_lz77_decode_device_wide if wide else lib().zpq_lz77_decode_device
    rc = entry(xmethod.encode(), IA, IL, n, OA, OC, OL, ST)
    return rc, [outs[i][:caps[i] + guard].tobytes() for i in range(n)], [int(x) for x in OL], [int(x) for x in ST]


def lz77_decode_device_wide(xmethod: str, streams: Sequence, caps: Sequence[int], guard: int = 0, fill: int = 0):
    """zpq_lz77_decode_device_wide: lz77_decode_device through the decoder for long streams (ZPAQ_AMD_UNLZ_WIDE_PIECE sets the piece)."""
    return lz77_decode_device(xmethod, streams, caps, guard, fill, wide=True)


def last_device_unlz_wide_segments() -> int:
    """Segments of the last decompress call that the device's LZ77 decoder for long streams decoded (ZPAQ_AMD_DEVICE_UNLZ_WIDE)."""
    return int(lib().zpq_last_device_unlz_wide_segments())


def last_unlz_wide_pieces() -> Tuple[int, int, int, int]:
    """Of this process's last call of that decoder: pieces, adopted as entered, met after a serial stretch, walked to their end."""
    out = (C.c_uint32 * 4)()
    lib().zpq_last_unlz_wide_pieces(out)
    return tuple(int(x) for x in out)


def last_unlz_wide_rounds() -> int:
    """Jump rounds of the longest copy of this process's last call of that decoder."""
    return int(lib().zpq_last_unlz_wide_rounds())


def last_device_unlz_segments() -> int:
    """Segments of the last decompress call that the device's LZ77 decoder decoded (ZPAQ_AMD_DEVICE_UNLZ)."""
    return int(lib().zpq_last_device_unlz_segments())


def bwt_decode_device(xmethod: str, streams: Sequence, caps: Sequence[int], guard: int = 0, fill: int = 0):
    """zpq_bwt_decode_device: a batch of BWT streams (level 3, no E8E9, args[0] <= 4) back into their blocks on the device.
    caps = the output capacities; `guard` bytes of `fill` lie behind each.  Returns (return code, buffers -- cap + guard bytes each,
    as the call left them --, sizes, statuses: 0 decoded, 1 declined)."""
    n = len(streams)
    ins = [_arr(x) if len(x) else np.zeros(1, np.uint8) for x in streams]
    caps = [int(c) for c in caps]
    outs = [np.full(max(c + guard, 1), fill, np.uint8) for c in caps]
    IA = (_u8p * n)(*[_p(a) for a in ins])
    IL = (C.c_uint32 * n)(*[len(x) for x in streams])
    OA = (_u8p * n)(*[_p(a) for a in outs])
    OC = (C.c_size_t * n)(*caps)
    OL = (C.c_size_t * n)()
    ST = (C.c_int32 * n)()
    rc = lib().zpq_bwt_decode_device(xmethod.encode(), IA, IL, n, OA, OC, OL, ST)
    return rc, [outs[i][:caps[i] + guard].tobytes() for i in range(n)], [int(x) for x in OL], [int(x) for x in ST]


def bwt_decode_device_wide(xmethod: str, streams: Sequence, caps: Sequence[int], guard: int = 0, fill: int = 0):
    """zpq_bwt_decode_device_wide: a batch of BWT streams of the program at args[0] 5 .. 11 (xN,3, and xN,7 behind the inverse E8E9
    filter) back into their blocks on the device.  caps = the output capacities; `guard` bytes of `fill` lie behind each.  Returns
    (return code, buffers -- cap + guard bytes each, as the call left them --, sizes, statuses: 0 decoded, 1 declined)."""
    n = len(streams)
    ins = [_arr(x) if len(x) else np.zeros(1, np.uint8) for x in streams]
    caps = [int(c) for c in caps]
    outs = [np.full(max(c + guard, 1), fill, np.uint8) for c in caps]
    IA = (_u8p * n)(*[_p(a) for a in ins])
    IL = (C.c_uint32 * n)(*[len(x) for x in streams])
    OA = (_u8p * n)(*[_p(a) for a in outs])
    OC = (C.c_size_t * n)(*caps)
    OL = (C.c_size_t * n)()
    ST = (C.c_int32 * n)()
    rc = lib().zpq_bwt_decode_device_wide(xmethod.encode(), IA, IL, n, OA, OC, OL, ST)
    return rc, [outs[i][:caps[i] + guard].tobytes() for i in range(n)], [int(x) for x in OL], [int(x) for x in ST]


def last_device_unbwt_segments() -> int:
    """Segments of the last decompress call that the device's BWT decoder decoded (ZPAQ_AMD_DEVICE_UNBWT)."""
    return int(lib().zpq_last_device_unbwt_segments())


def e8e9_decode_device(xmethod: str, streams: Sequence, caps: Sequence[int], guard: int = 0, fill: int = 0, wide: bool = False):
    """zpq_e8e9_decode_device: a batch of streams of an E8E9 method (args[1] 4 .. 7, the BWT at args[0] <= 4) back into their blocks
    on the device (wide: zpq_e8e9_decode_device_wide, args[1] 5 / 6 through the decoder that parses a stream in pieces).
    caps = the output capacities; `guard` bytes of `fill` lie behind each.  Returns (return code, buffers -- cap +
    guard bytes each, as the call left them --, sizes, statuses: 0 decoded, 1 declined)."""
    n = len(streams)
    ins = [_arr(x) if len(x) else np.zeros(1, np.uint8) for x in streams]
    caps = [int(c) for c in caps]
    outs = [np.full(max(c + guard, 1), fill, np.uint8) for c in caps]
    IA = (_u8p * n)(*[_p(a) for a in ins])
    IL = (C.c_uint32 * n)(*[len(x) for x in streams])
    OA = (_u8p * n)(*[_p(a) for a in outs])
    OC = (C.c_size_t * n)(*caps)
    OL = (C.c_size_t * n)()
    ST = (C.c_int32 * n)()
    entry = lib().zpq_e8e9_decode_device_wide if wide else lib().zpq_e8e9_decode_device
    rc = entry(xmethod.encode(), IA, IL, n, OA, OC, OL, ST)
    return rc, [outs[i][:caps[i] + guard].tobytes() for i in range(n)], [int(x) for x in OL], [int(x) for x in ST]


def e8e9_decode_device_wide(xmethod: str, streams: Sequence, caps: Sequence[int], guard: int = 0, fill: int = 0):
    """zpq_e8e9_decode_device_wide: e8e9_decode_device for x.,5 / x.,6 through the decoder for long streams, the inverse filter
    behind it (ZPAQ_AMD_UNLZ_WIDE_PIECE sets the piece; last_unlz_wide_pieces / last_unlz_wide_rounds report the call)."""
    return e8e9_decode_device(xmethod, streams, caps, guard, fill, wide=True)


def e8e9(block) -> bytes:
    """zpq_e8e9: the forward E8E9 filter of a block on the host (libzpaq.cpp:6450-6459)."""
    a = _arr(block).copy() if len(block) else np.zeros(1, np.uint8)
    lib().zpq_e8e9(_p(a), len(block))
    return a[:len(block)].tobytes()


def e8e9_device(blocks: Sequence, max_steps: int = 0, guard: int = 0, fill: int = 0):
    """zpq_e8e9_device: the forward E8E9 filter of a batch of blocks on the device, in place.  The buffers lie in one arena with
    `guard` bytes of `fill` behind each.  max_steps: the walk's cap on serial steps (0: the engine's).  Returns (return code,
    buffers -- len + guard bytes each, as the call left them --, statuses: 0 filtered, 1 declined and untouched)."""
    n = len(blocks)
    offs, total = [], 0
    for b in blocks:
        offs.append(total)
        total += len(b) + guard
    arena = np.full(max(total, 1), fill, np.uint8)
    for o, b in zip(offs, blocks):
        if len(b):
            arena[o:o + len(b)] = _arr(b)
    base = arena.ctypes.data
    DA = (_u8p * n)(*[C.cast(base + o, _u8p) for o in offs])
    DL = (C.c_uint32 * n)(*[len(b) for b in blocks])
    ST = (C.c_int32 * n)()
    rc = lib().zpq_e8e9_device(DA, DL, n, int(max_steps), ST)
    return rc, [arena[o:o + len(b) + guard].tobytes() for o, b in zip(offs, blocks)], [int(x) for x in ST]


def last_device_e8_blocks() -> int:
    """Blocks of the last compress_blocks call whose forward E8E9 filter ran on the device (ZPAQ_AMD_DEVICE_E8)."""
    return int(lib().zpq_last_device_e8_blocks())


def last_device_une8_wide_segments() -> int:
    """Segments of the last decompress call that went through the decoder for long LZ77 streams and then the inverse E8E9 filter
    (ZPAQ_AMD_DEVICE_UNE8 and ZPAQ_AMD_DEVICE_UNLZ_WIDE both 1)."""
    return int(lib().zpq_last_device_une8_wide_segments())


def last_device_une8_segments() -> int:
    """Segments of the last decompress call that went through the device's inverse E8E9 filter (ZPAQ_AMD_DEVICE_UNE8)."""
    return int(lib().zpq_last_device_une8_segments())


def pcomp_device(code: bytes, ph: int, pm: int, streams: Sequence, caps: Sequence[int], hints: Optional[Sequence[int]] = None, guard: int = 0,
                 fill: int = 0):
    """zpq_pcomp_device: the PCOMP program `code` (without its two length bytes) over a batch of raw streams on the device, one lane
    per stream.  caps = the output capacities; `guard` bytes of `fill` lie behind each; hints = the expected sizes (None: all 0).
    Returns (return code, buffers -- cap + guard bytes each, as the call left them --, sizes, statuses: 0 decoded, 1 declined)."""
    n = len(streams)
    ins = [_arr(x) if len(x) else np.zeros(1, np.uint8) for x in streams]
    caps = [int(c) for c in caps]
    outs = [np.full(max(c + guard, 1), fill, np.uint8) for c in caps]
    IA = (_u8p * n)(*[_p(a) for a in ins])
    IL = (C.c_uint32 * n)(*[len(x) for x in streams])
    HI = (C.c_uint64 * n)(*[int(h) for h in (hints if hints is not None else [0] * n)])
    OA = (_u8p * n)(*[_p(a) for a in outs])
    OC = (C.c_size_t * n)(*caps)
    OL = (C.c_size_t * n)()
    ST = (C.c_int32 * n)()
    code = bytes(code)
    rc = lib().zpq_pcomp_device(code, len(code), int(ph), int(pm), IA, IL, n, HI, OA, OC, OL, ST)
    return rc, [outs[i][:caps[i] + guard].tobytes() for i in range(n)], [int(x) for x in OL], [int(x) for x in ST]


def pcomp_host(code: bytes, ph: int, pm: int, stream, cap: Optional[int] = None):
    """zpq_pcomp_host: the host's interpreter with the PCOMP program `code` (without its two length bytes) over one stream.
    Returns (return code, output, size); 5 (ZPQ_E_VM) when the program stops with an error."""
    a = _arr(stream)
    src = a if a.size else np.zeros(1, np.uint8)
    code = bytes(code)
    ol = C.c_size_t(0)
    if cap is None:                                   # ask for the size first
        probe = np.zeros(1, np.uint8)
        rc = lib().zpq_pcomp_host(code, len(code), int(ph), int(pm), _p(src), a.size, _p(probe), 0, C.byref(ol))
        if rc not in (0, 3):
            return rc, b"", 0
        cap = int(ol.value)
    out = np.zeros(max(int(cap), 1), np.uint8)
    rc = lib().zpq_pcomp_host(code, len(code), int(ph), int(pm), _p(src), a.size, _p(out), int(cap), C.byref(ol))
    size = int(ol.value)
    return rc, (out[:size].tobytes() if rc == 0 else b""), size


def last_device_pcomp_segments() -> int:
    """Segments of the last decompress call whose block's own PCOMP program ran on the device (device/pcomp_kernel.h)."""
    return int(lib().zpq_last_device_pcomp_segments())


def fragment_limits(fragment: int, blocksize: int) -> Tuple[int, int]:
    """zpq_fragment_limits: (smallest, largest) fragment of -fragment `fragment` at the method's block size."""
    lo, hi = C.c_uint32(0), C.c_uint32(0)
    lib().zpq_fragment_limits(int(fragment), int(blocksize), C.byref(lo), C.byref(hi))
    return int(lo.value), int(hi.value)


def _fragment(entry, files: Sequence, fragment: int, blocksize: int, cap: Optional[int]):
    n = len(files)
    ins = [_arr(x) if len(x) else np.zeros(1, np.uint8) for x in files]
    IA = (_u8p * max(n, 1))(*[_p(a) for a in ins])
    IL = (C.c_uint64 * max(n, 1))(*[len(x) for x in files])
    NF = (C.c_uint32 * max(n, 1))()
    total = C.c_size_t(0)
    if cap is None:                                 # ask for the count first: nothing is written when cap is too small
        rc = entry(IA, IL, n, int(fragment), int(blocksize), NF, None, None, None, None, 0, C.byref(total))
        if rc not in (0, 3):
            return rc, None, int(total.value)
        cap = int(total.value)
    fill = 0xEE
    size = np.full(cap + 1, 0xEEEEEEEE, np.uint32)
    hits = np.full(cap + 1, 0xEEEEEEEE, np.uint32)
    sha = np.full(20 * (cap + 1), fill, np.uint8)
    o1 = np.full(256 * (cap + 1), fill, np.uint8)
    u32p = C.POINTER(C.c_uint32)
    for k in range(n):
        NF[k] = 0xEEEEEEEE
    rc = entry(IA, IL, n, int(fragment), int(blocksize), NF, size.ctypes.data_as(u32p), hits.ctypes.data_as(u32p), _p(sha), _p(o1), cap,
               C.byref(total))
    t = int(total.value)
    if rc != 0:
        untouched = (all(NF[k] == 0xEEEEEEEE for k in range(n)) and bool((size == 0xEEEEEEEE).all()) and bool((hits == 0xEEEEEEEE).all())
                     and bool((sha == fill).all()) and bool((o1 == fill).all()))
        return rc, untouched, t
    assert size[cap] == 0xEEEEEEEE and hits[cap] == 0xEEEEEEEE and (sha[20 * cap:] == fill).all() and (o1[256 * cap:] == fill).all()
    out, k = [], 0
    for f in range(n):
        fr = []
        for _ in range(int(NF[f])):
            fr.append((int(size[k]), int(hits[k]), sha[20 * k:20 * k + 20].tobytes(), o1[256 * k:256 * k + 256].tobytes()))
            k += 1
        out.append(fr)
    assert k == t
    return 0, out, t


def fragment_host(files: Sequence, fragment: int, blocksize: int, cap: Optional[int] = None):
    """zpq_fragment_host: the archiver's content-defined fragments of a batch of files, by the serial scan.  Returns (return code,
    per file a list of (size, hits, sha1, o1), the batch's fragment count).  cap None: the count is asked for first.  When the call
    fails the second element says whether the output arrays were left untouched."""
    return _fragment(lib().zpq_fragment_host, files, fragment, blocksize, cap)


def fragment_device(files: Sequence, fragment: int, blocksize: int, cap: Optional[int] = None):
    """zpq_fragment_device: the same from the device (device/fragment_kernel.h)."""
    return _fragment(lib().zpq_fragment_device, files, fragment, blocksize, cap)


def last_fragment_rounds() -> int:
    """Fix-up rounds of the last fragment_device call."""
    return int(lib().zpq_last_fragment_rounds())


def fragment_analyze(o1: bytes, sz: int, hits: int, o1prev: bytes) -> Tuple[int, int, int]:
    """zpq_fragment_analyze: (final hits, text1, exe1) of a fragment against the four tables in front of it."""
    a, b = _arr(o1), _arr(o1prev)
    assert a.size == 256 and b.size == 1024
    t, x = C.c_int(0), C.c_int(0)
    h = lib().zpq_fragment_analyze(_p(a), int(sz), int(hits), _p(b), C.byref(t), C.byref(x))
    return int(h), int(t.value), int(x.value)


def compress_block(data, method: str, filename: Optional[str] = None, comment: Optional[str] = None,
                   dosha1: bool = True) -> bytes:
    return compress_blocks([data], method, [filename], [comment], dosha1)[0]


def decompress(archive, cap: Optional[int] = None) -> bytes:
    """libzpaq::decompress over a whole archive (all blocks decoded as one device batch)."""
    a = _arr(archive)
    cap = int(cap) if cap is not None else max(4 * a.size, 1 << 20)
    while True:
        out = np.empty(max(cap, 1), np.uint8)
        n = C.c_uint64(0)
        rc = lib().zpq_decompress(_p(a), a.size, _p(out), out.size, C.byref(n))
        if rc == 3 and n.value > out.size:
            cap = int(n.value)
            continue
        _check(rc)
        return out[:n.value].tobytes()


# ---- host-side pieces -------------------------------------------------------
def sha1(data) -> bytes:
    a = _arr(data)
    out = np.empty(20, np.uint8)
    lib().zpq_sha1(_p(a), a.size, _p(out))
    return out.tobytes()


def expand_method(method: str, data) -> str:
    a = _arr(data)
    buf = C.create_string_buffer(4096)
    _check(lib().zpq_expand_method(method.encode(), _p(a), C.c_uint32(a.size), buf, C.c_size_t(len(buf))))
    return buf.value.decode()


def _two_bufs(fn, first, args):
    h = np.empty(1 << 17, np.uint8)
    p = np.empty(1 << 17, np.uint8)
    hl, pl = C.c_size_t(0), C.c_size_t(0)
    _check(fn(first, args, _p(h), C.c_size_t(h.size), C.byref(hl), _p(p), C.c_size_t(p.size), C.byref(pl)))
    return h[:hl.value].tobytes(), p[:pl.value].tobytes()


def method_to_header(xmethod: str):
    """makeConfig + Compiler: "x.." -> (stored header bytes, pcomp bytes, args[9])."""
    args = (C.c_int * 9)()
    h, p = _two_bufs(lib().zpq_method_to_header, xmethod.encode(), args)
    return h, p, list(args)


def builtin_model_header(level: int) -> bytes:
    """Compressor::startBlock(int level): the stored header of min.cfg / mid.cfg / max.cfg (level 1 / 2 / 3)."""
    h = np.empty(4096, np.uint8)
    hl = C.c_size_t(0)
    _check(lib().zpq_builtin_model_header(C.c_int(level), _p(h), C.c_size_t(h.size), C.byref(hl)))
    return h[:hl.value].tobytes()


def encoder_variants(plans: Sequence[Plan], blocks: Sequence[int], longest: Sequence[int], cus: int, xcds: int = 8,
                     persist_expected: bool = True) -> List[int]:
    """zpq_encoder_variants: the encoder variant the launch policy gives every chain of a batch (no device involved)."""
    n = len(plans)
    out = (C.c_int32 * n)()
    _check(lib().zpq_encoder_variants((C.c_void_p * n)(*[p._h for p in plans]), (C.c_uint32 * n)(*blocks), (C.c_uint32 * n)(*longest),
                                      C.c_uint32(n), C.c_int(cus), C.c_int(xcds), C.c_int(int(persist_expected)), out))
    return list(out)


def assemble(config: str, args: Optional[Iterable[int]] = None):
    """Compiler: ZPAQL source -> (stored header bytes, pcomp bytes)."""
    a9 = (C.c_int * 9)(*(list(args or []) + [0] * 9)[:9])
    return _two_bufs(lib().zpq_assemble, config.encode(), a9)


_TABLES = {"squash": (0, np.uint16, 4096), "stretch": (1, np.int16, 32768), "dt": (2, np.int32, 1024),
           "dt2k": (3, np.int32, 256), "state": (4, np.uint8, 1024)}


def table(name: str) -> np.ndarray:
    which, dt, n = _TABLES[name]
    out = np.empty(n, dt)
    got = lib().zpq_table(which, out.ctypes.data_as(C.c_void_p), out.nbytes)
    if got != out.nbytes:
        raise ZpaqError(7, f"table {name} unavailable")
    return out
