"""LZBuffer's codes written on the device (device/lz77_codes_kernel.h; reference: LZBuffer's literals() / match(),
libzpaq.cpp:6759-6883): the streams of zpq_lz77_serialize_device against the host's coder, the archives of zpq_compress_blocks
against the reference with ZPAQ_AMD_DEVICE_CODES on and off, and zpq_preprocess_blocks_device with the knob on."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lz77_codes_cases as cc  # noqa: E402
import lz77_hash_cases as hc  # noqa: E402

from zpaq_amd import corpus  # noqa: E402

pytestmark = pytest.mark.gpu

u8p = C.POINTER(C.c_ubyte)
u32p = C.POINTER(C.c_uint32)
GUARD = 64


def _entries(gpu):
    L = gpu.lib()
    L.zpq_lz77_serialize_device.argtypes = [C.c_char_p, C.POINTER(u8p), C.POINTER(C.c_uint32), C.POINTER(u32p), C.POINTER(C.c_size_t), C.c_uint32,
                                            C.POINTER(u8p), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.zpq_preprocess_blocks_device.argtypes = [C.c_char_p, C.POINTER(u8p), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(u8p), C.POINTER(C.c_size_t),
                                               C.POINTER(C.c_size_t)]
    L.zpq_last_device_coded_blocks.restype = C.c_uint32
    L.zpq_last_hash_parse_blocks.restype = C.c_uint32
    return L


def _serialize_device(L, xm, pairs, caps):
    """zpq_lz77_serialize_device over (block, token list) pairs with these capacities and GUARD bytes of 0xC3 behind each
    buffer: (return code, sizes, buffers with their guards)."""
    n = len(pairs)
    ins = [hc._buf(d) for d, _ in pairs]
    tks = [np.frombuffer(bytearray(t), np.uint32).copy() if t else np.zeros(4, np.uint32) for _, t in pairs]
    outs = [np.full(c + GUARD, 0xC3, np.uint8) for c in caps]
    IA = (u8p * n)(*[a.ctypes.data_as(u8p) for a in ins])
    LN = (C.c_uint32 * n)(*[len(d) for d, _ in pairs])
    TA = (u32p * n)(*[t.ctypes.data_as(u32p) for t in tks])
    TN = (C.c_size_t * n)(*[len(t) // 16 for _, t in pairs])
    OA = (u8p * n)(*[o.ctypes.data_as(u8p) for o in outs])
    CP = (C.c_size_t * n)(*caps)
    OL = (C.c_size_t * n)()
    rc = L.zpq_lz77_serialize_device(xm.encode(), IA, LN, TA, TN, n, OA, CP, OL)
    return rc, [int(x) for x in OL], outs


@pytest.fixture(scope="module")
def batch():
    """Every kind at the 13 lengths of the host test, and one 1 MiB text block (more than one workgroup per block)."""
    return list(hc.inputs()) + [corpus.block("text", 1 << 20, 4321).tobytes()]


@pytest.fixture(scope="module")
def host_streams(batch):
    """Per method, once: (block as the parse saw it, the host's token list) pairs and the host's streams."""
    made = {}

    def get(xm):
        if xm not in made:
            pairs = [hc.host_tokens(xm, d)[::-1] for d in batch]
            made[xm] = (pairs, [hc.serialize(xm, d, t) for d, t in pairs])
        return made[xm]
    return get


@pytest.mark.parametrize("xm", cc.METHODS)
def test_streams_of_the_hosts_lists(gpu, host_streams, xm):
    L = _entries(gpu)
    pairs, want = host_streams(xm)
    caps = [len(w) for w in want]                                     # exact: a byte more than the stream would hit the guard
    rc, sizes, outs = _serialize_device(L, xm, pairs, caps)
    assert rc == 0, (xm, L.zpq_last_error().decode())
    assert sizes == caps
    for k, (o, w) in enumerate(zip(outs, want)):
        assert o[:len(w)].tobytes() == w, (xm, k, len(pairs[k][0]))
        assert (o[len(w):] == 0xC3).all(), (xm, k, "a store past the capacity")


@pytest.mark.parametrize("xm", cc.METHODS)
def test_a_buffer_too_small_reports_every_size(gpu, host_streams, xm):
    L = _entries(gpu)
    pairs, want = host_streams(xm)
    caps = [len(w) for w in want]
    short = max(range(len(want)), key=lambda k: len(want[k]))
    caps[short] -= 1
    rc, sizes, outs = _serialize_device(L, xm, pairs, caps)
    assert rc == 3, (xm, rc)                                          # ZPQ_E_OVERFLOW
    assert sizes == [len(w) for w in want]
    for k, o in enumerate(outs):
        assert (o[caps[k]:] == 0xC3).all(), (xm, k, "a store past the capacity")


@pytest.mark.parametrize("xm", cc.METHODS)
def test_synthetic_lists_as_one_batch(gpu, xm):
    L = _entries(gpu)
    pairs = [(d, t) for _, d, t in cc.synthetic()]
    want = [hc.serialize(xm, d, t) for d, t in pairs]
    rc, sizes, outs = _serialize_device(L, xm, pairs, [len(w) for w in want])
    assert rc == 0, (xm, L.zpq_last_error().decode())
    for k, (o, w) in enumerate(zip(outs, want)):
        assert sizes[k] == len(w) and o[:len(w)].tobytes() == w, (xm, cc.synthetic()[k][0])
        assert (o[len(w):] == 0xC3).all(), (xm, cc.synthetic()[k][0], "a store past the capacity")


@pytest.mark.parametrize("xm", cc.METHODS[:2])
def test_a_refused_list_returns_the_hosts_error(gpu, xm):
    L = _entries(gpu)
    valid = cc.synthetic()[0][1:]
    for name, data, toks in cc.refusals():
        e, t = hc._buf(data), hc._buf(toks).view("uint32")
        ol = C.c_size_t(0)
        host_rc = L.zpq_lz77_serialize(xm.encode(), e.ctypes.data_as(u8p), len(data), t.ctypes.data_as(u32p), len(toks) // 16, (C.c_ubyte * 4096)(), 4096,
                                       C.byref(ol))
        assert host_rc == 7, (name, host_rc)                          # ZPQ_E_DEVICE
        rc, _, outs = _serialize_device(L, xm, [valid, (data, toks), valid], [65536, 4096, 65536])
        assert rc == host_rc, (xm, name, rc, L.zpq_last_error().decode())
        assert all((o == 0xC3).all() for o in outs), (xm, name, "a refused batch wrote something")


@pytest.fixture(scope="module")
def blocks():
    kinds = ["text", "lcg", "zeros", "records"]
    return [corpus.block(kinds[i % 4], 150000 + 1111 * i, 500 + i) for i in range(12)]


@pytest.fixture(scope="module")
def ref_archives(ref, blocks):
    """The reference's archives, made once per method."""
    made = {}

    def get(method):
        if method not in made:
            made[method] = [ref.compress_block(d.copy(), method) for d in blocks]
        return made[method]
    return get


def _lz_blocks(gpu, blocks, method):
    """Blocks whose expanded method pre-processes with an LZ77 (kind 1 or 2, with or without E8E9)."""
    n = 0
    for b in blocks:
        kind = gpu.method_to_header(gpu.expand_method(method, b))[2][1]
        n += kind in (1, 2, 5, 6)
    return n


# method -> blocks coded on the device with the knob on (None: the method picks per block -- counted from its expansion)
COMPRESS = {"1": 12, "2": None, "x0,2,4,0,3,20c0,0,511": 12, "x0,2,12,0,7,21,1c0,0,511": 12}


@pytest.mark.parametrize("method", list(COMPRESS))
def test_archives_are_the_references(gpu, ref_archives, blocks, monkeypatch, method):
    L = _entries(gpu)
    want = ref_archives(method)
    monkeypatch.setenv("ZPAQ_AMD_DEVICE_PARSE", "1")
    coded = COMPRESS[method] if COMPRESS[method] is not None else _lz_blocks(gpu, blocks, method)
    for knob in ("1", "0"):
        monkeypatch.setenv("ZPAQ_AMD_DEVICE_CODES", knob)
        arch = gpu.compress_blocks([b.copy() for b in blocks], method)
        assert L.zpq_last_device_coded_blocks() == (coded if knob == "1" else 0), (knob, method, L.zpq_last_device_coded_blocks())
        for k, (a, w) in enumerate(zip(arch, want)):
            assert a == w, (knob, method, k, blocks[k].size)
        assert gpu.decompress(b"".join(arch)) == b"".join(b.tobytes() for b in blocks), (knob, method)


def test_without_the_knob_the_engine_decides_per_batch(gpu, ref, monkeypatch):
    """The variable unset: a batch of text is coded on the device (its list is larger than its stream), an incompressible one is
    not (no matches: the list is empty, the stream is the input) -- DESIGN 4.5.2 has the measurement behind the rule.  Same
    archives as the reference either way."""
    L = _entries(gpu)
    monkeypatch.setenv("ZPAQ_AMD_DEVICE_PARSE", "1")
    monkeypatch.delenv("ZPAQ_AMD_DEVICE_CODES", raising=False)
    for kind, coded in (("text", 4), ("lcg", 0)):
        blks = [corpus.block(kind, 300000 + 77 * i, 800 + i) for i in range(4)]
        arch = gpu.compress_blocks([b.copy() for b in blks], "1")
        assert L.zpq_last_hash_parse_blocks() == 4 and L.zpq_last_device_coded_blocks() == coded, (kind, L.zpq_last_device_coded_blocks())
        assert arch == [ref.compress_block(b.copy(), "1") for b in blks], kind


def test_the_batch_pre_processor_with_the_codes_on_the_device(gpu, batch, monkeypatch):
    """zpq_preprocess_blocks_device with E8E9 in front: the host's streams, and the caller's buffers come back filtered."""
    L = _entries(gpu)
    xm = hc.METHODS[3]
    monkeypatch.setenv("ZPAQ_AMD_DEVICE_CODES", "1")
    n = len(batch)
    dev_in = [np.concatenate([np.frombuffer(b, np.uint8), np.zeros(8, np.uint8)]) for b in batch]        # (copies: E8E9 works in place)
    outs = [np.empty(len(b) + len(b) // 2 + 4096, np.uint8) for b in batch]
    IA = (u8p * n)(*[b.ctypes.data_as(u8p) for b in dev_in])
    LN = (C.c_uint32 * n)(*[len(b) for b in batch])
    OA = (u8p * n)(*[o.ctypes.data_as(u8p) for o in outs])
    CP = (C.c_size_t * n)(*[o.size for o in outs])
    OL = (C.c_size_t * n)()
    rc = L.zpq_preprocess_blocks_device(xm.encode(), IA, LN, n, OA, CP, OL)
    assert rc == 0, L.zpq_last_error().decode()
    for k, d in enumerate(batch):
        want, filtered = hc.preprocess(xm, d)
        assert outs[k][:OL[k]].tobytes() == want, (k, len(d), OL[k], len(want))
        assert dev_in[k][:len(d)].tobytes() == filtered, (k, len(d), "the caller's buffer after E8E9")
