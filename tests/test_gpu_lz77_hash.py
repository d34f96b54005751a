"""The LZ77 parse through LZBuffer's hash table on the device (device/lz77_hash_kernel.h; reference: LZBuffer::fill without a
suffix array, libzpaq.cpp:6702-6782): method 1, method 2 below type 64 and every x method with args[5] - args[0] < 21.  The
streams of a whole batch against the host's pre-processor, the archives of zpq_compress_blocks against the reference, and the
batches the device declines."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lz77_hash_cases as hc  # noqa: E402

from zpaq_amd import corpus  # noqa: E402

pytestmark = pytest.mark.gpu

u8p = C.POINTER(C.c_ubyte)


def _entries(gpu):
    L = gpu.lib()
    L.zpq_preprocess_blocks_device.argtypes = [C.c_char_p, C.POINTER(u8p), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(u8p), C.POINTER(C.c_size_t),
                                               C.POINTER(C.c_size_t)]
    L.zpq_last_hash_parse_blocks.restype = C.c_uint32
    return L


def _device_streams(L, xm, src):
    """zpq_preprocess_blocks_device over one batch: (return code, streams, the caller's buffers afterwards)."""
    n = len(src)
    dev_in = [np.concatenate([np.frombuffer(b, np.uint8), np.zeros(8, np.uint8)]) for b in src]        # (copies: E8E9 works in place)
    outs = [np.empty(len(b) + len(b) // 2 + 4096, np.uint8) for b in src]
    IA = (u8p * n)(*[b.ctypes.data_as(u8p) for b in dev_in])
    LN = (C.c_uint32 * n)(*[len(b) for b in src])
    OA = (u8p * n)(*[o.ctypes.data_as(u8p) for o in outs])
    CP = (C.c_size_t * n)(*[o.size for o in outs])
    OL = (C.c_size_t * n)()
    rc = L.zpq_preprocess_blocks_device(xm.encode(), IA, LN, n, OA, CP, OL)
    return rc, [outs[k][:OL[k]].tobytes() for k in range(n)], [dev_in[k][:len(src[k])].tobytes() for k in range(n)]


@pytest.fixture(scope="module")
def batch():
    """Every kind at the 13 lengths of the host test, and one 1 MiB text block (more than one workgroup per block, index and
    key arrays of a realistic size)."""
    return list(hc.inputs()) + [corpus.block("text", 1 << 20, 4321).tobytes()]


@pytest.mark.parametrize("xm", hc.METHODS)
def test_streams_of_a_batch_are_the_hosts(gpu, batch, xm):
    L = _entries(gpu)
    rc, got, after = _device_streams(L, xm, batch)
    assert rc == 0, (xm, L.zpq_last_error().decode())
    for k, d in enumerate(batch):
        want, filtered = hc.preprocess(xm, d)
        assert got[k] == want, (xm, k, len(d), len(got[k]), len(want))
        assert after[k] == filtered, (xm, k, len(d), "the caller's buffer after E8E9")


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


# method -> (blocks parsed on the device with the knob on; None: the method picks per block, not asserted), slot 7 of zpq_last_api_timing
# (blocks whose suffix array came from the device: none of these methods sorts, except "2" for blocks of type 64 and more --
# tests/test_gpu_parity.py pins its 12 for these blocks)
COMPRESS = {"1": (12, 0), "2": (None, 12), "x0,1,4,0,3,20": (12, 0), "x0,5,4,0,2,16": (12, 0), "x0,2,4,0,3,20c0,0,511": (12, 0)}


@pytest.mark.parametrize("method", list(COMPRESS))
def test_archives_are_the_references(gpu, ref_archives, blocks, monkeypatch, method):
    L = _entries(gpu)
    ph = (C.c_double * 8)()
    want = ref_archives(method)
    parsed, sorted_ = COMPRESS[method]
    for knob in ("1", "0"):
        monkeypatch.setenv("ZPAQ_AMD_DEVICE_PARSE", knob)
        arch = gpu.compress_blocks([b.copy() for b in blocks], method)
        L.zpq_last_api_timing(ph)
        assert int(ph[7]) == sorted_, (knob, method, ph[7])
        if knob == "0":
            assert L.zpq_last_hash_parse_blocks() == 0, (method, L.zpq_last_hash_parse_blocks())
        elif parsed is not None:
            assert L.zpq_last_hash_parse_blocks() == parsed, (method, L.zpq_last_hash_parse_blocks())
        for k, (a, w) in enumerate(zip(arch, want)):
            assert a == w, (knob, method, k, blocks[k].size)
        assert gpu.decompress(b"".join(arch)) == b"".join(b.tobytes() for b in blocks), (knob, method)


@pytest.mark.parametrize("method", ["x5,1,4,0,3,25", "x0,2,1,0,3,20c0,0,511"])
def test_a_batch_outside_the_range_stays_on_the_host(gpu, ref_archives, blocks, monkeypatch, method):
    """A table of 2^25 slots; min_match 1 at level 2 (the reference then compares the byte in front of a candidate, which for
    position 0 lies outside the block): same archives, nothing counted, no error."""
    L = _entries(gpu)
    monkeypatch.setenv("ZPAQ_AMD_DEVICE_PARSE", "1")
    arch = gpu.compress_blocks([b.copy() for b in blocks], method)
    assert L.zpq_last_hash_parse_blocks() == 0
    assert arch == ref_archives(method), method


def test_the_batch_entry_declines_and_hands_the_buffers_back(gpu):
    """zpq_preprocess_blocks_device outside the range: an error, and buffers E8E9 had filtered go back as they came."""
    L = _entries(gpu)
    src = []
    for i in range(4):
        a = corpus.block("lcg", 3000, 900 + i).copy()
        a[10::9] = 0xE8
        a[14::9] = 0
        src.append(a.tobytes())
    rc, _, after = _device_streams(L, "x5,5,4,0,3,25", src)
    assert rc != 0
    assert after == src
    assert hc.preprocess("x5,5,4,0,3,25", src[0])[1] != src[0]            # (the filter does change these bytes)
