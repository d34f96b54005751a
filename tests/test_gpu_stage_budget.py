"""The device budget of the engine's batch stages (device/engine_prep.cpp, device/engine_post.cpp): every stage sums what its
batch holds on the device -- inputs, outputs, the workspace its offsets carve, the slack behind them -- and declines the batch
when that exceeds the engine's budget.  For one fixed, tiny batch per stage this pins the sum to the byte: with a budget of
T - 1 the public entry declines with the stage's note (the post-processor hands its streams back), with T it delivers what the
stage's own tests expect."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import e8e9_cases as ec  # noqa: E402
import fragment_cases as fc  # noqa: E402
import lz77_codes_cases as cc  # noqa: E402
import lz77_decode_cases as dc  # noqa: E402
import lz77_hash_cases as hc  # noqa: E402
import pcomp_cases as pc  # noqa: E402
import sort_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

u8p, u32p = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint32)
GUARD, FILL = 64, 0xC3
UNSUPPORTED = 8

# stage -> (T, the note of the decline at T - 1).  THE PARENT'S ACCOUNTING: each T was found by bisecting the budget over the same
# batch on the build before the stages moved out of engine.cpp, never on the code under test.  They are sums of sizes -- integer
# arithmetic, so equality is exact -- and change only with a deliberate change of a stage's device layout.
BUDGETS = {
    "suffix arrays": (4904176, "suffix sort workspace exceeds the device budget"),
    "sort pre-process, LZ77": (6568976, "sort + parse workspace exceeds the device budget"),
    "sort pre-process, BWT": (4980680, "sort + parse workspace exceeds the device budget"),
    "hash pre-process": (4825856, "hash parse workspace exceeds the device budget"),
    "LZ77 codes": (1342016, "the coded streams exceed the device budget"),
    "LZ77 decode": (1992032, "the decoded blocks exceed the device budget"),
    "BWT decode": (1529628, "decoder workspace exceeds the device budget"),
    "E8E9 decode, kind 4": (1133196, "the filter's list exceeds the device budget"),
    "E8E9 decode, kind 5": (2367868, "the decoded blocks exceed the device budget"),
    "E8E9 decode, kind 7": (1524448, "decoder workspace exceeds the device budget"),
    "PCOMP": (1168576, "post-processor state exceeds the device budget"),
    "fragment": (1684060, "the files and the record lists exceed the device budget"),
}


# ---- the batches: 3 to 5 items, at most 256 KiB, an empty item and one whose length is no multiple of 4 among them ----
def _ragged(items):
    assert 3 <= len(items) <= 5 and sum(len(x) for x in items) <= 256 << 10
    assert any(len(x) == 0 for x in items) and any(len(x) % 4 for x in items)
    return tuple(items)


@functools.lru_cache(maxsize=None)
def blocks():
    """Five blocks of tests/lz77_hash_cases.py: text, nothing, 257 random bytes, records, 255 zeros."""
    def pick(n, kind):
        return hc.inputs()[hc.LENGTHS.index(n) * len(hc.KINDS) + hc.KINDS.index(kind)]
    return _ragged([pick(5000, "text"), pick(0, "lcg"), pick(257, "lcg"), pick(70000, "records"), pick(255, "zeros")])


@functools.lru_cache(maxsize=None)
def e8_blocks():
    """Four blocks of tests/e8e9_cases.py: nothing, a hit across the first tile's edge, 333 bytes of opcodes, x86-like bytes."""
    bl = ec.blocks()
    return _ragged([bl[0], next(b for b in bl if len(b) == ec.TILE + 1), next(b for b in bl if len(b) == 333), bl[-1]])


def _arr(d: bytes) -> np.ndarray:
    return np.frombuffer(bytes(d), np.uint8).copy() if len(d) else np.zeros(1, np.uint8)


def _note(gpu) -> str:
    return gpu.lib().zpq_last_error().decode()


# ---- the stages: each runs its batch once and returns (delivered, note), having checked what either outcome promises ----
def suffix_arrays(gpu):
    L = gpu.lib()
    L.zpq_suffix_arrays_device.argtypes = [C.POINTER(u8p), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(u32p)]
    bl = blocks()
    n = len(bl)
    bufs = [_arr(d) for d in bl]
    outs = [np.full(len(d) + 1, 0xA5A5A5A5, np.uint32) for d in bl]
    IA = (u8p * n)(*[b.ctypes.data_as(u8p) for b in bufs])
    LN = (C.c_uint32 * n)(*[len(d) for d in bl])
    OA = (u32p * n)(*[o.ctypes.data_as(u32p) for o in outs])
    rc = L.zpq_suffix_arrays_device(IA, LN, n, OA)
    if rc != 0:
        assert rc == UNSUPPORTED and all((o == 0xA5A5A5A5).all() for o in outs)
        return False, _note(gpu)
    for d, o in zip(bl, outs):
        assert (o[:len(d)] == sc.expected(d)).all() and o[len(d)] == 0xA5A5A5A5, len(d)
    return True, ""


def _preprocess(gpu, xm):
    L = gpu.lib()
    L.zpq_preprocess_blocks_device.argtypes = [C.c_char_p, C.POINTER(u8p), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(u8p), C.POINTER(C.c_size_t),
                                               C.POINTER(C.c_size_t)]
    bl = blocks()
    n = len(bl)
    dev_in = [np.concatenate([np.frombuffer(d, np.uint8), np.zeros(8, np.uint8)]) for d in bl]
    outs = [np.empty(len(d) + len(d) // 2 + 4096, np.uint8) for d in bl]
    IA = (u8p * n)(*[b.ctypes.data_as(u8p) for b in dev_in])
    LN = (C.c_uint32 * n)(*[len(d) for d in bl])
    OA = (u8p * n)(*[o.ctypes.data_as(u8p) for o in outs])
    CP = (C.c_size_t * n)(*[o.size for o in outs])
    OL = (C.c_size_t * n)()
    rc = L.zpq_preprocess_blocks_device(xm.encode(), IA, LN, n, OA, CP, OL)
    if rc != 0:
        assert rc == UNSUPPORTED
        return False, _note(gpu)
    for k, d in enumerate(bl):
        assert outs[k][:OL[k]].tobytes() == hc.preprocess(xm, d)[0], (xm, k)
    return True, ""


def _serialize(gpu, xm):
    pairs = [hc.host_tokens(xm, d)[::-1] for d in blocks()]
    want = [hc.serialize(xm, d, t) for d, t in pairs]
    rc, streams, sizes = gpu.lz77_serialize_device(xm, [d for d, _ in pairs], [t for _, t in pairs], [len(w) for w in want])
    if rc != 0:
        assert rc == UNSUPPORTED and sizes == [0] * len(want)
        return False, _note(gpu)
    assert streams == want
    return True, ""


def _decode(gpu, entry, xm, bl):
    """One of the three stream decoders over the streams the host's pre-processor makes of `bl`: they decode to the blocks."""
    streams, wants = [hc.preprocess(xm, d)[0] for d in bl], list(bl)
    rc, bufs, sizes, status = entry(xm, streams, [len(w) for w in wants], guard=GUARD, fill=FILL)
    if rc != 0:
        assert rc == UNSUPPORTED and sizes == [0] * len(bl) and status == [1] * len(bl)
        assert all(b == bytes([FILL]) * len(b) for b in bufs), "a declined batch wrote something"
        return False, _note(gpu)
    assert status == [0] * len(bl) and sizes == [len(w) for w in wants]
    for k, (b, w) in enumerate(zip(bufs, wants)):
        assert b == w + bytes([FILL]) * GUARD, (xm, k)
    return True, ""


def pcomp(gpu):
    p = pc.by_name("reverse")
    streams = _ragged(pc.batch(4))
    wants = [pc.expected(p, s)[1] for s in streams]
    rc, bufs, sizes, status = gpu.pcomp_device(pc.code(p), p.ph, p.pm, streams, [len(w) for w in wants], guard=GUARD, fill=FILL)
    assert rc == 0, _note(gpu)
    if status != [0] * len(streams):                  # handed back: the caller runs the batch on the host
        assert status == [1] * len(streams) and sizes == [0] * len(streams)
        assert all(b == bytes([FILL]) * len(b) for b in bufs), "a batch that was handed back wrote something"
        return False, _note(gpu)
    assert sizes == [len(w) for w in wants]
    assert all(b == w + bytes([FILL]) * GUARD for b, w in zip(bufs, wants))
    return True, ""


@functools.lru_cache(maxsize=None)
def fragment_files():
    f = dict(fc.files0())
    return _ragged([f["pattern0"], f["pattern63"], f["zeros"], f["text"], f["cutting50"]])


def fragment(gpu):
    files = list(fragment_files())
    rc, want, total = gpu.fragment_host(files, 0, fc.BLOCKSIZE)
    assert rc == 0
    rc, got, said = gpu.fragment_device(files, 0, fc.BLOCKSIZE, cap=total)
    if rc != 0:
        assert rc == UNSUPPORTED and got is True and said == 0          # (got: the output arrays were left untouched)
        return False, _note(gpu)
    assert said == total and got == want
    return True, ""


STAGES = {
    "suffix arrays": suffix_arrays,
    "sort pre-process, LZ77": lambda gpu: _preprocess(gpu, "x0,1,4,0,3,21,1"),
    "sort pre-process, BWT": lambda gpu: _preprocess(gpu, "x0,3ci1"),
    "hash pre-process": lambda gpu: _preprocess(gpu, "x0,1,4,0,3,20"),
    "LZ77 codes": lambda gpu: _serialize(gpu, cc.METHODS[0]),
    "LZ77 decode": lambda gpu: _decode(gpu, gpu.lz77_decode_device, dc.L1, blocks()),
    "BWT decode": lambda gpu: _decode(gpu, gpu.bwt_decode_device, "x0,3", blocks()),
    "E8E9 decode, kind 4": lambda gpu: _decode(gpu, gpu.e8e9_decode_device, "x0,4", e8_blocks()),
    "E8E9 decode, kind 5": lambda gpu: _decode(gpu, gpu.e8e9_decode_device, "x0,5,6,0,3,20", e8_blocks()),
    "E8E9 decode, kind 7": lambda gpu: _decode(gpu, gpu.e8e9_decode_device, "x0,7", e8_blocks()),
    "PCOMP": pcomp,
    "fragment": fragment,
}


@pytest.fixture
def budget(gpu, monkeypatch):
    """set_state_budget, undone afterwards; the knobs that change a stage's layout at their defaults."""
    monkeypatch.delenv("ZPAQ_AMD_DEVICE_CODES", raising=False)
    monkeypatch.delenv("ZPAQ_AMD_FRAG_PIECE", raising=False)
    try:
        yield gpu.set_state_budget
    finally:
        gpu.set_state_budget(0)


@pytest.mark.parametrize("stage", list(STAGES))
def test_the_budget_at_which_a_stage_declines(gpu, budget, stage):
    t, note = BUDGETS[stage]
    budget(t - 1)
    delivered, said = STAGES[stage](gpu)
    assert not delivered and note in said, (stage, t - 1, said)
    budget(t)
    delivered, said = STAGES[stage](gpu)
    assert delivered, (stage, t, said)
