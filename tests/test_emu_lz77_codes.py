"""device/lz77_codes_kernel.h on the wavefront emulator (tests/emu/lz77_codes_emu_main.cpp): the lengths (one lane per item
slot, with the checks of the host's coder), the scan, and the two emitting kernels (one lane per token, one per input position)
must give, byte for byte, the stream host/preproc.cpp Lz77::emit_tokens writes for the same list -- zpq_lz77_serialize, which
the CPU suite's archives and test_lz77_hash_host.py pin to the reference.  Several ragged blocks go in one batch, empty ones
among them: a read across a block's end would see the next block's bytes.  No GPU."""
import ctypes as C
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import lz77_codes_cases as cc  # noqa: E402
import lz77_codes_emu  # noqa: E402
import lz77_hash_cases as hc  # noqa: E402

RB_METHOD = "x6,1,4,0,3,24"       # rb = 2: level 1 writes the two low offset bits as they are


def _batch(zlib_, xm, pairs):
    """pairs of (block as the parse saw it, token list): the emulator's streams against the host's coder."""
    a = zlib_.method_to_header(xm)[2]
    err, got = lz77_codes_emu.run(a, pairs)
    assert err == 0, (xm, err)
    for k, ((data, toks), g) in enumerate(zip(pairs, got)):
        want = hc.serialize(xm, data, toks)
        assert g == want, (xm, k, len(data), len(toks) // 16, len(g), len(want))


@pytest.fixture(scope="module")
def host_lists():
    """The host's parse of every input, once per method: (token list, block as the parse saw it)."""
    made = {}

    def get(xm):
        if xm not in made:
            made[xm] = [hc.host_tokens(xm, d) for d in hc.inputs()]
        return made[xm]
    return get


@pytest.mark.parametrize("order", ["", "reverse"])
@pytest.mark.parametrize("xm", hc.METHODS + (RB_METHOD,))
def test_device_codes_are_the_hosts(zlib_, host_lists, monkeypatch, xm, order):
    """Every kind at every length as one ragged batch: the empty blocks, lengths 1..12, and at 70 000 one 49 152-byte match
    (zeros), the flush after 4 096 literals (lcg), offsets past 2^15 (text)."""
    if order:
        monkeypatch.setenv("ZPQ_EMU_ORDER", order)
    else:
        monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    host = host_lists(xm)
    assert sum(len(h[1]) == 70000 for h in host) == len(hc.KINDS) and any(len(h[1]) == 0 for h in host)
    _batch(zlib_, xm, [(seen, toks) for toks, seen in host])


@pytest.mark.parametrize("xm", hc.FAR_METHODS)
def test_far_offsets(zlib_, monkeypatch, xm):
    """Offsets of 2^16 and more: level 2 codes them in three bytes instead of two."""
    monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    toks, seen = hc.host_tokens(xm, hc.far_repeat())
    assert any(off >= 1 << 16 for off in memoryview(toks).cast("I")[1::4])
    _batch(zlib_, xm, [(seen, toks)])


@pytest.mark.parametrize("order", ["", "reverse"])
@pytest.mark.parametrize("xm", cc.METHODS)
def test_synthetic_lists(zlib_, monkeypatch, xm, order):
    if order:
        monkeypatch.setenv("ZPQ_EMU_ORDER", order)
    else:
        monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    cases = cc.synthetic()
    if xm == cc.METHODS[0]:           # the two level-1 blocks meant to end on and inside a byte do
        by_name = {name: (d, t) for name, d, t in cases}
        assert len(hc.serialize(xm, *by_name["ends on a byte"])) == 5 and len(hc.serialize(xm, *by_name["ends inside a byte"])) == 2
    _batch(zlib_, xm, [(d, t) for _, d, t in cases])


def test_seeded_random_rounds(zlib_, monkeypatch):
    monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    rng = random.Random(31)
    for r in range(20):
        _batch(zlib_, cc.METHODS[r % len(cc.METHODS)], cc.random_batch(rng))


@pytest.mark.parametrize("xm", cc.METHODS[:2])
@pytest.mark.parametrize("case", cc.refusals(), ids=[c[0] for c in cc.refusals()])
def test_a_refused_list_sets_the_error_word(zlib_, monkeypatch, xm, case):
    """Each list the host's coder refuses, between two valid blocks: the error word is set and nothing is emitted for the batch.
    The emulator runs with every array at its exact size, so a lane that indexed by an unchecked field would be seen."""
    monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    _, data, toks = case
    L = hc._lib()
    e, t = hc._buf(data), hc._buf(toks).view("uint32")
    out = (C.c_ubyte * 4096)()
    ol = C.c_size_t(0)
    rc = L.zpq_lz77_serialize(xm.encode(), e.ctypes.data_as(hc._u8p), len(data), t.ctypes.data_as(hc._u32p), len(toks) // 16, out, 4096, C.byref(ol))
    assert rc == 7, (case[0], rc)                                     # ZPQ_E_DEVICE: the host refuses it
    valid = cc.synthetic()[0]
    a = zlib_.method_to_header(xm)[2]
    err, got = lz77_codes_emu.run(a, [(valid[1], valid[2]), (data, toks), (valid[1], valid[2])])
    assert err & 1 and got is None, (case[0], err)


def test_the_batch_entry_exists_and_keeps_the_hosts_contract(zlib_):
    """zpq_lz77_serialize_device and zpq_last_device_coded_blocks through the ctypes mirror: without a device the call declines
    with ZPQ_E_UNSUPPORTED and a note; with one it returns the host's streams."""
    import zpaq_amd as z
    xm = cc.METHODS[1]
    cases = cc.synthetic()[:3]
    rc, got, sizes = z.lz77_serialize_device(xm, [d for _, d, _ in cases], [t for _, _, t in cases])
    assert isinstance(z.last_device_coded_blocks(), int)
    if rc == 0:
        assert got == [hc.serialize(xm, d, t) for _, d, t in cases]
    else:
        assert rc == 8 and b"device" in z.lib().zpq_last_error(), (rc, z.lib().zpq_last_error())
