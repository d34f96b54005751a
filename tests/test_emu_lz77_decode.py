"""device/lz77_decode_kernel.h on the wavefront emulator (tests/emu/lz77_decode_emu_main.cpp): the parse (one wavefront per
stream, 16 bytes per code) and the copy (groups of tokens whose sources are final, lane = output byte) must give, byte for byte,
what the method's own PCOMP program makes of the stream on the host (zpq_postprocess_block) -- or decline the stream, which no
stream of this library's coder may be.  Several ragged streams go in one batch, every array at its exact size between
inaccessible pages.  No GPU."""
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import lz77_codes_cases as cc  # noqa: E402
import lz77_decode_cases as dc  # noqa: E402
import lz77_decode_emu  # noqa: E402
import lz77_hash_cases as hc  # noqa: E402


def _order(monkeypatch, order):
    if order:
        monkeypatch.setenv("ZPQ_EMU_ORDER", order)
    else:
        monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)


def _host(z, xm, stream):
    rc, out, _ = z.postprocess_block(xm, stream)
    return rc, out


def _decode_all(z, xm, streams, wants):
    """Valid streams: everything is decoded, nothing declined."""
    overflow, res = lz77_decode_emu.run(dc.args_of(xm), streams)
    assert not overflow
    for k, ((status, out_len, ntok, out), want) in enumerate(zip(res, wants)):
        assert status == 0, (xm, k, len(streams[k]), status)
        assert ntok <= len(streams[k])
        assert out == want, (xm, k, len(streams[k]), out_len, len(want))


def _exact_or_declined(z, xm, streams):
    """Any streams: each is what the host makes of it, or declined.  Returns the statuses."""
    overflow, res = lz77_decode_emu.run(dc.args_of(xm), streams)
    assert not overflow
    for k, (status, out_len, ntok, out) in enumerate(res):
        if status == 0:
            rc, want = _host(z, xm, streams[k])
            assert rc == 0 and out == want, (xm, k, streams[k][:16].hex(), len(streams[k]), out_len, rc, len(want))
        else:
            assert out is None
    return [r[0] for r in res]


@pytest.fixture(scope="module")
def host_streams():
    """The host's stream of every input, once per method: (stream, block as the parse saw it)."""
    made = {}

    def get(xm):
        if xm not in made:
            made[xm] = [hc.preprocess(xm, d) for d in hc.inputs()]
        return made[xm]
    return get


@pytest.mark.parametrize("order", ["", "reverse"])
@pytest.mark.parametrize("xm", dc.METHODS)
def test_round_trip_of_every_input(zlib_, host_streams, monkeypatch, xm, order):
    """Every kind at every length as one ragged batch: the empty blocks, the 49 152-byte match of zeros (off = 1; at level 2 a
    chain of pieces), pattern (off < len), the flush after 4 096 literals (lcg), rb = 2."""
    _order(monkeypatch, order)
    host = host_streams(xm)
    assert sum(len(h[1]) == 70000 for h in host) == len(hc.KINDS) and any(len(h[1]) == 0 for h in host)
    _decode_all(zlib_, xm, [s for s, _ in host], [seen for _, seen in host])


@pytest.mark.parametrize("xm", hc.FAR_METHODS)
def test_far_offsets(zlib_, monkeypatch, xm):
    _order(monkeypatch, "")
    stream, seen = hc.preprocess(xm, hc.far_repeat())
    toks, _ = hc.host_tokens(xm, hc.far_repeat())
    assert any(off >= 1 << 16 for off in memoryview(toks).cast("I")[1::4])
    _decode_all(zlib_, xm, [stream], [seen])


@pytest.mark.parametrize("order", ["", "reverse"])
@pytest.mark.parametrize("xm", cc.METHODS)
def test_synthetic_lists_through_the_coder_and_back(zlib_, monkeypatch, xm, order):
    """The coder's hand-made lists (gaps around the flush, lengths around level 2's splits, offsets around its widths, streams
    that end on and inside a byte).  A list's matches need not match, so the block that comes back is what the host's program
    makes of the stream -- which, for a list that is a parse, is the block."""
    _order(monkeypatch, order)
    streams = [hc.serialize(xm, d, t) for _, d, t in cc.synthetic()]
    wants = []
    for s in streams:
        rc, want = _host(zlib_, xm, s)
        assert rc == 0
        wants.append(want)
    assert all(len(w) == len(d) for w, (_, d, _) in zip(wants, cc.synthetic()))
    _decode_all(zlib_, xm, streams, wants)


def test_seeded_random_rounds(zlib_, monkeypatch):
    """Random lists through the host's coder and back.  The coder does not ask whether a list is a parse: a match shorter than
    the minimum (4 here) is written as some other code, and what such a stream holds is anybody's guess -- it is the host's
    output or declined.  A list without one is a stream the coder writes for a parse's list: never declined."""
    _order(monkeypatch, "")
    rng = random.Random(47)
    faithful = 0
    for r in range(20):
        xm = cc.METHODS[r % len(cc.METHODS)]
        batch = cc.random_batch(rng)
        streams = [hc.serialize(xm, d, t) for d, t in batch]
        status = _exact_or_declined(zlib_, xm, streams)
        for (d, t), s in zip(batch, status):
            if all(length >= cc.MM for length in memoryview(t).cast("I")[2::4]):
                assert s == 0, (xm, r, len(d))
                faithful += 1
    assert faithful >= 20


@pytest.mark.parametrize("order", ["", "reverse"])
def test_handmade_streams_around_the_group_rule(zlib_, monkeypatch, order):
    _order(monkeypatch, order)
    for xm in cc.METHODS:
        cases = [c for c in dc.handmade() if c[1] == xm]
        status = _exact_or_declined(zlib_, xm, [c[2] for c in cases])
        for (name, _, _, declined), s in zip(cases, status):
            assert (s != 0) == declined, (xm, name, s)


@pytest.mark.parametrize("xm", cc.METHODS)
def test_damaged_streams_are_the_hosts_or_declined(zlib_, monkeypatch, xm):
    """Each stream of a small valid batch cut at every length, a first code that is a match, non-zero pad bits: what the host
    makes of it, or declined -- and the valid streams on either side come out as ever."""
    _order(monkeypatch, "")
    streams, ncut = dc.damaged_batch(xm)
    status = _exact_or_declined(zlib_, xm, streams)
    assert status[0] == 0 and status[-1] == 0
    # a cut changes how a stream ends, never whether the device takes it
    assert sum(1 for s in status if s) <= len(streams) - 2 - ncut


def test_a_capacity_one_byte_short(zlib_, monkeypatch):
    """The host's step between the kernels: sizes first, and nothing is emitted when one does not fit."""
    _order(monkeypatch, "")
    xm = cc.METHODS[0]
    pairs = [hc.preprocess(xm, d) for d in hc.inputs()[20:26]]
    streams = [s for s, _ in pairs]
    sizes = [len(seen) for _, seen in pairs]
    overflow, res = lz77_decode_emu.run(dc.args_of(xm), streams, caps=sizes)
    assert not overflow and [r[3] for r in res] == [seen for _, seen in pairs]
    caps = list(sizes)
    k = max(range(len(sizes)), key=lambda i: sizes[i])
    caps[k] -= 1
    overflow, res = lz77_decode_emu.run(dc.args_of(xm), streams, caps=caps)
    assert overflow and [r[1] for r in res] == sizes and all(r[3] is None for r in res)


@pytest.mark.parametrize("xm", hc.METHODS + ("x6,1,4,0,3,24", "x0,3", "x0,0", "x0,4"))
def test_postprocess_inverts_preprocess(zlib_, xm):
    """zpq_postprocess_block(zpq_preprocess_block(x)) == x: the new host entry against the existing pre-processor (E8E9, BWT and
    a method without a program among them)."""
    inputs = hc.inputs() if xm != "x6,1,4,0,3,24" else hc.inputs()[::6]
    for d in inputs:
        stream, _ = hc.preprocess(xm, d)
        rc, out = _host(zlib_, xm, stream)
        assert rc == 0 and out == d, (xm, len(d), rc)


def test_the_entries_exist_and_decline_without_a_device(zlib_):
    import zpaq_amd as z
    xm = cc.METHODS[1]
    pairs = [hc.preprocess(xm, d) for d in hc.inputs()[20:24]]
    assert isinstance(z.last_device_unlz_segments(), int)
    rc, bufs, sizes, status = z.lz77_decode_device(xm, [s for s, _ in pairs], [len(d) for _, d in pairs])
    if rc == 0:
        assert status == [0] * len(pairs) and bufs == [d for _, d in pairs]
    else:
        assert rc == 8 and b"device" in z.lib().zpq_last_error(), (rc, z.lib().zpq_last_error())
    # another kind of method is unsupported, with or without a device
    for other in (dc.E8E9, "x0,3", "x0,0"):
        rc, _, _, _ = z.lz77_decode_device(other, [b"\x00\x01"], [16])
        assert rc == 8 and b"unavailable" in z.lib().zpq_last_error(), (other, rc)
