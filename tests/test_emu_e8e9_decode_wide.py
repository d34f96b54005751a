"""device/lz77_decode_wide_kernel.h with device/e8e9_kernel.h behind it on the wavefront emulator
(tests/emu/lz77_decode_wide_e8_emu_main.cpp): the streams of the E8E9 forms of the LZ77 methods parsed in pieces, copied by pointer
jumping over the packed outputs, emitted into rooms on multiples of 16 bytes (unlzw_emit_placed_body) and filtered there must give,
byte for byte, what the method's own PCOMP program makes of the stream on the host (zpq_postprocess_block) -- or decline the
stream.  Ragged batches, every array at its exact size between inaccessible pages and dirty at the start, the lanes in order and
reversed, at pieces of 64, 256 and 4 096 stream bytes.  No GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import e8e9_cases as ec  # noqa: E402
import e8e9_wide_cases as e8w  # noqa: E402
import lz77_codes_cases as cc  # noqa: E402
import lz77_decode_cases as dc  # noqa: E402
import lz77_decode_wide_cases as wc  # noqa: E402
import lz77_decode_wide_e8_emu as emu  # noqa: E402
import lz77_decode_wide_emu  # noqa: E402
import lz77_hash_cases as hc  # noqa: E402

PIECES = (64, 256, 4096)


def _order(monkeypatch, order):
    if order:
        monkeypatch.setenv("ZPQ_EMU_ORDER", order)
    else:
        monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)


def test_the_host_gives_back_every_block(zlib_):
    """The expectation of every test below and of the GPU tests is what zpq_postprocess_block makes of the stream; here it is held
    against the input, method by method."""
    bl = e8w.blocks()
    assert bl[:len(ec.blocks())] == ec.blocks()
    assert [len(b) for b in bl[len(ec.blocks()):]] == [17, 31, 33, 70001, 70001, 300000]
    for b in bl[len(ec.blocks()):len(ec.blocks()) + 3]:
        assert b[:5] == bytes([0xe8, 0x10, 0x20, 0x30, 0x00]) and b[-5:] == bytes([0xe9, 0xff, 0xff, 0xff, 0xff])
    assert sum(len(b) % 16 != 0 for b in bl) > len(bl) // 2                # packed and aligned offsets differ
    for xm in e8w.METHODS:
        assert e8w.expected(xm) == bl, xm


@pytest.mark.parametrize("order", ["", "reverse"])
@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("xm", e8w.METHODS)
def test_the_whole_ragged_batch(zlib_, monkeypatch, xm, piece, order):
    """Every output is the expectation (the padding behind a block is never looked at); the byte in front of the first room and
    the page behind the last are untouched (the driver checks: "edges ok")."""
    _order(monkeypatch, order)
    streams, wants = e8w.streams(xm), e8w.expected(xm)
    res, pieces, rounds, launches = emu.run(dc.args_of(xm), streams, piece)
    for k, ((status, out_len, out, listed), want) in enumerate(zip(res, wants)):
        assert status == 0, (xm, piece, k, len(want), "declined")
        assert out == want, (xm, piece, k, len(want), out_len)
        assert listed == (len(want) > 0), (xm, piece, k)
    assert pieces[0] == sum((len(s) + piece - 1) // piece for s in streams) and sum(pieces[1:]) <= pieces[0]
    assert 1 <= rounds <= 32 and launches >= rounds + 3


def _exact_or_declined(z, xm8, streams, piece):
    """Any streams under an E8E9 method: each is what the host makes of it, or declined and nowhere in the filter's list."""
    res, _, _, _ = emu.run(dc.args_of(xm8), streams, piece)
    for k, (status, out_len, out, listed) in enumerate(res):
        if status == 0:
            rc, want, _ = z.postprocess_block(xm8, streams[k])
            assert rc == 0 and out == want, (xm8, piece, k, streams[k][:16].hex(), len(streams[k]), out_len, rc, len(want))
            assert listed == (out_len > 0), (xm8, k)
        else:
            assert out is None and not listed, (xm8, k, status, "a declined stream in the filter's list")
    return [r[0] for r in res]


@pytest.mark.parametrize("order", ["", "reverse"])
@pytest.mark.parametrize("piece", wc.SEAM_PIECES)
def test_handmade_streams_under_an_e8e9_methods_parameters(zlib_, monkeypatch, piece, order):
    """The seams, the leap, the late meet, the chain, the runs and the deferred checks of lz77_decode_wide_cases: the stream's
    format does not know of the filter, so the statuses are those of the plain method, and a decoded output is the host's."""
    _order(monkeypatch, order)
    for xm in wc.METHODS:
        xm8 = e8w.e8_of(xm)
        named = [(c[0], c[3], False) for c in wc.seams() if c[1] == xm and c[2] == piece]
        named += [(c[0], c[2], False) for c in wc.long_literals() if c[1] == xm]
        named += [("chain", wc.chain(xm), False), ("runs", wc.runs(xm), False)]
        named += [(c[0], c[2], c[3]) for c in wc.deferred(64) if c[1] == xm]
        named += [(c[0], c[2], c[3]) for c in dc.handmade() if c[1] == xm]
        if xm == wc.late_meet()[0]:
            named.append(("late meet", wc.late_meet()[1], False))
        status = _exact_or_declined(zlib_, xm8, [s for _, s, _ in named], piece)
        for (name, _, declined), s in zip(named, status):
            assert (s != 0) == declined, (xm8, name, s)


@pytest.mark.parametrize("xm", cc.METHODS)
def test_damaged_streams_are_the_hosts_or_declined(zlib_, monkeypatch, xm):
    """The damaged batch of DESIGN 4.5.3 under the E8E9 form of its method: what the host makes of a stream, or declined -- with
    the statuses of the decoder without the filter, which no stream here makes give up --, and no declined stream in the list."""
    _order(monkeypatch, "")
    xm8 = e8w.e8_of(xm)
    streams, ncut = dc.damaged_batch(xm)
    status = _exact_or_declined(zlib_, xm8, streams, 64)
    assert status[0] == 0 and status[-1] == 0
    assert sum(1 for s in status if s) <= len(streams) - 2 - ncut
    _, plain, _, _ = lz77_decode_wide_emu.run(dc.args_of(xm), streams, 64)
    assert status == [r[0] for r in plain]
    res, _, _, _ = emu.run(dc.args_of(xm8), streams, 64)
    assert all(not r[3] for r in res if r[0] != 0)


@pytest.mark.parametrize("xm", cc.METHODS[:2])
def test_the_step_cap_drops_the_block_and_keeps_its_neighbours(zlib_, monkeypatch, xm):
    """A decoded block that is one chain of 2 000 seeds (7 997 serial steps) between two ordinary blocks, under a cap of 100
    steps: it is dropped with status 1, both neighbours are delivered and right; under the engine's cap it is delivered too."""
    _order(monkeypatch, "")
    xm8 = e8w.e8_of(xm)
    a, c = ec.blocks()[3], ec.x86_like(5000, 11)
    streams = [ec.stream_of(xm8, a), hc.preprocess(xm, ec.ADVERSARIAL)[0], ec.stream_of(xm8, c)]
    res, _, _, _ = emu.run(dc.args_of(xm8), streams, 256, max_steps=100)
    assert [r[0] for r in res] == [0, 1, 0], res
    assert res[1][1] == 0 and res[1][2] is None and res[1][3]             # it was in the list, and nothing of it is delivered
    assert res[0][2] == a and res[2][2] == c
    res, _, _, _ = emu.run(dc.args_of(xm8), streams, 256)
    rc, want, _ = zlib_.postprocess_block(xm8, streams[1])
    assert rc == 0 and want == ec.model(ec.ADVERSARIAL)
    assert [r[0] for r in res] == [0, 0, 0] and res[1][2] == want


def test_no_kernel_is_started_over_an_empty_total(zlib_, monkeypatch):
    """A batch whose outputs are all empty, and one whose only live stream is empty: both are delivered as they are (empty,
    declined) and none of link, jump, emit or the filter's kernels runs."""
    _order(monkeypatch, "")
    xm8 = e8w.METHODS[0]
    empty = ec.stream_of(xm8, b"")
    rc, want, _ = zlib_.postprocess_block(xm8, empty)
    assert rc == 0 and want == b""
    res, _, rounds, launches = emu.run(dc.args_of(xm8), [empty, empty, empty], 64)
    assert [(r[0], r[2], r[3]) for r in res] == [(0, b"", False)] * 3 and rounds == 0 and launches == 0
    bad = [c[2] for c in dc.handmade() if c[1] == cc.METHODS[0] and c[3]][0]            # (level 1, as xm8)
    res, _, rounds, launches = emu.run(dc.args_of(xm8), [bad, empty], 64)
    assert res[0][0] != 0 and res[0][2] is None and not res[0][3]
    assert (res[1][0], res[1][2], res[1][3]) == (0, b"", False) and rounds == 0 and launches == 0


def test_the_entries_exist_and_decline_without_a_device(zlib_):
    import zpaq_amd as z
    assert isinstance(z.last_device_une8_wide_segments(), int)
    bl = [b for b in ec.blocks() if 64 <= len(b) <= 700][:4]
    for xm in e8w.METHODS[:2]:
        streams = [ec.stream_of(xm, b) for b in bl]
        rc, bufs, sizes, status = z.e8e9_decode_device_wide(xm, streams, [len(b) for b in bl])
        if rc == 0:
            assert status == [0] * len(bl) and bufs == bl and sizes == [len(b) for b in bl]
        else:
            assert rc == 8 and b"device" in z.lib().zpq_last_error(), (rc, z.lib().zpq_last_error())
    # another kind of method is unsupported, with or without a device
    for other in ("x0,1,4,0,3,20", "x0,4", "x0,7", "x5,7", "x0,0"):
        rc, _, _, _ = z.e8e9_decode_device_wide(other, [b"\0" * 8], [16])
        assert rc == 8 and b"unavailable" in z.lib().zpq_last_error(), (other, rc)
