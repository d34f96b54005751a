"""device/lz77_decode_wide_kernel.h on the wavefront emulator (tests/emu/lz77_decode_wide_emu_main.cpp): the parse of a stream in
pieces from provisional starts, the stitch along the true walk, the deferred checks, and the copy by pointer jumping must give,
byte for byte, what the method's own PCOMP program makes of the stream on the host (zpq_postprocess_block) -- or decline the
stream, which no stream of this library's coder may be.  Several ragged streams go in one batch, every array at its exact size
between inaccessible pages, at pieces of 64, 256 and 4 096 stream bytes.  No GPU."""
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
import lz77_decode_wide_cases as wc  # noqa: E402
import lz77_decode_wide_emu  # noqa: E402
import lz77_hash_cases as hc  # noqa: E402

PIECES = (64, 256, 4096)


def _order(monkeypatch, order):
    if order:
        monkeypatch.setenv("ZPQ_EMU_ORDER", order)
    else:
        monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)


def _host(z, xm, stream):
    rc, out, _ = z.postprocess_block(xm, stream)
    return rc, out


def _decode_all(xm, streams, wants, piece):
    """Valid streams: everything is decoded, nothing declined.  Returns (piece counters, jump rounds)."""
    overflow, res, pieces, rounds = lz77_decode_wide_emu.run(dc.args_of(xm), streams, piece)
    assert not overflow
    for k, ((status, out_len, ntok, out), want) in enumerate(zip(res, wants)):
        assert status == 0, (xm, piece, k, len(streams[k]), status)
        assert ntok <= len(streams[k])
        assert out == want, (xm, piece, k, len(streams[k]), out_len, len(want))
    assert pieces[0] == sum((len(s) + piece - 1) // piece for s in streams) and sum(pieces[1:]) <= pieces[0]
    return pieces, rounds


def _exact_or_declined(z, xm, streams, piece):
    """Any streams: each is what the host makes of it, or declined.  Returns (statuses, piece counters, jump rounds)."""
    overflow, res, pieces, rounds = lz77_decode_wide_emu.run(dc.args_of(xm), streams, piece)
    assert not overflow
    for k, (status, out_len, ntok, out) in enumerate(res):
        if status == 0:
            rc, want = _host(z, xm, streams[k])
            assert rc == 0 and out == want, (xm, piece, k, streams[k][:16].hex(), len(streams[k]), out_len, rc, len(want))
        else:
            assert out is None
    return [r[0] for r in res], pieces, rounds


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
@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("xm", dc.METHODS)
def test_round_trip_of_every_input(host_streams, monkeypatch, xm, piece, order):
    """Every kind at every length as one ragged batch (streams shorter than a piece and of many pieces among them)."""
    _order(monkeypatch, order)
    host = host_streams(xm)
    assert sum(len(h[1]) == 70000 for h in host) == len(hc.KINDS) and any(len(h[1]) == 0 for h in host)
    pieces, _ = _decode_all(xm, [s for s, _ in host], [seen for _, seen in host], piece)
    if piece == 64:
        assert pieces[2] > 0                       # pieces whose list the walk met after a serial stretch


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("xm", cc.METHODS)
def test_synthetic_lists_through_the_coder_and_back(zlib_, monkeypatch, xm, piece):
    _order(monkeypatch, "")
    streams = [hc.serialize(xm, d, t) for _, d, t in cc.synthetic()]
    wants = []
    for s in streams:
        rc, want = _host(zlib_, xm, s)
        assert rc == 0
        wants.append(want)
    _decode_all(xm, streams, wants, piece)


def test_seeded_random_rounds(zlib_, monkeypatch):
    """Random lists through the host's coder and back, as in test_emu_lz77_decode.py: a stream the coder writes for a parse's list
    is never declined; any other is the host's output or declined."""
    _order(monkeypatch, "")
    rng = random.Random(47)
    faithful = 0
    for r in range(20):
        xm = cc.METHODS[r % len(cc.METHODS)]
        batch = cc.random_batch(rng)
        streams = [hc.serialize(xm, d, t) for d, t in batch]
        status, _, _ = _exact_or_declined(zlib_, xm, streams, PIECES[r % 2])
        for (d, t), s in zip(batch, status):
            if all(length >= cc.MM for length in memoryview(t).cast("I")[2::4]):
                assert s == 0, (xm, r, len(d))
                faithful += 1
    assert faithful >= 20


@pytest.mark.parametrize("order", ["", "reverse"])
@pytest.mark.parametrize("piece", wc.SEAM_PIECES)
def test_a_code_straddles_a_seam_at_every_bit_of_its_header(zlib_, monkeypatch, piece, order):
    _order(monkeypatch, order)
    for xm in wc.METHODS:
        cases = [c for c in wc.seams() if c[1] == xm and c[2] == piece]
        assert len(cases) == 2 * (24 if wc.level_of(xm) == 1 else 4)
        status, _, _ = _exact_or_declined(zlib_, xm, [c[3] for c in cases], piece)
        assert status == [0] * len(cases), (xm, piece, status)


def test_a_run_of_literals_leaps_over_whole_pieces(zlib_, monkeypatch):
    _order(monkeypatch, "")
    for name, xm, stream in wc.long_literals():
        status, pieces, _ = _exact_or_declined(zlib_, xm, [stream], 256)
        assert status == [0]
        # 4 096 literal bytes cover 16 pieces of 256 bytes: at least 15 lie wholly inside the code and are never entered
        assert pieces[0] >= 17 and pieces[0] - sum(pieces[1:]) >= 15, (xm, pieces)


def test_a_piece_that_meets_the_true_parse_only_behind_its_end(zlib_, monkeypatch):
    _order(monkeypatch, "")
    xm, stream = wc.late_meet()
    status, pieces, _ = _exact_or_declined(zlib_, xm, [stream], wc.LATE_PIECE)
    assert status == [0] and pieces[3] >= 1, pieces            # the walk went through that piece serially, to its end


@pytest.mark.parametrize("order", ["", "reverse"])
def test_a_chain_of_a_thousand_matches(zlib_, monkeypatch, order):
    """Depth 1 000: pointer jumping halves it per round (10 rounds when no lane sees another's work of the same round) and needs
    one round more at the most; in the order of the positions a round resolves everything."""
    _order(monkeypatch, order)
    for xm in wc.METHODS:
        status, _, rounds = _exact_or_declined(zlib_, xm, [wc.chain(xm)], 256)
        assert status == [0] and rounds <= 11, (xm, rounds)
        if order == "reverse":
            assert rounds >= 10, (xm, rounds)


@pytest.mark.parametrize("order", ["", "reverse"])
def test_runs_over_a_source_that_is_a_run(zlib_, monkeypatch, order):
    _order(monkeypatch, order)
    for xm in wc.METHODS:
        status, _, _ = _exact_or_declined(zlib_, xm, [wc.runs(xm)], 64)
        assert status == [0], xm


@pytest.mark.parametrize("order", ["", "reverse"])
def test_handmade_streams_of_the_narrow_decoder(zlib_, monkeypatch, order):
    """lz77_decode_cases.handmade(): the same verdicts, and the same statuses as the decoder of a wavefront per stream."""
    _order(monkeypatch, order)
    for xm in cc.METHODS:
        cases = [c for c in dc.handmade() if c[1] == xm]
        status, _, _ = _exact_or_declined(zlib_, xm, [c[2] for c in cases], 64)
        for (name, _, _, declined), s in zip(cases, status):
            assert (s != 0) == declined, (xm, name, s)
        _, narrow = lz77_decode_emu.run(dc.args_of(xm), [c[2] for c in cases])
        assert status == [r[0] for r in narrow], xm


def test_checks_that_need_the_absolute_position(zlib_, monkeypatch):
    _order(monkeypatch, "")
    for xm in wc.METHODS:
        cases = [c for c in wc.deferred(64) if c[1] == xm]
        status, pieces, _ = _exact_or_declined(zlib_, xm, [c[2] for c in cases], 64)
        for (name, _, _, declined), s in zip(cases, status):
            assert s == (1 if declined else 0), (xm, name, s)
        assert pieces[0] >= 3 * len(cases)


@pytest.mark.parametrize("xm", cc.METHODS)
def test_damaged_streams_are_the_hosts_or_declined(zlib_, monkeypatch, xm):
    """Each stream of a small valid batch cut at every length, a first code that is a match, non-zero pad bits: what the host
    makes of it, or declined, with the statuses of the decoder of a wavefront per stream."""
    _order(monkeypatch, "")
    streams, ncut = dc.damaged_batch(xm)
    status, _, _ = _exact_or_declined(zlib_, xm, streams, 64)
    assert status[0] == 0 and status[-1] == 0
    assert sum(1 for s in status if s) <= len(streams) - 2 - ncut
    _, narrow = lz77_decode_emu.run(dc.args_of(xm), streams)
    assert status == [r[0] for r in narrow]


def test_a_capacity_one_byte_short(zlib_, monkeypatch):
    """The host's step between the kernels: sizes first, and nothing is emitted when one does not fit."""
    _order(monkeypatch, "")
    xm = cc.METHODS[0]
    pairs = [hc.preprocess(xm, d) for d in hc.inputs()[20:26]]
    streams = [s for s, _ in pairs]
    sizes = [len(seen) for _, seen in pairs]
    overflow, res, _, _ = lz77_decode_wide_emu.run(dc.args_of(xm), streams, 64, caps=sizes)
    assert not overflow and [r[3] for r in res] == [seen for _, seen in pairs]
    caps = list(sizes)
    k = max(range(len(sizes)), key=lambda i: sizes[i])
    caps[k] -= 1
    overflow, res, _, _ = lz77_decode_wide_emu.run(dc.args_of(xm), streams, 64, caps=caps)
    assert overflow and [r[1] for r in res] == sizes and all(r[3] is None for r in res)


def test_the_entries_exist_and_decline_without_a_device(zlib_):
    import zpaq_amd as z
    xm = cc.METHODS[1]
    pairs = [hc.preprocess(xm, d) for d in hc.inputs()[20:24]]
    assert isinstance(z.last_device_unlz_wide_segments(), int)
    assert len(z.last_unlz_wide_pieces()) == 4 and isinstance(z.last_unlz_wide_rounds(), int)
    rc, bufs, sizes, status = z.lz77_decode_device_wide(xm, [s for s, _ in pairs], [len(d) for _, d in pairs])
    if rc == 0:
        assert status == [0] * len(pairs) and bufs == [d for _, d in pairs]
    else:
        assert rc == 8 and b"device" in z.lib().zpq_last_error(), (rc, z.lib().zpq_last_error())
    for other in (dc.E8E9, "x0,3", "x0,0"):
        rc, _, _, _ = z.lz77_decode_device_wide(other, [b"\x00\x01"], [16])
        assert rc == 8 and b"unavailable" in z.lib().zpq_last_error(), (other, rc)
