"""device/bwt_decode_kernel.h on the wavefront emulator (tests/emu/bwt_decode_emu_main.cpp): the counting sort (count, scan,
link), the list ranking (rank, offsets) and the emission must give, byte for byte, what the BWT method's own PCOMP program makes
of the stream on the host (zpq_postprocess_block) -- or decline the stream, which no stream of this library's BWT may be.
Several ragged streams go in one batch, every array at its exact size between inaccessible pages and dirty at the start, with
the lanes in order and reversed.  No GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import bwt_decode_cases as bc  # noqa: E402
import bwt_decode_emu  # noqa: E402

MBITS = bc.mbits_of(bc.METHOD)


def _order(monkeypatch, order):
    if order:
        monkeypatch.setenv("ZPQ_EMU_ORDER", order)
    else:
        monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)


def _host(z, stream):
    rc, out, _ = z.postprocess_block(bc.METHOD, stream)
    return rc, out


@pytest.fixture(scope="module")
def host_of_rule_streams(zlib_):
    """The host's output of the 400 streams under the rule, once."""
    return tuple(_host(zlib_, s) for s, _ in bc.rule_streams())


@pytest.mark.parametrize("order", ["", "reverse"])
def test_valid_streams_decode_to_their_blocks(zlib_, monkeypatch, order):
    _order(monkeypatch, order)
    pairs = bc.valid_streams()
    assert sum(s == bc.EMPTY for s, _ in pairs) == 5 and any(len(d) == 3 * bc.TILE + 1 for _, d in pairs)
    overflow, res = bwt_decode_emu.run(MBITS, [s for s, _ in pairs])
    assert not overflow
    for k, ((status, out_len, out), (s, d)) in enumerate(zip(res, pairs)):
        assert status == 0, (k, len(d))
        assert out == d, (k, len(d), out_len)
        rc, want = _host(zlib_, s)
        assert rc == 0 and out == want, (k, len(d), rc)


def test_the_host_is_the_model_under_the_rule(host_of_rule_streams):
    for (s, m), (rc, out) in zip(bc.rule_streams(), host_of_rule_streams):
        assert rc == 0 and out == m, (s.hex(), rc)


@pytest.mark.parametrize("order", ["", "reverse"])
def test_streams_under_the_rule(monkeypatch, host_of_rule_streams, order):
    """A path of n nodes is decoded; a shorter one (cycles beside it) is declined, or the host's bytes."""
    _order(monkeypatch, order)
    streams = bc.rule_streams()
    overflow, res = bwt_decode_emu.run(MBITS, [s for s, _ in streams])
    assert not overflow
    for k, ((status, out_len, out), (s, m), (rc, want)) in enumerate(zip(res, streams, host_of_rule_streams)):
        assert status in (0, 1)
        if len(m) == len(s) - 5:
            assert status == 0, (k, s.hex())
        if status == 0:
            assert rc == 0 and out == want, (k, s.hex())
        else:
            assert out is None


@pytest.mark.parametrize("order", ["", "reverse"])
def test_streams_outside_the_rule_are_declined(zlib_, monkeypatch, order):
    _order(monkeypatch, order)
    streams = bc.outside_batch()
    overflow, res = bwt_decode_emu.run(MBITS, streams)
    assert not overflow
    assert res[0][0] == 0 and res[-1][0] == 0
    declined = 0
    for k, ((status, out_len, out), s) in enumerate(zip(res, streams)):
        if bc.model(s) is None:
            assert status == 1 and out is None and out_len == 0, (k, s.hex())
            declined += 1
        elif status == 0:
            rc, want = _host(zlib_, s)
            assert rc == 0 and out == want, (k, s.hex())
        else:
            assert status == 1 and out is None
    assert declined >= 40


def test_a_capacity_one_byte_short(monkeypatch):
    """Sizes are known before any kernel: nothing runs when one does not fit."""
    _order(monkeypatch, "")
    pairs = bc.valid_streams()[20:26] + (bc.outside_batch()[1],)
    streams = [s for s, _ in pairs[:-1]] + [pairs[-1]]
    sizes = [len(d) for _, d in pairs[:-1]] + [0]
    overflow, res = bwt_decode_emu.run(MBITS, streams, caps=sizes)
    assert not overflow and [r[2] for r in res[:-1]] == [d for _, d in pairs[:-1]] and res[-1][0] == 1
    caps = list(sizes)
    k = max(range(len(sizes)), key=lambda i: sizes[i])
    caps[k] -= 1
    overflow, res = bwt_decode_emu.run(MBITS, streams, caps=caps)
    assert overflow and [r[1] for r in res] == sizes and all(r[2] is None for r in res)


def test_the_range(monkeypatch):
    """n + 257 must fit the program's H; the node rides in 24 bits.  The host's step alone: no kernel runs."""
    _order(monkeypatch, "")

    def stream(n):
        body = bytearray(n + 1)
        body[1] = 255
        return bytes(body) + (1).to_bytes(4, "little")
    edge = (1 << 20) - 257
    _, res = bwt_decode_emu.run(20, [stream(edge), stream(edge + 1)], admit_only=True)
    assert [r[0] for r in res] == [0, 1] and res[0][1] == edge
    _, res = bwt_decode_emu.run(24, [stream((1 << 24) - 257), stream(1 << 24)], admit_only=True)
    assert [r[0] for r in res] == [0, 1]
    _, res = bwt_decode_emu.run(32, [stream((1 << 24) - 1), stream(1 << 24)], admit_only=True)
    assert [r[0] for r in res] == [0, 1]


def test_the_entries_exist_and_decline_without_a_device(zlib_):
    import zpaq_amd as z
    pairs = bc.valid_streams()[20:24]
    assert isinstance(z.last_device_unbwt_segments(), int)
    rc, bufs, sizes, status = z.bwt_decode_device(bc.METHOD, [s for s, _ in pairs], [len(d) for _, d in pairs])
    if rc == 0:
        assert status == [0] * len(pairs) and bufs == [d for _, d in pairs]
    else:
        assert rc == 8 and b"device" in z.lib().zpq_last_error(), (rc, z.lib().zpq_last_error())
    # another kind of method is unsupported, with or without a device
    for other in ("x0,7", "x5,3", "x0,1,4,0,3,20", "x0,0"):
        rc, _, _, _ = z.bwt_decode_device(other, [bc.EMPTY], [16])
        assert rc == 8 and b"unavailable" in z.lib().zpq_last_error(), (other, rc)
