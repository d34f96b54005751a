"""device/bwt_decode_wide_kernel.h on the wavefront emulator (tests/emu/bwt_decode_wide_emu_main.cpp): the counting sort (the
small decoder's count, the scan in four parts, the 8-byte link), the list ranking over two levels of splitters (rank, rank2, offsets2,
offsets1) and the emission must give, byte for byte, what the program of a BWT method at args[0] > 4 makes of the stream on the
host (zpq_postprocess_block with x5,3) -- or decline the stream, which no stream of this library's BWT may be.  Several ragged
streams go in one batch, every array at its exact size between inaccessible pages and dirty at the start, with the lanes in
order and reversed.  No GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import bwt_decode_cases as bc  # noqa: E402
import bwt_decode_wide_cases as wc  # noqa: E402
import bwt_decode_wide_emu  # noqa: E402
import e8e9_cases as ec  # noqa: E402
import e8e9_emu  # noqa: E402


def _order(monkeypatch, order):
    if order:
        monkeypatch.setenv("ZPQ_EMU_ORDER", order)
    else:
        monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)


def _host(z, stream, method=wc.METHOD):
    rc, out, _ = z.postprocess_block(method, stream)
    return rc, out


@pytest.fixture(scope="module")
def host_of_valid_streams(zlib_):
    """The host's output of every valid stream, once (the program allocates its full arrays per call)."""
    return tuple(_host(zlib_, s) for s, _ in wc.valid_streams())


@pytest.mark.parametrize("order", ["", "reverse"])
def test_valid_streams_decode_to_their_blocks(monkeypatch, host_of_valid_streams, order):
    _order(monkeypatch, order)
    pairs = wc.valid_streams()
    sizes = {len(d) for _, d in pairs}
    assert sum(s == bc.EMPTY for s, _ in pairs) == 5 and {1, 2, 3, 255, 256, 257, 4095, 4096, 4097}.issubset(sizes)
    assert set(wc.LEVEL2_LENGTHS).issubset(sizes) and wc.LEVEL2_LENGTHS == (65535, 65536, 65537, 131073)
    overflow, res, batches = bwt_decode_wide_emu.run(wc.MBITS, [s for s, _ in pairs])
    assert not overflow and batches == 1
    for k, ((status, out_len, out), (s, d), (rc, want)) in enumerate(zip(res, pairs, host_of_valid_streams)):
        assert status == 0, (k, len(d))
        assert out == d, (k, len(d), out_len)
        assert rc == 0 and out == want, (k, len(d), rc)


def test_the_host_is_the_model_on_the_sample(zlib_):
    streams = bc.rule_streams()
    for k in wc.rule_sample():
        s, m = streams[k]
        assert _host(zlib_, s) == (0, m), (k, s.hex())


@pytest.mark.parametrize("order", ["", "reverse"])
def test_streams_under_the_rule(monkeypatch, order):
    """A path of n nodes is decoded to the model's bytes (the host's program written out); a shorter one (cycles beside it) is
    declined."""
    _order(monkeypatch, order)
    streams = bc.rule_streams()
    overflow, res, _ = bwt_decode_wide_emu.run(wc.MBITS, [s for s, _ in streams])
    assert not overflow
    whole = 0
    for k, ((status, out_len, out), (s, m)) in enumerate(zip(res, streams)):
        if len(m) == len(s) - 5:
            assert status == 0 and out == m, (k, s.hex())
            whole += 1
        else:
            assert status == 1 and out is None and out_len == 0, (k, s.hex())
    assert 20 <= whole <= 380


@pytest.mark.parametrize("order", ["", "reverse"])
def test_long_streams_under_the_rule(monkeypatch, order):
    """70 000 and 140 001 positions over 2 and 4 symbols: a short path with cycles through second-level splitters beside it is
    declined and nothing of it written; a real BWT of the same alphabet beside it is decoded."""
    _order(monkeypatch, order)
    streams = wc.large_rule_streams()
    overflow, res, _ = bwt_decode_wide_emu.run(wc.MBITS, [s for s, _ in streams])
    assert not overflow
    for k, ((status, out_len, out), (s, m)) in enumerate(zip(res, streams)):
        if len(m) == len(s) - 5:
            assert status == 0 and out == m, k
        else:
            assert status == 1 and out is None and out_len == 0, (k, len(m))


@pytest.mark.parametrize("order", ["", "reverse"])
def test_streams_outside_the_rule_are_declined(zlib_, monkeypatch, order):
    _order(monkeypatch, order)
    streams = bc.outside_batch()
    overflow, res, _ = bwt_decode_wide_emu.run(wc.MBITS, streams)
    assert not overflow
    assert res[0][0] == 0 and res[-1][0] == 0
    declined = 0
    for k, ((status, out_len, out), s) in enumerate(zip(res, streams)):
        m = bc.model(s)
        if m is None:
            assert status == 1 and out is None and out_len == 0, (k, s.hex())
            declined += 1
        elif len(m) == len(s) - 5:
            assert status == 0 and out == m, (k, s.hex())
        else:
            assert status == 1 and out is None, (k, s.hex())
    assert declined >= 40


def test_a_capacity_one_byte_short(monkeypatch):
    """Sizes are known before any kernel: nothing runs when one does not fit."""
    _order(monkeypatch, "")
    pairs = bc.valid_streams()[20:26] + (bc.outside_batch()[1],)
    streams = [s for s, _ in pairs[:-1]] + [pairs[-1]]
    sizes = [len(d) for _, d in pairs[:-1]] + [0]
    overflow, res, _ = bwt_decode_wide_emu.run(wc.MBITS, streams, caps=sizes)
    assert not overflow and [r[2] for r in res[:-1]] == [d for _, d in pairs[:-1]] and res[-1][0] == 1
    caps = list(sizes)
    k = max(range(len(sizes)), key=lambda i: sizes[i])
    caps[k] -= 1
    overflow, res, batches = bwt_decode_wide_emu.run(wc.MBITS, streams, caps=caps)
    assert overflow and batches == 0 and [r[1] for r in res] == sizes and all(r[2] is None for r in res)


def test_the_range():
    """mbits 25 .. 31, n + 257 must fit the program's H, and the 24-bit limit is gone.  The host's step alone: no array exists."""
    adm = bwt_decode_wide_emu.admitted
    assert adm(25, 1 << 24) == (True, False)                      # the smallest n the small form's word cannot hold
    assert adm(25, (1 << 24) - 1) == (True, True)
    assert adm(25, (1 << 25) - 257)[0] and not adm(25, (1 << 25) - 256)[0]
    assert adm(31, (1 << 31) - 257)[0] and not adm(31, (1 << 31) - 256)[0]
    assert adm(31, 1)[0] and adm(28, (1 << 28) - 257)[0] and not adm(28, (1 << 28) - 256)[0]
    assert not adm(24, 1000)[0] and not adm(32, 1000)[0] and not adm(20, 1000)[0]


@pytest.mark.parametrize("order", ["", "reverse"])
def test_a_batch_is_cut_where_its_outputs_pass_the_limit(monkeypatch, order):
    """Three streams under a limit that holds two go in two sub-batches and decode as they do in one."""
    _order(monkeypatch, order)
    pairs = [next(p for p in wc.valid_streams() if len(p[1]) == n) for n in (4097, 5000, 4096)]
    streams = [s for s, _ in pairs]
    sizes = sorted(len(d) for _, d in pairs)
    _, one, batches = bwt_decode_wide_emu.run(wc.MBITS, streams)
    assert batches == 1 and [r[2] for r in one] == [d for _, d in pairs]
    limit = max(len(pairs[0][1]) + len(pairs[1][1]), len(pairs[2][1]))
    assert limit < sum(sizes)
    _, two, batches = bwt_decode_wide_emu.run(wc.MBITS, streams, out_limit=limit)
    assert batches == 2 and two == one
    # a limit that holds one: three sub-batches; a stream that does not fit alone is declined, the others are decoded
    _, three, batches = bwt_decode_wide_emu.run(wc.MBITS, streams, out_limit=sizes[-1])
    assert batches == 3 and three == one
    _, res, batches = bwt_decode_wide_emu.run(wc.MBITS, streams, out_limit=sizes[-1] - 1)
    big = [k for k, (_, d) in enumerate(pairs) if len(d) == sizes[-1]]
    assert [r[0] for r in res] == [1 if k in big else 0 for k in range(3)]
    assert all(res[k][2] == pairs[k][1] for k in range(3) if k not in big)


@pytest.mark.parametrize("order", ["", "reverse"])
def test_the_e8e9_blocks_behind_the_wide_stage(zlib_, monkeypatch, order):
    """x5,7: the stage's output is the filtered block, and the device's inverse filter over it gives what the method's own windowed
    program makes of the stream."""
    _order(monkeypatch, order)
    blocks = [d for d in ec.blocks() if d]
    streams = [ec.stream_of(wc.E8_METHOD, d) for d in blocks]
    overflow, res, _ = bwt_decode_wide_emu.run(wc.MBITS, streams)
    assert not overflow and all(r[0] == 0 for r in res)
    back = e8e9_emu.run([r[2] for r in res])
    for k, ((status, out), d, s) in enumerate(zip(back, blocks, streams)):
        assert status == 0 and out == d, (k, len(d))
        if not order:
            assert _host(zlib_, s, wc.E8_METHOD) == (0, d), (k, len(d))


def test_the_entry_exists_and_declines_without_a_device(zlib_):
    import zpaq_amd as z
    pairs = bc.valid_streams()[20:24]
    rc, bufs, sizes, status = z.bwt_decode_device_wide(wc.METHOD, [s for s, _ in pairs], [len(d) for _, d in pairs])
    if rc == 0:
        assert status == [0] * len(pairs) and bufs == [d for _, d in pairs]
    else:
        assert rc == 8 and b"device" in z.lib().zpq_last_error(), (rc, z.lib().zpq_last_error())
    # another kind of method is unsupported, with or without a device
    for other in ("x0,3", "x4,3", "x5,1", "x0,0", "x12,3"):
        rc, _, _, _ = z.bwt_decode_device_wide(other, [bc.EMPTY], [16])
        assert rc == 8 and b"unavailable" in z.lib().zpq_last_error(), (other, rc)
    # the small entries keep refusing the wide methods
    assert z.bwt_decode_device(wc.METHOD, [bc.EMPTY], [16])[0] == 8
    assert z.e8e9_decode_device(wc.E8_METHOD, [bc.EMPTY], [16])[0] == 8
