"""device/e8e9_kernel.h on the wavefront emulator (tests/emu/e8e9_emu_main.cpp): the mark pass, the scatter and the walk must
give, byte for byte, what the sequential scan gives -- the host's E8E9 program (zpq_postprocess_block of "x0,4"), whose readable
copy is e8e9_cases.model.  All blocks go in one ragged batch, every array at its exact size between inaccessible pages and dirty
at the start, with the lanes in order and reversed.  No GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import e8e9_cases as ec  # noqa: E402
import e8e9_emu  # noqa: E402


@pytest.fixture(scope="module")
def wanted():
    """model(block) of every block, once."""
    return tuple(ec.model(b) for b in ec.blocks())


def test_the_host_program_is_the_model(zlib_, wanted):
    changed = 0
    for k, (b, w) in enumerate(zip(ec.blocks(), wanted)):
        rc, out, _ = zlib_.postprocess_block("x0,4", b)
        assert rc == 0 and out == w, (k, len(b))
        changed += b != w
    assert 2 * changed > len(wanted)                                # most of the blocks do have hits


def test_the_chains_give_the_scan():
    """The argument of DESIGN 4.5.5 on 1 000 seeded strings of 0 - 700 bytes over the four alphabets, and the walks' lengths on
    the two shapes that bound them."""
    import random
    rng = random.Random(5)
    for r in range(1000):
        alphabet = ec.ALPHABETS[r % len(ec.ALPHABETS)]
        o = bytes(rng.choice(alphabet) for _ in range(rng.randrange(701)))
        assert ec.chains_model(o)[0] == ec.model(o), o.hex()
    for b in ec.blocks():
        assert ec.chains_model(b)[0] == ec.model(b), len(b)
    assert ec.chains_model(b"\xe8" + bytes(5000))[1] <= 8              # one chain of 5 000 candidates: skipped
    assert 7000 < ec.chains_model(ec.ADVERSARIAL)[1] < 10000           # one chain of 2 000 seeds: every position walked


@pytest.mark.parametrize("order", ["", "reverse"])
def test_every_block_is_filtered_as_the_scan_filters_it(monkeypatch, wanted, order):
    if order:
        monkeypatch.setenv("ZPQ_EMU_ORDER", order)
    else:
        monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    bl = ec.blocks()
    assert {len(b) for b in bl} >= set(range(10)) | set(range(ec.TILE - 5, ec.TILE + 6)) | set(range(2 * ec.TILE - 3, 2 * ec.TILE + 4)) | {70001}
    res = e8e9_emu.run(bl)
    for k, ((status, out), w) in enumerate(zip(res, wanted)):
        assert status == 0, (k, len(w), "declined")
        assert out == w, (k, len(w))


def test_the_step_cap_declines_and_does_not_truncate(monkeypatch):
    """7 997 serial steps do not fit a cap of 1 000: the block is absent, its neighbours are whole."""
    monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    a, c = ec.blocks()[3], ec.x86_like(5000, 11)
    res = e8e9_emu.run([a, ec.ADVERSARIAL, c], max_steps=1000)
    assert [r[0] for r in res] == [0, 1, 0]
    assert res[1][1] is None
    assert res[0][1] == ec.model(a) and res[2][1] == ec.model(c)
    res = e8e9_emu.run([ec.ADVERSARIAL], max_steps=8000)
    assert res[0] == (0, ec.model(ec.ADVERSARIAL))


def test_the_entries_exist_and_decline_without_a_device(zlib_):
    import zpaq_amd as z
    assert isinstance(z.last_device_une8_segments(), int)
    bl = [b for b in ec.blocks() if 64 <= len(b) <= 700][:4]
    for xm in ec.METHODS[:2]:
        streams = [ec.stream_of(xm, b) for b in bl]
        rc, bufs, sizes, status = z.e8e9_decode_device(xm, streams, [len(b) for b in bl])
        if rc == 0:
            assert status == [0] * len(bl) and bufs == bl and sizes == [len(b) for b in bl]
        else:
            assert rc == 8 and b"device" in z.lib().zpq_last_error(), (rc, z.lib().zpq_last_error())
    # another kind of method is unsupported, with or without a device
    for other in ec.OTHER_METHODS:
        rc, _, _, _ = z.e8e9_decode_device(other, [b"\0" * 8], [16])
        assert rc == 8 and b"unavailable" in z.lib().zpq_last_error(), (other, rc)
