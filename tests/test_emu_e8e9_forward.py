"""device/e8e9_forward_kernel.h on the wavefront emulator (tests/emu/e8e9_forward_emu_main.cpp): the mark pass, the scatter and
the walk must give, byte for byte, what the sequential scan gives -- the host's zpq_e8e9, whose readable copy is
e8e9_forward_cases.model.  The blocks lie back to back at whatever offsets their lengths give, the buffer at its exact size in front
of an inaccessible page and dirty at the start, with the lanes in order and reversed.  No GPU."""
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import e8e9_forward_cases as fc  # noqa: E402
import e8e9_forward_emu  # noqa: E402


@pytest.fixture(scope="module")
def wanted():
    """model(block) of every block, once."""
    return tuple(fc.model(b) for b in fc.blocks())


def test_the_host_filter_is_the_model(zlib_, wanted):
    import zpaq_amd as z
    changed = 0
    for k, (b, w) in enumerate(zip(fc.blocks(), wanted)):
        assert z.e8e9(b) == w, (k, len(b))
        changed += b != w
    assert 2 * changed > len(wanted)                                # most of the blocks do have hits


def test_the_chains_give_the_scan():
    """The decomposition on 2 000 seeded strings of 0 - 700 bytes over six alphabets, and the walks' lengths on the shapes that
    bound them."""
    rng = random.Random(5)
    alphabets = fc.ALPHABETS + ((0xe8, 0xff), (0xe8, 0xe9, 0xff, 0xff, 0x00, 0x00))
    for r in range(2000):
        alphabet = alphabets[r % len(alphabets)]
        o = bytes(rng.choice(alphabet) for _ in range(rng.randrange(80 if r % 2 else 701)))
        assert fc.chains_model(o)[0] == fc.model(o), o.hex()
    longest = 0
    for b in fc.blocks():
        out, steps = fc.chains_model(b)
        assert out == fc.model(b), len(b)
        longest = max(longest, steps)
    assert longest == fc.chains_model(fc.WORST)[1] == 6019            # every third position is a seed: no skipping
    assert fc.chains_model(fc.MANY_CHAINS)[1] <= 4                   # 2 000 chains, a head each
    assert fc.chains_model(fc.SKIPPING)[1] <= 8                      # one chain of 4 000 candidates: skipped
    assert fc.chains_model(fc.skipping_block())[1] <= 8


@pytest.mark.parametrize("order", ["", "reverse"])
def test_every_block_is_filtered_as_the_scan_filters_it(monkeypatch, wanted, order):
    """In one batch at the default cap: nothing declines."""
    if order:
        monkeypatch.setenv("ZPQ_EMU_ORDER", order)
    else:
        monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    bl = fc.blocks()
    assert {len(b) for b in bl} >= set(range(10)) | set(range(fc.TILE - 5, fc.TILE + 6)) | set(range(2 * fc.TILE - 3, 2 * fc.TILE + 4)) | {70001, 1 << 20}
    res = e8e9_forward_emu.run(bl)
    for k, ((status, out), w) in enumerate(zip(res, wanted)):
        assert status == 0, (k, len(w), "declined")
        assert out == w, (k, len(w))


def test_every_block_alone(monkeypatch, wanted):
    """One by one: a block at offset 0 that ends where the inaccessible page starts."""
    monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    for k, (b, w) in enumerate(zip(fc.blocks(), wanted)):
        assert e8e9_forward_emu.run([b]) == [(0, w)], (k, len(b))


def test_the_step_cap_declines_and_does_not_truncate(monkeypatch):
    """6 019 serial steps do not fit a cap of 1 000: the block is withheld, every other block of its batch is whole."""
    monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    bl = [b for b in fc.blocks() if len(b) < (1 << 20)]
    at = bl.index(fc.WORST)
    res = e8e9_forward_emu.run(bl, max_steps=1000)
    assert [r[0] for r in res] == [int(k == at) for k in range(len(bl))]
    assert res[at][1] is None
    for k, (b, r) in enumerate(zip(bl, res)):
        assert k == at or r[1] == fc.model(b), (k, len(b))
    res = e8e9_forward_emu.run([fc.WORST], max_steps=6019)
    assert res[0] == (0, fc.model(fc.WORST))


def test_the_entries_exist_and_decline_without_a_device(zlib_):
    import zpaq_amd as z
    assert isinstance(z.last_device_e8_blocks(), int)
    bl = [b for b in fc.blocks() if 64 <= len(b) <= 700][:4]
    rc, bufs, status = z.e8e9_device(bl)
    if rc == 0:
        assert status == [0] * len(bl) and bufs == [fc.model(b) for b in bl]
    else:
        assert rc == 8 and b"device" in z.lib().zpq_last_error(), (rc, z.lib().zpq_last_error())
        assert bufs == bl                                            # untouched
