"""device/lz77_hash_kernel.h on the wavefront emulator (tests/emu/lz77_hash_emu_main.cpp): the keys, the index, the search (one
lane per position, both values of the pending-literals bit) and the walk of lz77_kernel.h must give the host's list of matches
-- whose coded form is the pre-processor's stream (test_lz77_hash_host.py), which the reference's archives pin.  Several ragged
blocks go in one batch, empty ones among them: a read across a block's end would see the next block's bytes where the host sees
zeros.  No GPU."""
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import lz77_hash_cases as hc  # noqa: E402
import lz77_hash_emu  # noqa: E402


def _batch(zlib_, xm, datas, idx_bits=-1):
    a = zlib_.method_to_header(xm)[2]
    host = [hc.host_tokens(xm, d) for d in datas]
    got = lz77_hash_emu.run(a, [h[1] for h in host], idx_bits)
    for k, (h, g) in enumerate(zip(host, got)):
        assert h[0] == g, (xm, idx_bits, k, len(datas[k]), len(h[0]) // 16, len(g) // 16)


@pytest.mark.parametrize("order", ["", "reverse"])
@pytest.mark.parametrize("xm", hc.METHODS)
def test_device_parse_is_the_host_parse(zlib_, monkeypatch, xm, order):
    if order:
        monkeypatch.setenv("ZPQ_EMU_ORDER", order)
    else:
        monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    # every kind at every length up to 5 000; at 70 000 the inputs whose parse does something only a long block reaches -- zeros
    # (one 49 152-byte match, then the next), random bytes (the flush after 4 096 literals) and, in lane order, text (offsets past
    # 2^15).  The emulator's cost is per position: the other 70 000-byte inputs run on the host and on the GPU.
    long_kinds = ("zeros",) if order else ("zeros", "lcg", "text")
    ins = [d for k, d in enumerate(hc.inputs()) if len(d) <= 5000 or hc.KINDS[k % len(hc.KINDS)] in long_kinds]
    assert sum(len(d) == 70000 for d in ins) == len(long_kinds) and b"" in ins
    _batch(zlib_, xm, ins)


def test_far_offsets_and_any_index_width(zlib_, monkeypatch):
    """Offsets of 2^16 and more at level 2; and the answers do not depend on how fine the index is (none .. one entry per bucket)."""
    monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    _batch(zlib_, hc.FAR_METHODS[1], [hc.far_repeat()])
    small = [d for d in hc.inputs() if len(d) <= 5000]
    for xm in ("x0,1,4,8,3,16,2", "x0,1,4,0,0,10"):
        for bits in (0, 3, 24):
            _batch(zlib_, xm, small, bits)


def fuzz_round(zlib_, rng):
    """Random parameters inside the device's range, random ragged inputs, one batch."""
    from zpaq_amd import corpus
    level = rng.choice([1, 2])
    mm = rng.randrange(4, 10) if level == 1 else rng.randrange(2, 12)
    mm2 = rng.choice([0, 0, rng.randrange(1, 14)])
    la = rng.choice([0, 0, 1, 2, 3, 7]) if mm2 else 0
    lb = rng.randrange(0, 5)
    a0 = rng.choice([0, 0, 1, 4])
    bits = rng.randrange(max(lb, 1), min(20 + a0, 24) + 1)
    xm = "x%d,%d,%d,%d,%d,%d,%d" % (a0, level + (4 if rng.random() < 0.25 else 0), mm, mm2, lb, bits, la)

    def data(n):
        k = rng.randrange(7)
        if k < 5:
            return corpus.block(hc.KINDS[k], n, rng.randrange(1 << 30)).tobytes()
        if k == 5:
            return bytes(rng.choice(b"abc") for _ in range(n))
        unit = bytes(rng.randrange(256) for _ in range(rng.randrange(1, 40)))
        out = b""
        while len(out) < n:
            out += unit * rng.randrange(1, 300) + bytes(rng.randrange(256) for _ in range(rng.randrange(0, 30)))
        return out[:n]

    ns = [rng.choice([0, 1, 2, 5, 11, 17, 64, 255, 300, 1000, 2500, 4095, 4097, 6000, 9000]) for _ in range(6)]
    if rng.random() < 0.15:
        ns.append(rng.randrange(20000, 70000))
    _batch(zlib_, xm, [data(n) for n in ns])
    return xm, ns


def test_seeded_fuzz_round(zlib_, monkeypatch):
    monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    rng = random.Random(20)
    for _ in range(20):
        fuzz_round(zlib_, rng)
