"""device/fragment_kernel.h and the host's stitch (device/fragment_stitch.hpp) on the wavefront emulator
(tests/emu/fragment_emu_main.cpp): the records must be, field by field, what the serial scan gives (fragment_cases.model, which
test_fragment_host.py holds against zpq_fragment_host and the reference).  The whole ragged batch of fragment 0 goes in one
run, with pieces of 16 KiB and of 4 KiB, every array at its exact size between inaccessible pages and dirty at the start, with
the lanes in order and reversed.  No GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import fragment_cases as fc  # noqa: E402
import fragment_emu  # noqa: E402

LIMITS0 = (64, 8128, 1 << 22)


@pytest.fixture(scope="module")
def wanted():
    fc.check_shapes()
    return [[(sz, hits, o1) for sz, hits, _, o1 in m] for m in fc.models0()]


@pytest.mark.parametrize("order", ["", "reverse"])
@pytest.mark.parametrize("piece", [16384, 4096])
def test_the_batch_is_cut_as_the_scan_cuts_it(monkeypatch, wanted, piece, order):
    if order:
        monkeypatch.setenv("ZPQ_EMU_ORDER", order)
    else:
        monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    files = [d for _, d in fc.files0()]
    rounds, got = fragment_emu.run(files, piece, *LIMITS0)
    assert rounds >= 1
    for (name, _), g, w in zip(fc.files0(), got, wanted):
        assert [x[0] for x in g] == [x[0] for x in w], (name, "sizes")
        assert g == w, (name, "hits or tables")


def test_text_rejoins_in_the_first_round_and_zeros_never(monkeypatch, wanted):
    """Text, random bytes and records find a common cut a few KiB into every piece, so one fix-up round finishes them.  Zeros
    cut every 107 bytes and 4 096 is no multiple of it: every fix-up runs to its piece's end and moves the start of the next."""
    monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    f = dict(fc.files0())
    names = [k for k, _ in fc.files0()]
    for name in ("text", "lcg", "records"):
        rounds, got = fragment_emu.run([f[name]], 4096, *LIMITS0)
        assert rounds == 1, (name, rounds)
        assert got[0] == wanted[names.index(name)]
    rounds, got = fragment_emu.run([f["zeros"]], 4096, *LIMITS0)
    assert {x[0] for x in wanted[names.index("zeros")][:-1]} == {107}
    assert rounds == 4, rounds                                       # five pieces: one fix-up round per piece behind the first
    assert got[0] == wanted[names.index("zeros")]
    rounds, got = fragment_emu.run([f["pattern0"], f["pattern8128"]], 16384, *LIMITS0)
    assert rounds == 0                                               # one piece each: nothing to stitch


def test_other_limits(monkeypatch):
    """MIN = MAX (no room for the hash), and a threshold of 0 (fragment > 22: the hash never cuts)."""
    monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)
    f = dict(fc.files0())
    rounds, got = fragment_emu.run([f["text"][:30000], f["zeros"]], 4096, 1000, 1000, 1 << 22)
    assert [x[0] for x in got[0]] == [1000] * 30 + [0] and [x[0] for x in got[1]] == [1000] * 20 + [0]
    rounds, got = fragment_emu.run([f["text"][:30000]], 4096, 64, 8128, 0)
    assert [x[0] for x in got[0]] == [8128, 8128, 8128, 30000 - 3 * 8128]
