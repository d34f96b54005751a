"""The batched suffix sort (device/sa_kernel.h: the kernels' bodies and the loop's two decisions, as device/sa_kernels.hip runs
them) on the host-side emulator, over the inputs of tests/sort_cases.py: every array at its exact size between guard pages,
std::stable_sort on the masked key and std::partial_sum in place of the two library calls (tests/emu/sa_emu.h)."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import emu  # noqa: E402
import sort_cases as sc  # noqa: E402


@pytest.fixture(scope="module")
def shapes():
    return sc.batch_shapes(sc.CPU_LENGTHS)


def test_the_reference_side_on_the_hard_inputs(zlib_, shapes):
    """Before any kernel is judged by it: the host sorter against Python's sort of the suffixes, every block of at most 3 000 bytes."""
    assert sc.check_reference_side(shapes) > 300


def test_the_reference_side_against_divsufsort(zlib_, ref, shapes):
    """... and against the reference's own sorter, the longer blocks too."""
    assert sc.check_reference_side(shapes, ref) > 300


def _check_batch(shape, blocks, sa, rank):
    for k, ((name, d), s, r) in enumerate(zip(blocks, sa, rank)):
        want = sc.expected(d)
        assert s.size == len(d) and r.size == len(d), (shape, k, name, s.size, r.size)
        bad = np.flatnonzero(s != want)
        assert bad.size == 0, (shape, k, name, "suffix array differs first at", int(bad[0]), int(s[bad[0]]), int(want[bad[0]]))
        inv = np.empty(len(d), np.uint32)
        inv[want] = np.arange(1, len(d) + 1, dtype=np.uint32)
        bad = np.flatnonzero(r != inv)
        assert bad.size == 0, (shape, k, name, "rank is not the inverse + 1 first at", int(bad[0]))


def test_every_batch_shape_against_the_host_sorter(zlib_, shapes):
    """One block alone (every hard string at every length), two and three blocks, 256 and 257 blocks, the boundary batch: the
    emulated arrays are the host sorter's entry for entry, the ranks the loop ends with are the inverse array + 1 (what
    lz77_search_body and bwt_emit_body consume), and no access leaves an array (a guard page ends the emulator: emu.sa_run_batches
    raises)."""
    got = emu.sa_run_batches([[d for _, d in blocks] for _, blocks in shapes], [k for k, _ in shapes])
    assert len(got) == len(shapes)
    for (shape, blocks), (sa, rank, rounds) in zip(shapes, got):
        _check_batch(shape, blocks, sa, rank)
        assert rounds <= max(1, math.ceil(math.log2(max(len(d) for _, d in blocks)))), (shape, rounds)


ROUND_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 4095, 4096, 4097)


def test_rounds_of_a_run_of_zeros(zlib_):
    """zeros(n) alone takes max(1, ceil(log2 n)) rounds -- round k tells prefixes of 2^k bytes apart, the suffixes of a run differ
    only in their length -- and a batch takes the count of its slowest block."""
    batches = [[bytes(n)] for n in ROUND_LENGTHS] + [[bytes(4096), sc.lcg(4096, 5)], [sc.lcg(4096, 5)]]
    got = emu.sa_run_batches(batches)
    for n, (sa, rank, rounds) in zip(ROUND_LENGTHS, got):
        assert rounds == max(1, math.ceil(math.log2(n))), ("zeros", n, rounds)
        assert (sa[0] == np.arange(n - 1, -1, -1, dtype=np.uint32)).all(), ("zeros", n)
    (sa, rank, rounds), (_, _, lcg_rounds) = got[-2], got[-1]
    assert rounds == 12 and lcg_rounds < 12, ("zeros(4096) beside lcg(4096)", rounds, lcg_rounds)
    _check_batch("zeros(4096),lcg(4096)", (("run00/4096", bytes(4096)), ("lcg/4096", sc.lcg(4096, 5))), sa, rank)


def test_the_loops_two_decisions(zlib_):
    """The helpers of device/sa_kernel.h themselves.  Key bits: 48 + the bits of the largest block id, either side of every power
    of two.  Stop rule: all names distinct, or h has reached the longest block.  The second clause never ends a healthy sort
    (a round with 2h >= max_len tells whole suffixes apart, so the names are distinct a round earlier: no input reaches it), it
    bounds the loop -- so it is checked here, directly, and not through an input."""
    for nblocks, bits in ((1, 49), (2, 49), (3, 50), (4, 50), (5, 51), (255, 56), (256, 56), (257, 57), (32768, 63), (32769, 64), (65535, 64)):
        assert emu.sa_helper("bits", nblocks) == bits, nblocks
    for names, total, h, max_len, stop in ((10, 10, 1, 10, 1), (9, 10, 1, 10, 0), (9, 10, 8, 10, 0), (9, 10, 16, 10, 1), (9, 10, 10, 10, 1),
                                           (1, 3, 1, 3, 0), (2, 3, 1, 3, 0), (2, 3, 2, 3, 0), (4095, 4096, 2048, 4096, 0), (1, 1, 1, 1, 1)):
        assert emu.sa_helper("stop", names, total, h, max_len) == stop, (names, total, h, max_len)
