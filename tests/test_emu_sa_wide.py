"""The wide suffix sort (device/sa_wide_kernel.h: the kernels' bodies and the host helpers, as build_suffix_array_wide in
device/sa_kernels.hip runs them) on the host-side emulator, over the hard strings of tests/sort_cases.py, each as a block alone:
every array at its exact size between guard pages and dirty at the start, std::stable_sort on the masked key and std::partial_sum
in place of the two library calls (tests/emu/sa_wide_emu_main.cpp).  And the host side of the split without a device."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import sa_wide_emu  # noqa: E402
import sort_cases as sc  # noqa: E402

u8p = C.POINTER(C.c_ubyte)
TINY = (("byte00", b"\x00"), ("byteFF", b"\xff"), ("byte61", b"a"), ("aa", b"aa"), ("ab", b"ab"), ("ba", b"ba"), ("00FF", b"\x00\xff"), ("FF00", b"\xff\x00"),
        ("aaa", b"aaa"), ("aab", b"aab"), ("aba", b"aba"), ("baa", b"baa"), ("FFFFFF", b"\xff\xff\xff"), ("FF00FF", b"\xff\x00\xff"))
WIDTH_LENGTH = 4097
UNSUPPORTED = 8                 # ZPQ_E_UNSUPPORTED


def _blocks(lengths):
    """(name, bytes) of every hard string at these lengths, and the blocks of 1, 2 and 3 bytes."""
    return [(f"{k}/{n}", d) for n in lengths for k, d in sc.strings(n)] + [(f"{k}/{len(d)}", d) for k, d in TINY]


@pytest.fixture(scope="module")
def blocks():
    return _blocks(sc.CPU_LENGTHS)


@pytest.fixture(scope="module")
def sorted_blocks(blocks):
    """Every block through the emulated sort at its natural field width, once for the tests below (read only)."""
    return sa_wide_emu.run([d for _, d in blocks], 0, [k for k, _ in blocks])


def _check(name, d, sa, rank):
    want = sc.expected(d)
    assert sa.size == len(d) and rank.size == len(d), (name, sa.size, rank.size)
    bad = np.flatnonzero(sa != want)
    assert bad.size == 0, (name, "suffix array differs first at", int(bad[0]), int(sa[bad[0]]), int(want[bad[0]]))
    inv = np.empty(len(d), np.uint32)
    inv[want] = np.arange(1, len(d) + 1, dtype=np.uint32)
    bad = np.flatnonzero(rank != inv)
    assert bad.size == 0, (name, "rank is not the inverse + 1 first at", int(bad[0]))


def test_every_hard_string_against_the_host_sorter(zlib_, blocks, sorted_blocks):
    """The emulated arrays are the host sorter's entry for entry, the ranks the loop ends with are the inverse array + 1 (what
    bwt_wide_body consumes), the rounds stay within max(1, ceil(log2 n)), and no access leaves an array (a guard page ends the
    emulator: sa_wide_emu.run raises)."""
    assert len(sorted_blocks) == len(blocks) > 300
    for (name, d), (sa, rank, _, rounds) in zip(blocks, sorted_blocks):
        _check(name, d, sa, rank)
        assert 1 <= rounds <= max(1, math.ceil(math.log2(len(d)))), (name, rounds)


def test_rounds_of_a_run_of_zeros(zlib_, blocks, sorted_blocks):
    """zeros(n) takes exactly max(1, ceil(log2 n)) rounds: round k tells prefixes of 2^k bytes apart, and the suffixes of a run
    differ only in their length."""
    seen = 0
    for (name, d), (sa, _, _, rounds) in zip(blocks, sorted_blocks):
        if d != bytes(len(d)):
            continue
        seen += 1
        assert rounds == max(1, math.ceil(math.log2(len(d)))), (name, rounds)
        assert (sa == np.arange(len(d) - 1, -1, -1, dtype=np.uint32)).all(), name
    assert seen == len(sc.CPU_LENGTHS) + 1


@pytest.mark.parametrize("bits", [25, 31])
def test_forced_field_widths(zlib_, bits):
    """The widths a block of 16 MiB and of 2 GiB - 4096 bytes would use, on strings of 4097 bytes: the key is rank << bits | rank,
    the stand-in sort masks 2 * bits bits.  Arrays, ranks and rounds are those of the natural width (13 bits)."""
    cases = _blocks((WIDTH_LENGTH,))
    natural = sa_wide_emu.run([d for _, d in cases], 0, [k for k, _ in cases])
    forced = sa_wide_emu.run([d for _, d in cases], bits, [k for k, _ in cases])
    for (name, d), (sa0, rank0, bwt0, rounds0), (sa, rank, bwt, rounds) in zip(cases, natural, forced):
        _check(name, d, sa0, rank0)
        assert (sa == sa0).all() and (rank == rank0).all() and bwt == bwt0 and rounds == rounds0, (name, bits, rounds, rounds0)


def test_rank_field_width(zlib_):
    """sa_wide_rank_bits: the smallest r with 2^r > n (ranks are 1..n, 0 is past the end).  sa_wide_field_bits: the first round's
    ranks are byte + 1, up to 256, whatever n is -- its fields are never narrower than 9 bits; later rounds use r."""
    for n, r in ((1, 1), (2, 2), (3, 2), (4, 3), ((1 << 24) - 1, 24), (1 << 24, 25), ((1 << 31) - 4096, 31),
                 (255, 8), (256, 9), ((1 << 26) - 4096, 26), ((1 << 31) - 1, 31)):
        assert sa_wide_emu.helper("bits", n) == r, n
    for r, h, w in ((1, 1, 9), (8, 1, 9), (9, 1, 9), (25, 1, 25), (1, 2, 1), (8, 2, 8), (8, 4, 8), (31, 1, 31), (31, 1 << 30, 31)):
        assert sa_wide_emu.helper("field", r, h) == w, (r, h)


def _host_stream(L, xm, d):
    buf = np.frombuffer(bytes(d), np.uint8).copy()
    out = np.empty(len(d) + 64, np.uint8)
    ol = C.c_size_t(0)
    assert L.zpq_preprocess_block(xm.encode(), buf.ctypes.data_as(u8p), len(d), out.ctypes.data_as(u8p), out.size, C.byref(ol)) == 0
    return out[:ol.value].tobytes()


def test_bwt_body_against_the_host(zlib_, blocks, sorted_blocks):
    """bwt_wide_body's column and index, scattered from the ranks, are byte for byte the stream zpq_preprocess_block("x0,3")
    writes -- on every block above (the one-byte blocks among them), and on blocks with a real 255 where the index stands."""
    L = zlib_.lib()
    L.zpq_preprocess_block.argtypes = [C.c_char_p, u8p, C.c_uint32, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    for (name, d), (_, _, bwt, _) in zip(blocks, sorted_blocks):
        assert bwt == _host_stream(L, "x0,3", d), name
    # a real 255 in the column beside the 255 that stands for the byte in front of the whole string
    extra = [("FF+lcg", b"\xff" + sc.lcg(300, 3)), ("lcg+FF", sc.lcg(300, 4) + b"\xff"), ("00FF00", b"\x00\xff\x00"), ("FFx5", b"\xff" * 5),
             ("aFFb", b"a\xffb" * 40)]
    got = sa_wide_emu.run([d for _, d in extra], 0, [k for k, _ in extra])
    for (name, d), (sa, rank, bwt, _) in zip(extra, got):
        _check(name, d, sa, rank)
        want = _host_stream(L, "x0,3", d)
        assert bwt == want, name
        idx = int.from_bytes(want[-4:], "little")
        assert want[idx] == 255 and want[:-4].count(255) >= 2, (name, "the case has no real 255 beside the index")


def test_entries_without_a_device(zlib_):
    """The host side of the split: without a device both stage entries say ZPQ_E_UNSUPPORTED with a note and touch nothing; a method
    that does not sort suffixes is refused whatever the machine has; the counter exists."""
    import zpaq_amd as z
    L = z.lib()
    assert z.last_wide_sort_blocks() == 0
    assert isinstance(z.last_wide_sort_rounds(), int)
    d = sc.lcg(1000, 9)
    for xm in ("x0,0", "x0,4", "x0,1,4,0,3,16,1"):      # nothing, E8E9 alone, LZ77 through the hash table
        rc, out, size = z.preprocess_block_device_wide(xm, d, 2000, guard=8, fill=0x5A)
        assert rc == UNSUPPORTED and size == 0, xm
        assert "does not sort suffixes" in L.zpq_last_error().decode(), xm
        assert out == b"\x5a" * 2008, xm
    L.zpq_device_count.restype = C.c_int
    if L.zpq_device_count() > 0:
        return                                        # (with a device the entries work: tests/test_gpu_sort_wide.py)
    rc, sa = z.suffix_array_device_wide(d, spare=1, fill=0xA5A5A5A5)
    assert rc == UNSUPPORTED and "no device" in L.zpq_last_error().decode()
    assert (sa == 0xA5A5A5A5).all()
    for xm in ("x0,3", "x0,7", "x0,2,5,0,7,21,1c0,0,511"):
        buf = np.frombuffer(d, np.uint8).copy()
        rc, out, size = z.preprocess_block_device_wide(xm, buf, 2000, guard=8, fill=0x5A)
        assert rc == UNSUPPORTED and "no device" in L.zpq_last_error().decode(), xm
        assert out == b"\x5a" * 2008 and buf.tobytes() == d, xm
