"""The hash-table LZ77 parse (LZBuffer without a suffix array: method 1, method 2 below type 64, ...) as a token list on the
host: zpq_lz77_tokens_host followed by zpq_lz77_serialize must be zpq_preprocess_block, byte for byte -- the list is what the
device's parser (device/lz77_hash_kernel.h) hands back, the coder what turns it into the stream the archives pin.  No GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lz77_hash_cases as hc  # noqa: E402


def _check(xm, data):
    toks, seen = hc.host_tokens(xm, data)
    want, after = hc.preprocess(xm, data)
    assert seen == after, (xm, len(data), "E8E9")
    got = hc.serialize(xm, seen, toks)
    assert got == want, (xm, len(data), len(toks) // 16, len(got), len(want))
    return toks


@pytest.mark.parametrize("xm", hc.METHODS)
def test_token_list_then_coder_is_the_preprocessor(zlib_, xm):
    """Five kinds of input at 13 lengths: zeros reach the empty-looking table entry p(0) == 0 and one 49 152-byte match, random
    bytes the flush after 4 096 literals, lengths up to minMatchBoth a block that never inserts, every tail the frozen hashes."""
    ntok = 0
    for d in hc.inputs():
        ntok += len(_check(xm, d)) // 16
    assert ntok > 0


def test_offsets_of_two_bytes_and_more_at_level_2(zlib_):
    """Level 2 asks one byte more of a match whose offset needs three bytes: a repeat 70 000 bytes back."""
    import numpy as np
    for xm in hc.FAR_METHODS:
        toks = np.frombuffer(_check(xm, hc.far_repeat()), np.uint32).reshape(-1, 4)
        assert (toks[:, 1] >= 1 << 16).any(), xm
    _check("x0,2,3,5,2,12,1", hc.far_repeat())           # (a table of 2^12 slots has forgotten the first half by then)


def test_the_entries_still_refuse_what_is_no_lz77(zlib_):
    import ctypes as C
    for xm in ("x0,0", "x0,3", "x0,4", "x0,7"):
        rc, _, _ = hc.host_tokens_rc(xm, b"abcdabcdabcd")
        assert rc != 0, xm
    L = hc._lib()
    cnt = C.c_size_t(0)
    buf = (C.c_ubyte * 8)()
    assert L.zpq_lz77_tokens_host(b"x0,1,4,0,3,20", buf, 8, None, 4, C.byref(cnt)) != 0        # a capacity without a buffer
