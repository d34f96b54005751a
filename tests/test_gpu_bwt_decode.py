"""BWT streams decoded on the device (device/bwt_decode_kernel.h): zpq_bwt_decode_device against the blocks the streams were
made from and against the host's post-processor (zpq_postprocess_block), with guard bytes behind exact capacities, the overflow
and decline contracts, and archives through zpq_decompress with ZPAQ_AMD_DEVICE_UNBWT on, off and unset, each in a fresh
process."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bwt_decode_cases as bc  # noqa: E402
import lz77_hash_cases as hc  # noqa: E402

from zpaq_amd import corpus  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xC3
ROOT = os.path.dirname(HERE)


def _all_decoded(gpu, xm, streams, wants):
    rc, bufs, sizes, status = gpu.bwt_decode_device(xm, streams, [len(w) for w in wants], guard=GUARD, fill=FILL)
    assert rc == 0, (xm, gpu.lib().zpq_last_error().decode())
    assert status == [0] * len(streams), (xm, status)
    assert sizes == [len(w) for w in wants]
    for k, (b, w) in enumerate(zip(bufs, wants)):
        assert b[:len(w)] == w, (xm, k, len(w))
        assert b[len(w):] == bytes([FILL]) * GUARD, (xm, k, "a store past the capacity")


def test_valid_streams_decode_to_their_blocks(gpu):
    pairs = bc.valid_streams()
    _all_decoded(gpu, bc.METHOD, [s for s, _ in pairs], [d for _, d in pairs])


def test_a_block_of_a_mebibyte(gpu):
    """1 048 319 bytes: the largest block x0,3's program holds (n + 257 = 2^20)."""
    d = corpus.block("text", 1048319, 4321).tobytes()
    s, _ = hc.preprocess(bc.METHOD, d)
    rc, want, _ = gpu.postprocess_block(bc.METHOD, s)
    assert rc == 0 and want == d
    _all_decoded(gpu, bc.METHOD, [s], [d])


def test_blocks_around_two_mebibytes(gpu):
    """More than 8 192 splitters, links beyond 21 bits.  The stream does not depend on args[0]; the program's room does:
    x1,3 holds 2^21 - 257 bytes, so 2^21 + 3 take x2,3 and are declined, untouched, for x1,3 and x0,3."""
    d = corpus.block("records", (1 << 21) + 3, 4322).tobytes()
    s, _ = hc.preprocess(bc.HUGE_METHOD, d)
    _all_decoded(gpu, bc.HUGE_METHOD, [s, bc.EMPTY], [d, b""])
    for xm in (bc.BIG_METHOD, bc.METHOD):
        rc, bufs, sizes, status = gpu.bwt_decode_device(xm, [s], [len(d)], guard=GUARD, fill=FILL)
        assert rc == 0 and status == [1] and sizes == [0] and bufs[0] == bytes([FILL]) * len(bufs[0]), xm
    d = d[:(1 << 21) - 257]
    s, _ = hc.preprocess(bc.BIG_METHOD, d)
    _all_decoded(gpu, bc.BIG_METHOD, [s], [d])


def test_streams_under_the_rule(gpu):
    streams = bc.rule_streams()
    host = [gpu.postprocess_block(bc.METHOD, s) for s, _ in streams]
    rc, bufs, sizes, status = gpu.bwt_decode_device(bc.METHOD, [s for s, _ in streams], [len(s) - 5 for s, _ in streams], guard=GUARD, fill=FILL)
    assert rc == 0, gpu.lib().zpq_last_error().decode()
    for k, ((s, m), (hrc, want, _), b, st) in enumerate(zip(streams, host, bufs, status)):
        assert hrc == 0 and want == m
        if len(m) == len(s) - 5:
            assert st == 0, (k, s.hex())
        if st == 0:
            assert sizes[k] == len(want) and b[:len(want)] == want, (k, s.hex())
            assert b[len(want):] == bytes([FILL]) * (len(b) - len(want)), k
        else:
            assert st == 1 and sizes[k] == 0 and b == bytes([FILL]) * len(b), (k, "a declined stream's output was touched")


def test_a_buffer_too_small_reports_every_size(gpu):
    pairs = bc.valid_streams()
    sizes_want = [len(d) for _, d in pairs]
    caps = list(sizes_want)
    short = max(range(len(caps)), key=lambda k: caps[k])
    caps[short] -= 1
    rc, bufs, sizes, status = gpu.bwt_decode_device(bc.METHOD, [s for s, _ in pairs], caps, guard=GUARD, fill=FILL)
    assert rc == 3, rc                                                # ZPQ_E_OVERFLOW
    assert sizes == sizes_want
    assert all(b == bytes([FILL]) * len(b) for b in bufs), "an overflowing batch wrote something"


def test_streams_outside_the_rule_are_declined(gpu):
    streams = bc.outside_batch()
    caps = [max(len(s) - 5, 0) for s in streams]
    rc, bufs, sizes, status = gpu.bwt_decode_device(bc.METHOD, streams, caps, guard=GUARD, fill=FILL)
    assert rc == 0, gpu.lib().zpq_last_error().decode()
    assert status[0] == 0 and status[-1] == 0
    for k, (s, b, st) in enumerate(zip(streams, bufs, status)):
        if bc.model(s) is None:
            assert st == 1, (k, s.hex())
        if st == 0:
            hrc, want, _ = gpu.postprocess_block(bc.METHOD, s)
            assert hrc == 0 and sizes[k] == len(want) and b[:len(want)] == want, (k, s.hex())
            assert b[len(want):] == bytes([FILL]) * (len(b) - len(want)), k
        else:
            assert st == 1 and sizes[k] == 0 and b == bytes([FILL]) * len(b), (k, "a declined stream's output was touched")


def test_a_capacity_one_byte_short_among_declined_streams(gpu):
    good, d = bc.valid_streams()[30]
    bad = bc.outside_batch()[1]
    assert len(d) > 0 and bc.model(bad) is None
    rc, bufs, sizes, status = gpu.bwt_decode_device(bc.METHOD, [good, bad, good], [len(d), 64, len(d) - 1], guard=GUARD, fill=FILL)
    assert rc == 3 and sizes == [len(d), 0, len(d)]
    assert all(b == bytes([FILL]) * len(b) for b in bufs)


# ---- archives: each setting in a fresh process ----
BWT_METHODS = ("x0,3", "x0,3ci1")
OTHER_METHODS = ("x0,7ci1", "1", "x0,2,4,0,3,20")                  # E8E9 in front of the BWT, LZ77

CHILD = r"""
import json, sys
import zpaq_amd as z
from zpaq_amd import corpus
z.init(0)
kinds = ["text", "lcg", "zeros", "records", "pattern"]
sizes = [150000, 1, 70001, 300, 131072, 4097, 99999, 65]
blocks = [corpus.block(kinds[i % 5], n, 900 + i) for i, n in enumerate(sizes)]
out = {}
for m in json.loads(sys.argv[1]):
    arch = z.compress_blocks([b.copy() for b in blocks], m)
    back = z.decompress(b"".join(arch))
    out[m] = [back == b"".join(b.tobytes() for b in blocks), z.last_device_unbwt_segments(), z.last_device_unlz_segments()]
z.shutdown()
print("RESULT " + json.dumps(out))
"""


def _child(env_changes, methods):
    env = dict(os.environ)
    for k in ("ZPAQ_AMD_DEVICE_UNBWT", "ZPAQ_AMD_DEVICE_UNLZ", "ZPAQ_AMD_PCOMP"):
        env.pop(k, None)
    env.update(env_changes)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", CHILD, json.dumps(list(methods))], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


@pytest.mark.parametrize("knob,count", [("1", 8), ("0", 0), (None, 0)])
def test_archives_round_trip_on_either_route(gpu, knob, count):
    """8 blocks of mixed kinds and lengths, one segment each: with the knob at 1 every BWT segment is decoded by the new kernels,
    with 0 none, unset none either (8 segments are below the floor of 64) -- and E8E9 and LZ77 methods never are.  The LZ77
    decoder's counter stays 0 for BWT archives.  The bytes are the inputs every time."""
    got = _child({} if knob is None else {"ZPAQ_AMD_DEVICE_UNBWT": knob}, BWT_METHODS + OTHER_METHODS)
    for m in BWT_METHODS:
        assert got[m] == [True, count, 0], (knob, m, got[m])
    for m in OTHER_METHODS:
        assert got[m][:2] == [True, 0], (knob, m, got[m])


@pytest.mark.parametrize("mode", ["device", "host"])
def test_a_forced_pcomp_route_keeps_its_meaning(gpu, mode):
    got = _child({"ZPAQ_AMD_PCOMP": mode, "ZPAQ_AMD_DEVICE_UNBWT": "1"}, BWT_METHODS)
    for m, res in got.items():
        assert res[:2] == [True, 0], (mode, m, res)
