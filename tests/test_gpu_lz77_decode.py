"""LZ77 streams decoded on the device (device/lz77_decode_kernel.h): zpq_lz77_decode_device against the blocks the streams were
made from and against the host's post-processor (zpq_postprocess_block), with guard bytes behind exact capacities, the overflow
and decline contracts, and archives through zpq_decompress with ZPAQ_AMD_DEVICE_UNLZ on and off, each in a fresh process."""
import json
import os
import random
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lz77_codes_cases as cc  # noqa: E402
import lz77_decode_cases as dc  # noqa: E402
import lz77_hash_cases as hc  # noqa: E402

from zpaq_amd import corpus  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xC3
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def batch():
    """Every kind at the 13 lengths of the host test, and one 1 MiB text block (many windows, many groups)."""
    return list(hc.inputs()) + [corpus.block("text", 1 << 20, 4321).tobytes()]


@pytest.fixture(scope="module")
def host_streams(batch):
    made = {}

    def get(xm):
        if xm not in made:
            made[xm] = [hc.preprocess(xm, d) for d in batch]
        return made[xm]
    return get


def _all_decoded(gpu, xm, streams, wants):
    rc, bufs, sizes, status = gpu.lz77_decode_device(xm, streams, [len(w) for w in wants], guard=GUARD, fill=FILL)
    assert rc == 0, (xm, gpu.lib().zpq_last_error().decode())
    assert status == [0] * len(streams), (xm, status)
    assert sizes == [len(w) for w in wants]
    for k, (b, w) in enumerate(zip(bufs, wants)):
        assert b[:len(w)] == w, (xm, k, len(w))
        assert b[len(w):] == bytes([FILL]) * GUARD, (xm, k, "a store past the capacity")


@pytest.mark.parametrize("xm", dc.METHODS)
def test_streams_decode_to_their_blocks(gpu, host_streams, xm):
    pairs = host_streams(xm)
    _all_decoded(gpu, xm, [s for s, _ in pairs], [seen for _, seen in pairs])


@pytest.mark.parametrize("xm", hc.FAR_METHODS)
def test_far_offsets(gpu, xm):
    stream, seen = hc.preprocess(xm, hc.far_repeat())
    _all_decoded(gpu, xm, [stream], [seen])


@pytest.mark.parametrize("xm", cc.METHODS)
def test_synthetic_and_random_lists_through_the_coder_and_back(gpu, xm):
    streams = [hc.serialize(xm, d, t) for _, d, t in cc.synthetic()]
    rng = random.Random(53)
    for _ in range(3):
        streams += [hc.serialize(xm, d, t) for d, t in cc.random_batch(rng) if all(n >= cc.MM for n in memoryview(t).cast("I")[2::4])]
    wants = []
    for s in streams:
        rc, w, _ = gpu.postprocess_block(xm, s)
        assert rc == 0
        wants.append(w)
    _all_decoded(gpu, xm, streams, wants)


@pytest.mark.parametrize("xm", cc.METHODS)
def test_a_buffer_too_small_reports_every_size(gpu, host_streams, xm):
    pairs = host_streams(xm)
    sizes_want = [len(seen) for _, seen in pairs]
    caps = list(sizes_want)
    short = max(range(len(caps)), key=lambda k: caps[k])
    caps[short] -= 1
    rc, bufs, sizes, status = gpu.lz77_decode_device(xm, [s for s, _ in pairs], caps, guard=GUARD, fill=FILL)
    assert rc == 3, (xm, rc)                                          # ZPQ_E_OVERFLOW
    assert sizes == sizes_want
    assert all(b == bytes([FILL]) * len(b) for b in bufs), (xm, "an overflowing batch wrote something")


@pytest.mark.parametrize("xm", cc.METHODS)
def test_handmade_and_damaged_streams_are_the_hosts_or_declined(gpu, xm):
    hand = [c for c in dc.handmade() if c[1] == xm]
    damaged, ncut = dc.damaged_batch(xm)
    streams = [c[2] for c in hand] + damaged
    host = [gpu.postprocess_block(xm, s) for s in streams]
    caps = [size for _, _, size in host]
    rc, bufs, sizes, status = gpu.lz77_decode_device(xm, streams, caps, guard=GUARD, fill=FILL)
    assert rc == 0, (xm, gpu.lib().zpq_last_error().decode())
    for k, (b, st) in enumerate(zip(bufs, status)):
        if st == 0:
            hrc, want, _ = host[k]
            assert hrc == 0 and sizes[k] == len(want) and b[:len(want)] == want, (xm, k, len(streams[k]))
            assert b[len(want):] == bytes([FILL]) * (len(b) - len(want)), (xm, k)
        else:
            assert st == 1 and b == bytes([FILL]) * len(b), (xm, k, "a declined stream's output was touched")
    for (name, _, _, declined), st in zip(hand, status):
        assert (st != 0) == declined, (xm, name, st)
    rest = status[len(hand):]
    assert rest[0] == 0 and rest[-1] == 0
    assert sum(1 for s in rest if s) <= len(damaged) - 2 - ncut


def test_a_capacity_one_byte_short_among_damaged_streams(gpu):
    xm = cc.METHODS[0]
    good = hc.preprocess(xm, hc.inputs()[30])
    bad = [c[2] for c in dc.handmade() if c[1] == xm and c[3]][0]
    rc, bufs, sizes, status = gpu.lz77_decode_device(xm, [good[0], bad, good[0]], [len(good[1]), 64, len(good[1]) - 1], guard=GUARD, fill=FILL)
    assert rc == 3 and sizes == [len(good[1]), 0, len(good[1])]
    assert all(b == bytes([FILL]) * len(b) for b in bufs)


# ---- archives: each setting in a fresh process ----
LZ_METHODS = ("1", "2", "x0,1,4,0,2,16", "x0,2,12,0,7,21,1c0,0,511", "x0,2,4,0,3,20c0,0,511")     # levels, a hash table, a suffix array, a model behind
OTHER_METHODS = ("x0,5,6,0,3,20", "x0,3ci1")                                                       # E8E9 in front, BWT

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
    out[m] = [back == b"".join(b.tobytes() for b in blocks), z.last_device_unlz_segments()]
z.shutdown()
print("RESULT " + json.dumps(out))
"""


def _child(env_changes, methods):
    env = dict(os.environ)
    for k in ("ZPAQ_AMD_DEVICE_UNLZ", "ZPAQ_AMD_PCOMP"):
        env.pop(k, None)
    env.update(env_changes)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", CHILD, json.dumps(list(methods))], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


@pytest.mark.parametrize("knob,count", [("1", 8), ("0", 0)])
def test_archives_round_trip_on_either_route(gpu, knob, count):
    """8 blocks of mixed kinds and lengths, one segment each: with the knob at 1 every LZ77 segment is decoded by the new
    kernels, with 0 none -- and E8E9 and BWT methods never are.  The bytes are the inputs either way."""
    got = _child({"ZPAQ_AMD_DEVICE_UNLZ": knob}, LZ_METHODS + OTHER_METHODS)
    for m in LZ_METHODS:
        assert got[m] == [True, count], (knob, m, got[m])
    for m in OTHER_METHODS:
        assert got[m] == [True, 0], (knob, m, got[m])


@pytest.mark.parametrize("mode", ["device", "host"])
def test_a_forced_pcomp_route_keeps_its_meaning(gpu, mode):
    got = _child({"ZPAQ_AMD_PCOMP": mode, "ZPAQ_AMD_DEVICE_UNLZ": "1"}, ("1", "x0,2,4,0,3,20c0,0,511"))
    for m, res in got.items():
        assert res == [True, 0], (mode, m, res)
