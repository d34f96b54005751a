"""Streams of the E8E9 methods decoded on the device (the stage's decoder, then device/e8e9_kernel.h):
zpq_e8e9_decode_device against the blocks the streams were made from and against the host's post-processor
(zpq_postprocess_block), with guard bytes behind exact capacities, the overflow and decline contracts, and archives through
zpq_decompress with ZPAQ_AMD_DEVICE_UNE8 on, off and unset, each in a fresh process."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import e8e9_cases as ec  # noqa: E402
import lz77_decode_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xC3
ROOT = os.path.dirname(HERE)


def _all_decoded(gpu, xm, streams, wants):
    rc, bufs, sizes, status = gpu.e8e9_decode_device(xm, streams, [len(w) for w in wants], guard=GUARD, fill=FILL)
    assert rc == 0, (xm, gpu.lib().zpq_last_error().decode())
    assert status == [0] * len(streams), (xm, status)
    assert sizes == [len(w) for w in wants]
    for k, (b, w) in enumerate(zip(bufs, wants)):
        assert b[:len(w)] == w, (xm, k, len(w))
        assert b[len(w):] == bytes([FILL]) * GUARD, (xm, k, "a store past the capacity")


@pytest.mark.parametrize("xm", ec.METHODS)
def test_streams_decode_to_their_blocks(gpu, xm):
    bl = ec.blocks()
    streams = [ec.stream_of(xm, b) for b in bl]
    for k, (s, b) in enumerate(zip(streams, bl)):
        rc, want, _ = gpu.postprocess_block(xm, s)
        assert rc == 0 and want == b, (xm, k, len(b))
    _all_decoded(gpu, xm, streams, list(bl))


@pytest.mark.parametrize("xm", ["x0,4", "x1,5,6,0,3,21"])
def test_a_chain_of_a_mebibyte_is_skipped_through(gpu, xm):
    """e8, zeros, one e9 in the middle: a single chain of 2^20 candidates with two seeds.  The walk jumps from one to the other."""
    b = ec.skipping_block()
    s = ec.stream_of(xm, b)
    rc, want, _ = gpu.postprocess_block(xm, s)
    assert rc == 0 and want == b
    _all_decoded(gpu, xm, [s], [b])


@pytest.mark.parametrize("xm", ec.METHODS[:4])
def test_a_buffer_too_small_reports_every_size(gpu, xm):
    bl = [b for b in ec.blocks() if len(b) >= 64][:12]
    streams = [ec.stream_of(xm, b) for b in bl]
    caps = [len(b) for b in bl]
    short = max(range(len(caps)), key=lambda k: caps[k])
    caps[short] -= 1
    rc, bufs, sizes, status = gpu.e8e9_decode_device(xm, streams, caps, guard=GUARD, fill=FILL)
    assert rc == 3, rc                                                # ZPQ_E_OVERFLOW
    assert sizes == [len(b) for b in bl]
    assert all(b == bytes([FILL]) * len(b) for b in bufs), "an overflowing batch wrote something"


def test_what_the_stage_in_front_declines_stays_declined(gpu):
    """A match that reaches in front of the output's start: the LZ77 decoder declines it, so does this route -- beside good
    streams, which decode."""
    xm = dc.E8E9
    bad = [dc.encode(xm, [("match", 5, 1), dc._lit(3, 340)]), dc.encode(xm, [dc._lit(3, 341), ("match", 5, 4)])]
    good = [b for b in ec.blocks() if len(b) >= 64][:3]
    streams = [ec.stream_of(xm, good[0]), bad[0], ec.stream_of(xm, good[1]), bad[1], ec.stream_of(xm, good[2])]
    caps = [len(good[0]), 64, len(good[1]), 64, len(good[2])]
    rc, bufs, sizes, status = gpu.e8e9_decode_device(xm, streams, caps, guard=GUARD, fill=FILL)
    assert rc == 0, gpu.lib().zpq_last_error().decode()
    assert status == [0, 1, 0, 1, 0] and sizes == [len(good[0]), 0, len(good[1]), 0, len(good[2])]
    for k in (1, 3):
        assert bufs[k] == bytes([FILL]) * len(bufs[k]), (k, "a declined stream's output was touched")
    for k, g in zip((0, 2, 4), good):
        assert bufs[k] == g + bytes([FILL]) * GUARD, k


# ---- archives: each setting in a fresh process ----
OTHER_METHODS = ("1", "x0,3", "x0,2,4,0,3,20")

CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[2], "tests"))
import numpy as np
import e8e9_cases as ec
import zpaq_amd as z
from zpaq_amd import corpus
z.init(0)
blocks = [np.frombuffer(ec.x86_like(150000, 31), np.uint8), corpus.block("text", 1, 901), np.frombuffer(ec.x86_like(70001, 32), np.uint8),
          corpus.block("records", 300, 903), np.frombuffer(ec.x86_like(131072, 33), np.uint8), corpus.block("zeros", 4097, 905),
          np.frombuffer(ec.ADVERSARIAL, np.uint8), corpus.block("pattern", 65, 907)]
out = {}
for m in json.loads(sys.argv[1]):
    arch = z.compress_blocks([b.copy() for b in blocks], m)
    back = z.decompress(b"".join(arch))
    out[m] = [back == b"".join(b.tobytes() for b in blocks), z.last_device_une8_segments(), z.last_device_unlz_segments(), z.last_device_unbwt_segments()]
z.shutdown()
print("RESULT " + json.dumps(out))
"""


def _child(env_changes, methods):
    env = dict(os.environ)
    for k in ("ZPAQ_AMD_DEVICE_UNE8", "ZPAQ_AMD_DEVICE_UNBWT", "ZPAQ_AMD_DEVICE_UNLZ", "ZPAQ_AMD_PCOMP"):
        env.pop(k, None)
    env.update(env_changes)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", CHILD, json.dumps(list(methods)), ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


@pytest.mark.parametrize("knob,count", [("1", 8), ("0", 0), (None, 0)])
def test_archives_round_trip_on_either_route(gpu, knob, count):
    """8 blocks, x86-like ones among them, one segment each: with the knob at 1 every segment of the five E8E9 methods goes
    through the new route, with 0 none, unset none either (no measurement has set a group size yet) -- and methods without the
    filter never do.  The LZ77 and BWT decoders' counters stay 0 for E8E9 archives.  The bytes are the inputs every time."""
    got = _child({} if knob is None else {"ZPAQ_AMD_DEVICE_UNE8": knob}, ec.METHODS + OTHER_METHODS)
    for m in ec.METHODS:
        assert got[m] == [True, count, 0, 0], (knob, m, got[m])
    for m in OTHER_METHODS:
        assert got[m][:2] == [True, 0], (knob, m, got[m])


@pytest.mark.parametrize("mode", ["device", "host"])
def test_a_forced_pcomp_route_keeps_its_meaning(gpu, mode):
    got = _child({"ZPAQ_AMD_PCOMP": mode, "ZPAQ_AMD_DEVICE_UNE8": "1"}, ec.METHODS)
    for m, res in got.items():
        assert res[:2] == [True, 0], (mode, m, res)
