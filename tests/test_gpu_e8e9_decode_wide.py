"""Streams of the E8E9 forms of the LZ77 methods decoded on the device in pieces and filtered there
(device/lz77_decode_wide_kernel.h, device/e8e9_kernel.h): zpq_e8e9_decode_device_wide against the host's post-processor
(zpq_postprocess_block) over one ragged batch, at pieces of 4 096 and 16 384 bytes, with guard bytes behind exact capacities; a
capacity one byte short; other kinds of methods; and archives through zpq_decompress with ZPAQ_AMD_DEVICE_UNE8 and
ZPAQ_AMD_DEVICE_UNLZ_WIDE on, off and unset, each in a fresh process under its own time limit.  The give-up path of the filter's
walk is covered on the emulator only (tests/test_emu_e8e9_decode_wide.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import e8e9_cases as ec  # noqa: E402
import e8e9_wide_cases as e8w  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xA5
ROOT = os.path.dirname(HERE)
KNOBS = ("ZPAQ_AMD_DEVICE_UNE8", "ZPAQ_AMD_DEVICE_UNLZ_WIDE", "ZPAQ_AMD_UNLZ_WIDE_FROM", "ZPAQ_AMD_UNLZ_WIDE_PIECE", "ZPAQ_AMD_DEVICE_UNLZ",
         "ZPAQ_AMD_DEVICE_UNBWT", "ZPAQ_AMD_PCOMP")
PIECES = ("4096", "16384")
BOTH = {"ZPAQ_AMD_DEVICE_UNE8": "1", "ZPAQ_AMD_DEVICE_UNLZ_WIDE": "1"}
SMALL = {"ZPAQ_AMD_UNLZ_WIDE_FROM": "1", "ZPAQ_AMD_UNLZ_WIDE_PIECE": "4096"}


@pytest.fixture(scope="module")
def batch(gpu):
    """(streams, expected outputs) per method, made once: the expectation is the host's, and it is the block."""
    made = {}

    def get(xm):
        if xm not in made:
            made[xm] = (e8w.streams(xm), e8w.expected(xm))
            assert made[xm][1] == e8w.blocks(), xm
        return made[xm]
    return get


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("xm", e8w.METHODS)
def test_the_batch_decodes_to_what_the_host_makes_of_it(gpu, batch, monkeypatch, xm, piece):
    monkeypatch.setenv("ZPAQ_AMD_UNLZ_WIDE_PIECE", piece)
    streams, wants = batch(xm)
    rc, bufs, sizes, status = gpu.e8e9_decode_device_wide(xm, streams, [len(w) for w in wants], guard=GUARD, fill=FILL)
    assert rc == 0, (xm, gpu.lib().zpq_last_error().decode())
    assert status == [0] * len(streams), (xm, status)
    assert sizes == [len(w) for w in wants]
    for k, (b, w) in enumerate(zip(bufs, wants)):
        assert b[:len(w)] == w, (xm, k, len(w))
        assert b[len(w):] == bytes([FILL]) * GUARD, (xm, k, "a store past the capacity")
    assert gpu.last_unlz_wide_pieces()[0] >= len(streams)


@pytest.mark.parametrize("xm", e8w.METHODS)
def test_a_buffer_too_small_reports_every_size(gpu, batch, monkeypatch, xm):
    monkeypatch.setenv("ZPAQ_AMD_UNLZ_WIDE_PIECE", "4096")
    streams, wants = batch(xm)
    sizes_want = [len(w) for w in wants]
    caps = list(sizes_want)
    short = max(range(len(caps)), key=lambda k: caps[k])
    caps[short] -= 1
    rc, bufs, sizes, status = gpu.e8e9_decode_device_wide(xm, streams, caps, guard=GUARD, fill=FILL)
    assert rc == 3, (xm, rc)                                          # ZPQ_E_OVERFLOW
    assert sizes == sizes_want
    assert all(b == bytes([FILL]) * len(b) for b in bufs), (xm, "an overflowing batch wrote something")


@pytest.mark.parametrize("other", ("x0,1,4,0,3,20", "x0,4", "x0,7", "x5,7", "x0,0"))
def test_other_kinds_of_methods_are_unsupported(gpu, other):
    rc, bufs, _, _ = gpu.e8e9_decode_device_wide(other, [b"\0" * 8], [16], guard=GUARD, fill=FILL)
    assert rc == 8, (other, rc)                                       # ZPQ_E_UNSUPPORTED
    assert b"unavailable" in gpu.lib().zpq_last_error(), other
    assert bufs[0] == bytes([FILL]) * len(bufs[0])


# ---- archives: each setting in a fresh process ----
E8_METHODS = ("x0,5,6,0,3,20", "x0,6,4,0,3,20")
BIG_METHOD, BIG_BYTES = "x5,5,4,0,3,24", (1 << 24) + 4097

# (the sizes and kinds of tests/test_gpu_lz77_decode_wide.py's CHILD; blocks 0 and 4 are x86-like bytes)
CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[2])
import numpy as np
import zpaq_amd as z
from zpaq_amd import corpus
import e8e9_cases as ec
z.init(0)
kinds = ["text", "lcg", "zeros", "records", "pattern"]
sizes = [150000, 1, 70001, 300, 131072, 4097, 99999, 65]
blocks = [corpus.block(kinds[i % 5], n, 900 + i) for i, n in enumerate(sizes)]
for i in (0, 4):
    blocks[i] = np.frombuffer(ec.x86_like(sizes[i], 40 + i), np.uint8).copy()
out = {}
for m in json.loads(sys.argv[1]):
    arch = z.compress_blocks([b.copy() for b in blocks], m)
    back = z.decompress(b"".join(arch))
    out[m] = [back == b"".join(b.tobytes() for b in blocks), z.last_device_une8_wide_segments(), z.last_device_une8_segments(),
              z.last_device_unlz_wide_segments(), z.last_device_unlz_segments()]
z.shutdown()
print("RESULT " + json.dumps(out))
"""

CHILD_BIG = r"""
import json, sys
import zpaq_amd as z
z.init(0)
arch = open(sys.argv[1], "rb").read()
want = open(sys.argv[2], "rb").read()
back = z.decompress(arch)
out = [back == want, z.last_device_une8_wide_segments(), list(z.last_unlz_wide_pieces())]
z.shutdown()
print("RESULT " + json.dumps(out))
"""


def _child(code, env_changes, args, limit):
    env = dict(os.environ)
    for k in KNOBS:
        env.pop(k, None)
    env.update(env_changes)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code, *args], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    assert r.returncode == 0, r.stdout[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def _archives(env, methods=E8_METHODS):
    return _child(CHILD, env, [json.dumps(list(methods)), HERE], 240)


def test_both_knobs_send_every_segment_through_the_new_route(gpu):
    for m, res in _archives({**BOTH, **SMALL}).items():
        assert res == [True, 8, 0, 0, 0], (m, res)


def test_une8_alone_is_the_route_it_was(gpu):
    for m, res in _archives({"ZPAQ_AMD_DEVICE_UNE8": "1", **SMALL}).items():
        assert res == [True, 0, 8, 0, 0], (m, res)


def test_unlz_wide_alone_never_touches_an_e8e9_group(gpu):
    for m, res in _archives({"ZPAQ_AMD_DEVICE_UNLZ_WIDE": "1", **SMALL}).items():
        assert res == [True, 0, 0, 0, 0], (m, res)


def test_nothing_set_changes_nothing(gpu):
    for m, res in _archives({}).items():
        assert res[:2] == [True, 0], (m, res)


@pytest.mark.parametrize("mode", ["device", "host"])
def test_a_forced_pcomp_route_keeps_its_meaning(gpu, mode):
    for m, res in _archives({**BOTH, **SMALL, "ZPAQ_AMD_PCOMP": mode}).items():
        assert res[:2] == [True, 0], (mode, m, res)


def test_streams_below_the_threshold_stay_in_their_group(gpu):
    """The default threshold of 1 MiB: none of the eight blocks qualifies, and today's route takes the whole group."""
    for m, res in _archives({**BOTH, "ZPAQ_AMD_UNLZ_WIDE_PIECE": "4096"}).items():
        assert res == [True, 0, 8, 0, 0], (m, res)


def test_methods_beside_the_route_go_where_they_went(gpu):
    got = _archives({**BOTH, **SMALL}, ("x0,1,4,0,3,20", "x0,4", "x0,7"))
    ok, e8wide, e8, lzwide, _ = got["x0,1,4,0,3,20"]
    assert ok and e8wide == 0 and e8 == 0 and lzwide == 8, got
    for m in ("x0,4", "x0,7"):
        ok, e8wide, e8, lzwide, _ = got[m]
        assert ok and e8wide == 0 and e8 == 8 and lzwide == 0, (m, got[m])


@pytest.fixture(scope="module")
def big_archive(gpu, tmp_path_factory):
    """One block of 2^24 + 4 097 bytes: 17 copies of 1 MiB of x86-like bytes (the generator is a Python loop), cut to length.  Some
    e8 / e9 with a 00 / ff four bytes behind it lies at a position of 2^24 and more: the subtraction mod 2^24 wraps."""
    d = tmp_path_factory.mktemp("une8_wide")
    unit = np.frombuffer(ec.x86_like(1 << 20, 77), np.uint8)
    b = np.tile(unit, 17)[:BIG_BYTES].copy()
    tail = b[1 << 24:]
    hit = ((tail[:-4] & 254) == 0xe8) & ((tail[4:] == 0) | (tail[4:] == 255))
    assert hit.any(), "no opcode at a position of 2^24 and more"
    arch = gpu.compress_blocks([b.copy()], BIG_METHOD)
    (d / "arch").write_bytes(b"".join(arch))
    (d / "data").write_bytes(b.tobytes())
    return str(d / "arch"), str(d / "data")


@pytest.mark.parametrize("knob,count", [("1", 1), ("0", 0)])
def test_a_block_of_sixteen_mebibytes_and_more(gpu, big_archive, knob, count):
    ok, segments, pieces = _child(CHILD_BIG, {"ZPAQ_AMD_DEVICE_UNE8": knob, "ZPAQ_AMD_DEVICE_UNLZ_WIDE": knob}, list(big_archive), 300)
    assert ok and segments == count, (knob, ok, segments, pieces)
    if count:
        assert pieces[0] >= 64, pieces
