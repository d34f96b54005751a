"""BWT streams of the program at args[0] 5 .. 11 decoded on the device (device/bwt_decode_wide_kernel.h):
zpq_bwt_decode_device_wide against the blocks the streams were made from and against the host's post-processor, with guard bytes
behind exact capacities; one block beyond the small decoder's 24-bit word, alone and between small ones; and archives through
zpq_decompress with ZPAQ_AMD_DEVICE_UNBWT / ZPAQ_AMD_DEVICE_UNE8 on, off and unset, each in a fresh process."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bwt_decode_cases as bc  # noqa: E402
import bwt_decode_wide_cases as wc  # noqa: E402
import e8e9_cases as ec  # noqa: E402

from zpaq_amd import corpus  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xC3
ROOT = os.path.dirname(HERE)
LARGE = (1 << 24) + 4097                     # the smallest block the 24-bit word cannot hold, and a tile more
UNSUPPORTED, OVERFLOW = 8, 3


def _decode(gpu, xm, streams, caps):
    rc, bufs, sizes, status = gpu.bwt_decode_device_wide(xm, streams, caps, guard=GUARD, fill=FILL)
    assert rc == 0, (xm, gpu.lib().zpq_last_error().decode())
    return bufs, sizes, status


def _all_decoded(gpu, xm, streams, wants):
    bufs, sizes, status = _decode(gpu, xm, streams, [len(w) for w in wants])
    assert status == [0] * len(streams), (xm, status)
    assert sizes == [len(w) for w in wants]
    for k, (b, w) in enumerate(zip(bufs, wants)):
        assert b[:len(w)] == w, (xm, k, len(w))
        assert b[len(w):] == bytes([FILL]) * GUARD, (xm, k, "a store past the capacity")


def test_valid_streams_decode_to_their_blocks(gpu):
    pairs = wc.valid_streams()
    _all_decoded(gpu, wc.METHOD, [s for s, _ in pairs], [d for _, d in pairs])


def test_streams_under_the_rule(gpu):
    """A whole path is decoded to the model's bytes (the host's program: tests/test_emu_bwt_decode_wide.py), a shorter one is
    declined and its output untouched."""
    streams = bc.rule_streams()
    bufs, sizes, status = _decode(gpu, wc.METHOD, [s for s, _ in streams], [len(s) - 5 for s, _ in streams])
    for k, ((s, m), b, st) in enumerate(zip(streams, bufs, status)):
        if len(m) == len(s) - 5:
            assert st == 0 and sizes[k] == len(m) and b[:len(m)] == m, (k, s.hex())
            assert b[len(m):] == bytes([FILL]) * GUARD, k
        else:
            assert st == 1 and sizes[k] == 0 and b == bytes([FILL]) * len(b), (k, "a declined stream's output was touched")
    for k in wc.rule_sample()[:5]:
        assert gpu.postprocess_block(wc.METHOD, streams[k][0])[:2] == (0, streams[k][1]), k


def test_streams_outside_the_rule_are_declined(gpu):
    streams = bc.outside_batch()
    bufs, sizes, status = _decode(gpu, wc.METHOD, streams, [max(len(s) - 5, 0) for s in streams])
    assert status[0] == 0 and status[-1] == 0
    for k, (s, b, st) in enumerate(zip(streams, bufs, status)):
        m = bc.model(s)
        if m is not None and len(m) == len(s) - 5:
            assert st == 0 and sizes[k] == len(m) and b[:len(m)] == m, (k, s.hex())
            assert b[len(m):] == bytes([FILL]) * (len(b) - len(m)), k
        else:
            assert st == 1 and sizes[k] == 0 and b == bytes([FILL]) * len(b), (k, s.hex())


def test_a_buffer_too_small_reports_every_size(gpu):
    pairs = wc.valid_streams()
    sizes_want = [len(d) for _, d in pairs]
    caps = list(sizes_want)
    caps[max(range(len(caps)), key=lambda k: caps[k])] -= 1
    rc, bufs, sizes, status = gpu.bwt_decode_device_wide(wc.METHOD, [s for s, _ in pairs], caps, guard=GUARD, fill=FILL)
    assert rc == OVERFLOW and sizes == sizes_want
    assert all(b == bytes([FILL]) * len(b) for b in bufs), "an overflowing batch wrote something"


def test_the_e8e9_blocks_behind_the_wide_stage(gpu):
    """x5,7: the inverse filter over the stage's output on the device gives the blocks, which is what the method's own windowed
    program makes of the streams (tests/test_emu_bwt_decode_wide.py runs it over every one of them)."""
    blocks = [d for d in ec.blocks()]
    streams = [ec.stream_of(wc.E8_METHOD, d) for d in blocks]
    _all_decoded(gpu, wc.E8_METHOD, streams, blocks)
    for k in (25, len(blocks) - 2):
        assert gpu.postprocess_block(wc.E8_METHOD, streams[k])[:2] == (0, blocks[k]), k


def test_the_top_of_the_range(gpu):
    """x11,3: mbits 31.  The device's arrays are sized by the stream, not by the program's 2^31."""
    pairs = wc.valid_streams()[20:30]
    _all_decoded(gpu, "x11,3", [s for s, _ in pairs], [d for _, d in pairs])


@pytest.fixture(scope="module")
def large(gpu):
    """2^24 + 4 097 bytes of text and their stream, from the device's wide sorter (tests/test_gpu_sort_wide.py tests it)."""
    d = corpus.block("text", LARGE, 777)
    rc, out, size = gpu.preprocess_block_device_wide(wc.METHOD, d.copy(), LARGE + 5)
    assert rc == 0 and size == LARGE + 5, gpu.lib().zpq_last_error().decode()
    return out[:size], d.tobytes()


def test_one_large_block(gpu, large):
    s, d = large
    _all_decoded(gpu, wc.METHOD, [s], [d])
    # the small decoder declines it: n >= 2^24
    rc, bufs, sizes, status = gpu.bwt_decode_device("x4,3", [s], [len(d)], guard=GUARD, fill=FILL)
    assert rc == 0 and status == [1] and sizes == [0]


def test_the_host_program_over_the_large_block(gpu, large):
    s, d = large
    rc, want, _ = gpu.postprocess_block(wc.METHOD, s)
    assert rc == 0 and want == d


def test_a_run_of_zeros_beyond_the_24_bit_word(gpu):
    """2^24 + 1 zeros: the stream is written down without a sort, and the list is sequential."""
    n = (1 << 24) + 1
    _all_decoded(gpu, wc.METHOD, [wc.zeros_stream(n)], [bytes(n)])


def test_the_large_block_between_two_small_ones(gpu, large):
    s, d = large
    a, b = wc.valid_streams()[30], wc.level2_streams()[5]
    assert len(a[1]) > 0 and len(b[1]) > 0
    _all_decoded(gpu, wc.METHOD, [a[0], s, b[0]], [a[1], d, b[1]])


def test_a_budget_below_the_large_blocks_workspace(gpu, large):
    """128 MiB hold less than the block's 8 bytes of list per byte: declined with a note before anything is launched, the output
    untouched; two small streams beside it are decoded in the sub-batches around it."""
    s, d = large
    a, b = wc.valid_streams()[30], wc.level2_streams()[5]
    gpu.set_state_budget(128 << 20)
    try:
        rc, bufs, sizes, status = gpu.bwt_decode_device_wide(wc.METHOD, [s], [len(d)], guard=GUARD, fill=FILL)
        note = gpu.lib().zpq_last_error().decode()
        mixed = gpu.bwt_decode_device_wide(wc.METHOD, [a[0], s, b[0]], [len(a[1]), len(d), len(b[1])], guard=GUARD, fill=FILL)
    finally:
        gpu.set_state_budget(0)
    assert rc == UNSUPPORTED and "budget" in note, (rc, note)
    assert sizes == [0] and bufs[0] == bytes([FILL]) * len(bufs[0])
    rc, bufs, sizes, status = mixed
    assert rc == 0 and status == [0, 1, 0] and sizes == [len(a[1]), 0, len(b[1])]
    assert bufs[0][:len(a[1])] == a[1] and bufs[2][:len(b[1])] == b[1] and bufs[1] == bytes([FILL]) * len(bufs[1])


# ---- archives: each setting in a fresh process ----
SIZES = (70001, 33333, 100003, 4097, 65537, 12345)                # tests/test_gpu_sort_wide.py SMALL_SIZES
WIDE_BWT = ("x5,3", "x6,3", "x11,3")
WIDE_E8 = ("x5,7",)
# The routes an archive had before refuse x11,3 outright -- host/postproc.cpp at ph > 28, engine_pcomp at such arrays -- so the
# six blocks go through them with the methods they can decode; test_x11_in_every_setting runs x11,3 through each of them.
OLD_ROUTE = ("x5,3", "x6,3", "x5,7")
BESIDE = ("x0,3", "1")

CHILD = r"""
import json, sys
import zpaq_amd as z
from zpaq_amd import corpus
spec = json.loads(sys.argv[1])
z.init(0)
if spec.get("large"):
    blocks = [corpus.block(spec.get("kind", "text"), spec["large"], 777)]
else:
    blocks = [corpus.block("text" if i % 2 == 0 else "records", n, 500 + i) for i, n in enumerate(spec["sizes"])]
want = b"".join(b.tobytes() for b in blocks)
out = {}
for m in spec["methods"]:
    arch = z.compress_blocks([b.copy() for b in blocks], m)
    if spec.get("budget"):
        z.set_state_budget(spec["budget"])
    try:
        back = z.decompress(b"".join(arch), cap=len(want) + 64)
    except z.ZpaqError as e:
        if not spec.get("errors"):
            raise
        out[m] = ["error", str(e)]
        continue
    finally:
        z.set_state_budget(0)
    out[m] = [back == want, z.last_device_unbwt_segments(), z.last_device_une8_segments(), z.last_device_unlz_segments()]
z.shutdown()
print("RESULT " + json.dumps(out))
"""


def _child(env_changes, spec):
    env = dict(os.environ)
    for k in ("ZPAQ_AMD_DEVICE_UNBWT", "ZPAQ_AMD_DEVICE_UNE8", "ZPAQ_AMD_DEVICE_UNLZ", "ZPAQ_AMD_PCOMP", "ZPAQ_AMD_DEVICE_SORT_WIDE",
              "ZPAQ_AMD_SORT_WIDE_FROM"):
        env.pop(k, None)
    env.update(env_changes)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", CHILD, json.dumps(spec)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def _pays(stream_bytes):
    """bwt_unbwt_wide_pays (device/engine.hpp): on from the smallest group measured, 2^24 + 4 097 bytes."""
    return stream_bytes >= (1 << 24) + 4097


def test_archives_with_the_knobs_at_1(gpu):
    """Six ragged blocks, one segment each: every segment of a wide program is decoded by the new kernels and counted -- x.,3 by
    ZPAQ_AMD_DEVICE_UNBWT's counter, x.,7 by ZPAQ_AMD_DEVICE_UNE8's -- and x0,3 and method 1 beside them are as they were."""
    got = _child({"ZPAQ_AMD_DEVICE_UNBWT": "1", "ZPAQ_AMD_DEVICE_UNE8": "1"}, {"sizes": SIZES, "methods": WIDE_BWT + WIDE_E8 + BESIDE})
    for m in WIDE_BWT:
        assert got[m] == [True, len(SIZES), 0, 0], (m, got[m])
    for m in WIDE_E8:
        assert got[m] == [True, 0, len(SIZES), 0], (m, got[m])
    assert got["x0,3"] == [True, len(SIZES), 0, 0] and got["1"] == [True, 0, 0, 0], got


@pytest.mark.parametrize("knob", ["0", None])
def test_archives_with_the_knobs_at_0_or_unset(gpu, knob):
    env = {} if knob is None else {"ZPAQ_AMD_DEVICE_UNBWT": knob, "ZPAQ_AMD_DEVICE_UNE8": knob}
    got = _child(env, {"sizes": SIZES, "methods": OLD_ROUTE + BESIDE})
    count = len(SIZES) if knob is None and _pays(sum(SIZES) + 5 * len(SIZES)) else 0
    assert count == 0
    for m in OLD_ROUTE + BESIDE:
        assert got[m] == [True, count if m.endswith(",3") and m != "x0,3" else 0, count if m.endswith(",7") else 0, 0], (knob, m, got[m])


@pytest.mark.parametrize("mode", ["device", "host"])
def test_a_forced_pcomp_route_keeps_its_meaning(gpu, mode):
    got = _child({"ZPAQ_AMD_PCOMP": mode, "ZPAQ_AMD_DEVICE_UNBWT": "1", "ZPAQ_AMD_DEVICE_UNE8": "1"}, {"sizes": SIZES, "methods": OLD_ROUTE})
    for m, res in got.items():
        assert res == [True, 0, 0, 0], (mode, m, res)


@pytest.mark.parametrize("knob", ["1", None])
def test_the_large_block_through_decompress(gpu, knob):
    """With the knob at 1, and unset, where bwt_unbwt_wide_pays takes a group of this size -- never at 0: the routes the archive
    had before need 2 to 18 seconds for it."""
    assert _pays(LARGE + 5)
    env = {"ZPAQ_AMD_DEVICE_SORT_WIDE": "1"}
    if knob is not None:
        env["ZPAQ_AMD_DEVICE_UNBWT"] = knob
    got = _child(env, {"large": LARGE, "methods": ["x5,3"]})
    assert got["x5,3"] == [True, 1, 0, 0], got


def test_an_archive_under_a_budget_below_its_workspace(gpu):
    """1 MiB: every block is declined before any launch, the call succeeds by the route it had, and the counter is 0."""
    got = _child({"ZPAQ_AMD_DEVICE_UNBWT": "1"}, {"sizes": SIZES, "methods": ["x5,3"], "budget": 1 << 20})
    assert got["x5,3"] == [True, 0, 0, 0], got


X11_SETTINGS = (
    ({"ZPAQ_AMD_DEVICE_UNBWT": "1"}, None),
    ({"ZPAQ_AMD_DEVICE_UNBWT": "0"}, "NOMEM"),
    ({}, "NOMEM"),
    ({"ZPAQ_AMD_PCOMP": "host", "ZPAQ_AMD_DEVICE_UNBWT": "1"}, "NOMEM"),
    ({"ZPAQ_AMD_PCOMP": "device", "ZPAQ_AMD_DEVICE_UNBWT": "1"}, "UNSUPPORTED"),
)


@pytest.mark.parametrize("env,error", X11_SETTINGS)
def test_x11_in_every_setting(gpu, env, error):
    """One block with x11,3 (ph = pm = 31).  The routes an archive had before cannot decode it at all: the host's post-processor
    refuses ph > 28 ("Out of memory") and the one-lane kernel's arrays are too large -- so with the knob at 0, unset (4 097 bytes
    lie below bwt_unbwt_wide_pays) and under ZPAQ_AMD_PCOMP the call fails as it did, and with the knob at 1 it now decodes."""
    got = _child(env, {"sizes": SIZES[3:4], "methods": ["x11,3"], "errors": True})["x11,3"]
    if error is None:
        assert got == [True, 1, 0, 0], got
    else:
        assert got[0] == "error" and error in got[1], (env, got)


def test_a_large_e8e9_block(gpu):
    """2^24 + 4 097 LCG bytes (e8 / e9 with 00 / ff four bytes on about every 8 000th position) with x5,7: through the stage against
    the block, and through zpq_decompress with ZPAQ_AMD_DEVICE_UNE8=1 -- counted there, while unset it is not: no x.,7 group has
    been timed (bwt_une8_wide_pays)."""
    d = corpus.block("lcg", LARGE, 777)
    seen = d.copy()
    rc, out, size = gpu.preprocess_block_device_wide(wc.E8_METHOD, seen, LARGE + 5)
    assert rc == 0 and size == LARGE + 5, gpu.lib().zpq_last_error().decode()
    assert (seen != d).any(), "the block holds nothing for the filter"
    _all_decoded(gpu, wc.E8_METHOD, [out[:size]], [d.tobytes()])
    got = _child({"ZPAQ_AMD_DEVICE_UNE8": "1", "ZPAQ_AMD_DEVICE_SORT_WIDE": "1"}, {"large": LARGE, "kind": "lcg", "methods": ["x5,7"]})
    assert got["x5,7"] == [True, 0, 1, 0], got
