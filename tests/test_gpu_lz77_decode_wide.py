"""LZ77 streams decoded on the device in pieces (device/lz77_decode_wide_kernel.h): zpq_lz77_decode_device_wide against the blocks
the streams were made from and against the host's post-processor (zpq_postprocess_block), at pieces of 4 096 bytes and at the
default, with guard bytes behind exact capacities; the statuses of zpq_lz77_decode_device on hand-made and damaged streams; and
archives through zpq_decompress with ZPAQ_AMD_DEVICE_UNLZ_WIDE on, off and unset, each in a fresh process under its own time
limit."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lz77_codes_cases as cc  # noqa: E402
import lz77_decode_cases as dc  # noqa: E402
import lz77_decode_wide_cases as wc  # noqa: E402
import lz77_hash_cases as hc  # noqa: E402

from zpaq_amd import corpus  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xC3
ROOT = os.path.dirname(HERE)
KNOBS = ("ZPAQ_AMD_DEVICE_UNLZ_WIDE", "ZPAQ_AMD_UNLZ_WIDE_FROM", "ZPAQ_AMD_UNLZ_WIDE_PIECE", "ZPAQ_AMD_DEVICE_UNLZ", "ZPAQ_AMD_PCOMP")
PIECES = ("4096", None)                      # None: the default


def _piece(monkeypatch, piece):
    if piece is None:
        monkeypatch.delenv("ZPAQ_AMD_UNLZ_WIDE_PIECE", raising=False)
    else:
        monkeypatch.setenv("ZPAQ_AMD_UNLZ_WIDE_PIECE", piece)


@pytest.fixture(scope="module")
def batch():
    """Every kind at the 13 lengths of the host test, and one 1 MiB text block (hundreds of pieces of 4 096 bytes)."""
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
    rc, bufs, sizes, status = gpu.lz77_decode_device_wide(xm, streams, [len(w) for w in wants], guard=GUARD, fill=FILL)
    assert rc == 0, (xm, gpu.lib().zpq_last_error().decode())
    assert status == [0] * len(streams), (xm, status)
    assert sizes == [len(w) for w in wants]
    for k, (b, w) in enumerate(zip(bufs, wants)):
        assert b[:len(w)] == w, (xm, k, len(w))
        assert b[len(w):] == bytes([FILL]) * GUARD, (xm, k, "a store past the capacity")


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("xm", dc.METHODS)
def test_streams_decode_to_their_blocks(gpu, host_streams, monkeypatch, xm, piece):
    _piece(monkeypatch, piece)
    pairs = host_streams(xm)
    _all_decoded(gpu, xm, [s for s, _ in pairs], [seen for _, seen in pairs])
    pieces = gpu.last_unlz_wide_pieces()
    want = int(piece) if piece else 16384
    assert pieces[0] == sum((len(s) + want - 1) // want for s, _ in pairs) and sum(pieces[1:]) <= pieces[0]
    assert 1 <= gpu.last_unlz_wide_rounds() <= 32


@pytest.mark.parametrize("xm", (dc.L1, dc.RB))
def test_text_always_meets_within_a_piece(gpu, monkeypatch, xm):
    """1 MiB of text at level 1 in pieces of 4 096 bytes: every piece is entered (no code of text leaps over one) and every
    piece's list is met inside the piece -- none is walked serially to its end."""
    _piece(monkeypatch, "4096")
    data = corpus.block("text", 1 << 20, 4321).tobytes()
    stream, seen = hc.preprocess(xm, data)
    _all_decoded(gpu, xm, [stream], [seen])
    pieces = gpu.last_unlz_wide_pieces()
    assert pieces[0] >= 64 and sum(pieces[1:]) == pieces[0] and pieces[3] == 0, pieces


@pytest.mark.parametrize("piece", ("64", "256"))
def test_handmade_streams_of_the_wide_decoder(gpu, monkeypatch, piece):
    """The seams, the leap, the late meet, the chain, the runs and the deferred checks of lz77_decode_wide_cases, as one batch
    per method."""
    _piece(monkeypatch, piece)
    for xm in wc.METHODS:
        named = [(c[0], c[3], False) for c in wc.seams() if c[1] == xm and c[2] == int(piece)]
        named += [(c[0], c[2], False) for c in wc.long_literals() if c[1] == xm]
        named += [("chain", wc.chain(xm), False), ("runs", wc.runs(xm), False)]
        named += [(c[0], c[2], c[3]) for c in wc.deferred(64) if c[1] == xm]
        if xm == wc.late_meet()[0]:
            named.append(("late meet", wc.late_meet()[1], False))
        streams = [s for _, s, _ in named]
        host = [gpu.postprocess_block(xm, s) for s in streams]
        rc, bufs, sizes, status = gpu.lz77_decode_device_wide(xm, streams, [size for _, _, size in host], guard=GUARD, fill=FILL)
        assert rc == 0, (xm, gpu.lib().zpq_last_error().decode())
        for k, ((name, _, declined), b, st) in enumerate(zip(named, bufs, status)):
            assert st == (1 if declined else 0), (xm, name, st)
            if st == 0:
                hrc, want, _ = host[k]
                assert hrc == 0 and sizes[k] == len(want) and b[:len(want)] == want, (xm, name)
                assert b[len(want):] == bytes([FILL]) * (len(b) - len(want)), (xm, name)
            else:
                assert b == bytes([FILL]) * len(b), (xm, name, "a declined stream's output was touched")


def test_a_chain_of_a_thousand_matches_takes_ten_rounds(gpu, monkeypatch):
    _piece(monkeypatch, "256")
    for xm in wc.METHODS:
        stream = wc.chain(xm)
        _, want, size = gpu.postprocess_block(xm, stream)
        rc, bufs, sizes, status = gpu.lz77_decode_device_wide(xm, [stream], [size], guard=GUARD, fill=FILL)
        assert rc == 0 and status == [0] and bufs[0][:size] == want
        assert gpu.last_unlz_wide_rounds() <= 11, (xm, gpu.last_unlz_wide_rounds())


@pytest.mark.parametrize("xm", cc.METHODS)
def test_handmade_and_damaged_streams_have_the_narrow_decoders_statuses(gpu, monkeypatch, xm):
    _piece(monkeypatch, "64")
    hand = [c for c in dc.handmade() if c[1] == xm]
    damaged, ncut = dc.damaged_batch(xm)
    streams = [c[2] for c in hand] + damaged
    host = [gpu.postprocess_block(xm, s) for s in streams]
    caps = [size for _, _, size in host]
    rc, bufs, sizes, status = gpu.lz77_decode_device_wide(xm, streams, caps, guard=GUARD, fill=FILL)
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
    rc, _, sizes_narrow, narrow = gpu.lz77_decode_device(xm, streams, caps, guard=GUARD, fill=FILL)
    assert rc == 0 and status == narrow and sizes == sizes_narrow


@pytest.mark.parametrize("xm", cc.METHODS)
def test_a_buffer_too_small_reports_every_size(gpu, host_streams, monkeypatch, xm):
    _piece(monkeypatch, "4096")
    pairs = host_streams(xm)
    sizes_want = [len(seen) for _, seen in pairs]
    caps = list(sizes_want)
    short = max(range(len(caps)), key=lambda k: caps[k])
    caps[short] -= 1
    rc, bufs, sizes, status = gpu.lz77_decode_device_wide(xm, [s for s, _ in pairs], caps, guard=GUARD, fill=FILL)
    assert rc == 3, (xm, rc)                                          # ZPQ_E_OVERFLOW
    assert sizes == sizes_want
    assert all(b == bytes([FILL]) * len(b) for b in bufs), (xm, "an overflowing batch wrote something")


# ---- archives: each setting in a fresh process ----
LZ_METHODS = ("1", "2", "x0,1,4,0,2,16", "x0,2,12,0,7,21,1c0,0,511", "x0,2,4,0,3,20c0,0,511")     # levels, a hash table, a suffix array, a model behind
OTHER_METHODS = ("x0,5,6,0,3,20", "x0,3ci1")                                                       # E8E9 in front, BWT
BIG_METHOD, BIG_BYTES = "x5,1,4,0,3,24", (1 << 24) + 4097

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
    out[m] = [back == b"".join(b.tobytes() for b in blocks), z.last_device_unlz_wide_segments(), z.last_device_unlz_segments()]
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
out = [back == want, z.last_device_unlz_wide_segments(), list(z.last_unlz_wide_pieces())]
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


@pytest.mark.parametrize("knob,count", [("1", 8), ("0", 0)])
def test_small_archives_round_trip_on_either_route(gpu, knob, count):
    """8 blocks of mixed kinds and lengths, one segment each, every stream long enough (ZPAQ_AMD_UNLZ_WIDE_FROM=1): with the knob
    at 1 every LZ77 segment is decoded by the wide kernels, with 0 none -- and E8E9 and BWT methods never are.  The bytes are the
    inputs either way."""
    got = _child(CHILD, {"ZPAQ_AMD_DEVICE_UNLZ_WIDE": knob, "ZPAQ_AMD_UNLZ_WIDE_FROM": "1", "ZPAQ_AMD_UNLZ_WIDE_PIECE": "4096"},
                 [json.dumps(list(LZ_METHODS + OTHER_METHODS))], 240)
    for m in LZ_METHODS:
        assert got[m][:2] == [True, count], (knob, m, got[m])
    for m in OTHER_METHODS:
        assert got[m] == [True, 0, 0], (knob, m, got[m])


def test_only_long_streams_take_the_route_and_the_rest_goes_on(gpu):
    """The default threshold of 1 MiB: none of the eight small blocks qualifies, and with ZPAQ_AMD_DEVICE_UNLZ=1 the group goes
    through the decoder of a wavefront per stream as ever."""
    got = _child(CHILD, {"ZPAQ_AMD_DEVICE_UNLZ_WIDE": "1", "ZPAQ_AMD_DEVICE_UNLZ": "1"}, [json.dumps(["1", "2"])], 240)
    for m, res in got.items():
        assert res == [True, 0, 8], (m, res)
    # streams of 64 KiB and more take the wide route, the others stay in their group
    got = _child(CHILD, {"ZPAQ_AMD_DEVICE_UNLZ_WIDE": "1", "ZPAQ_AMD_DEVICE_UNLZ": "1", "ZPAQ_AMD_UNLZ_WIDE_FROM": "65536"}, [json.dumps(["1"])], 240)
    ok, wide, narrow = got["1"]
    assert ok and wide >= 1 and wide + narrow == 8, got


def test_every_new_knob_unset_changes_nothing(gpu):
    got = _child(CHILD, {}, [json.dumps(["1", "2"])], 240)
    for m, res in got.items():
        assert res[:2] == [True, 0], (m, res)


@pytest.mark.parametrize("mode", ["device", "host"])
def test_a_forced_pcomp_route_keeps_its_meaning(gpu, mode):
    got = _child(CHILD, {"ZPAQ_AMD_PCOMP": mode, "ZPAQ_AMD_DEVICE_UNLZ_WIDE": "1", "ZPAQ_AMD_UNLZ_WIDE_FROM": "1"}, [json.dumps(["1", "x0,2,4,0,3,20c0,0,511"])], 240)
    for m, res in got.items():
        assert res == [True, 0, 0], (mode, m, res)


@pytest.fixture(scope="module")
def big_archive(gpu, tmp_path_factory):
    """One block of 2^24 + 4 097 bytes of text, stored LZ77 without a model: only the pre-processor and the decoder run."""
    d = tmp_path_factory.mktemp("unlz_wide")
    data = corpus.block("text", BIG_BYTES, 77)
    arch = gpu.compress_blocks([data.copy()], BIG_METHOD)
    (d / "arch").write_bytes(b"".join(arch))
    (d / "data").write_bytes(data.tobytes())
    return str(d / "arch"), str(d / "data")


@pytest.mark.parametrize("knob,count", [("1", 1), ("0", 0)])
def test_a_block_of_sixteen_mebibytes_and_more(gpu, big_archive, knob, count):
    ok, segments, pieces = _child(CHILD_BIG, {"ZPAQ_AMD_DEVICE_UNLZ_WIDE": knob}, list(big_archive), 300)
    assert ok and segments == count, (knob, ok, segments, pieces)
    if count:
        assert pieces[0] >= 64 and pieces[3] == 0, pieces
