"""The LZ77 parse of one block in pieces on the device (device/lz77_wide_kernel.h behind the wide suffix sort): the stage entry
zpq_lz77_parse_device_wide token for token against zpq_lz77_tokens_host, the streams of zpq_preprocess_block_device_wide against
zpq_preprocess_block, and the route through zpq_compress_blocks in fresh child processes -- the device parse forced on against
the wide route forced off, small blocks and one real block of 2^24 + 4097 bytes."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sort_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(HERE)
u8p = C.POINTER(C.c_ubyte)
u32p = C.POINTER(C.c_uint32)
FILL = 0xA5A5A5A5
GUARD, GFILL = 64, 0xC3
UNSUPPORTED, OVERFLOW = 8, 3
KNOBS = ("ZPAQ_AMD_DEVICE_SORT_WIDE", "ZPAQ_AMD_SORT_WIDE_FROM", "ZPAQ_AMD_DEVICE_PARSE", "ZPAQ_AMD_DEVICE_PARSE_WIDE", "ZPAQ_AMD_LZ_WIDE_PIECE",
         "ZPAQ_AMD_DEVICE_CODES")
STAGE_METHODS = ("x0,1,4,0,7,21,1", "x0,2,12,0,7,21,1c0,0,511i2", "x0,6,5,0,7,21,1c0,0,511")        # (the last with E8E9 in front)


@functools.lru_cache(maxsize=None)
def _host(xm, d):
    """zpq_lz77_tokens_host, once per method and string: (the list as uint32 words, the block as the host's parse left it)."""
    import zpaq_amd as z
    L = z.lib()
    L.zpq_lz77_tokens_host.argtypes = [C.c_char_p, u8p, C.c_uint32, u32p, C.c_size_t, C.POINTER(C.c_size_t)]
    buf = np.frombuffer(bytearray(d), np.uint8).copy() if d else np.zeros(1, np.uint8)
    cap = len(d) + 4
    toks = np.zeros(4 * cap, np.uint32)
    cnt = C.c_size_t(0)
    assert L.zpq_lz77_tokens_host(xm.encode(), buf.ctypes.data_as(u8p), len(d), toks.ctypes.data_as(u32p), cap, C.byref(cnt)) == 0, L.zpq_last_error()
    want = toks[:4 * cnt.value].copy()
    want.setflags(write=False)
    return want, buf[:len(d)].tobytes()


def _stage(gpu, xm, name, d):
    """One string through zpq_lz77_parse_device_wide: into a list of exactly its size with one spare entry behind it, then into
    one a token short."""
    want, filtered = _host(xm, bytes(d))
    count = want.size // 4
    buf = np.frombuffer(bytes(d), np.uint8).copy()
    rc, toks, got = gpu.lz77_parse_device_wide(xm, buf, count, spare=1, fill=FILL)
    assert rc == 0, (xm, name, gpu.lib().zpq_last_error().decode())
    assert got == count, (xm, name, got, count)
    bad = np.flatnonzero(toks[:4 * count] != want)
    assert bad.size == 0, (xm, name, "token", int(bad[0]) // 4, toks[int(bad[0]) // 4 * 4:][:4].tolist(), want[int(bad[0]) // 4 * 4:][:4].tolist())
    assert (toks[4 * count:] == FILL).all(), (xm, name, "a store behind the list")
    assert buf.tobytes() == filtered, (xm, name, "the block is not the host's filtered block")
    if not count:
        return
    buf = np.frombuffer(bytes(d), np.uint8).copy()
    rc, toks, got = gpu.lz77_parse_device_wide(xm, buf, count - 1, spare=1, fill=FILL)
    assert rc == OVERFLOW and got == count, (xm, name, rc, got, count)
    assert (toks == FILL).all(), (xm, name, "a call that overflowed wrote something")
    assert buf.tobytes() == bytes(d), (xm, name, "a call that failed left the block filtered")


# ---- the stage ----
@pytest.mark.parametrize("piece", ["4096", None])
@pytest.mark.parametrize("n", [4097, 65537])
@pytest.mark.parametrize("xm", STAGE_METHODS)
def test_the_stage_against_the_host(gpu, monkeypatch, xm, n, piece):
    """Every hard string at this length (and the empty buffer), token for token the host's list."""
    if piece is None:
        monkeypatch.delenv("ZPAQ_AMD_LZ_WIDE_PIECE", raising=False)
    else:
        monkeypatch.setenv("ZPAQ_AMD_LZ_WIDE_PIECE", piece)
    for name, d in tuple(sc.strings(n)) + ((("empty", b""),) if n == 4097 else ()):
        _stage(gpu, xm, (name, n, piece), d)
    if n == 65537:
        pieces = gpu.last_wide_parse_pieces()
        assert pieces[0] == (17 if piece else 2) and sum(pieces[1:]) == pieces[0], pieces


def test_a_block_across_the_inverse_arrays_window(gpu, monkeypatch):
    """2^17 + 4097 bytes of text at 17 check bits: a look-ahead that leaves the window of its position finds nothing."""
    from zpaq_amd import corpus
    monkeypatch.delenv("ZPAQ_AMD_LZ_WIDE_PIECE", raising=False)
    d = corpus.block("text", (1 << 17) + 4097, corpus.BASE_SEED + 17).tobytes()
    _stage(gpu, "x0,1,4,0,7,21,1", "text", d)
    pieces = gpu.last_wide_parse_pieces()
    assert pieces[0] == 3 and sum(pieces[1:]) == 3 and pieces[2] >= 1, pieces


def test_the_stage_declines(gpu):
    """A method whose LZ77 does not search a suffix array: ZPQ_E_UNSUPPORTED with a note, nothing touched."""
    d = sc.lcg(1000, 9)
    for xm in ("x0,3", "x0,1,4,0,3,16,1"):
        buf = np.frombuffer(d, np.uint8).copy()
        rc, toks, count = gpu.lz77_parse_device_wide(xm, buf, 300, spare=1, fill=FILL)
        assert rc == UNSUPPORTED and count == 0 and (toks == FILL).all() and buf.tobytes() == d, xm
        assert "does not search a suffix array" in gpu.lib().zpq_last_error().decode(), xm


def test_the_stage_declines_a_parse_over_the_budget(gpu, monkeypatch):
    """Under a budget between zpq_wide_stage_bytes' two sums the sort alone would fit; the stage entry has no use for the array
    and declines: ZPQ_E_UNSUPPORTED with the budget in the note, nothing touched."""
    monkeypatch.delenv("ZPAQ_AMD_LZ_WIDE_PIECE", raising=False)
    xm, d = "x0,6,5,0,7,21,1c0,0,511", sc.string(65537, "zipf+zipf")
    sort, both = gpu.wide_stage_bytes(xm, len(d))
    buf = np.frombuffer(d, np.uint8).copy()
    gpu.set_state_budget((sort + both) // 2)
    try:
        rc, toks, count = gpu.lz77_parse_device_wide(xm, buf, len(d), spare=1, fill=FILL)
    finally:
        gpu.set_state_budget(0)
    assert rc == UNSUPPORTED and count == 0 and (toks == FILL).all() and buf.tobytes() == d
    assert "exceeds the device budget" in gpu.lib().zpq_last_error().decode()
    _stage(gpu, xm, "after the budget is lifted", d)


# ---- the streams ----
def _host_stream(gpu, xm, d):
    L = gpu.lib()
    L.zpq_preprocess_block.argtypes = [C.c_char_p, u8p, C.c_uint32, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    buf = np.frombuffer(bytes(d), np.uint8).copy() if len(d) else np.zeros(1, np.uint8)
    out = np.empty(2 * len(d) + 4096, np.uint8)
    ol = C.c_size_t(0)
    assert L.zpq_preprocess_block(xm.encode(), buf.ctypes.data_as(u8p), len(d), out.ctypes.data_as(u8p), out.size, C.byref(ol)) == 0
    return out[:ol.value].tobytes(), buf[:len(d)].tobytes()


@pytest.mark.parametrize("codes", ["1", "0"])
@pytest.mark.parametrize("xm", ["x0,1,4,0,7,21,1", "x0,2,12,0,7,21,1c0,0,511i2"])
def test_the_streams_against_the_host(gpu, monkeypatch, xm, codes):
    """zpq_preprocess_block_device_wide with the device parse forced on gives zpq_preprocess_block's stream byte for byte, the
    codes written on the device (ZPAQ_AMD_DEVICE_CODES=1) or by the host from the device's list (0); guard bytes untouched."""
    from zpaq_amd import corpus
    monkeypatch.setenv("ZPAQ_AMD_DEVICE_PARSE_WIDE", "1")
    monkeypatch.setenv("ZPAQ_AMD_DEVICE_CODES", codes)
    monkeypatch.setenv("ZPAQ_AMD_LZ_WIDE_PIECE", "4096")
    cases = tuple(sc.strings(4097)) + (("text", corpus.block("text", 70001, corpus.BASE_SEED).tobytes()), ("lcg", sc.lcg(12289, 5)), ("empty", b""))
    for name, d in cases:
        want, filtered = _host_stream(gpu, xm, d)
        buf = np.frombuffer(bytes(d), np.uint8).copy()
        rc, out, size = gpu.preprocess_block_device_wide(xm, buf, len(want), guard=GUARD, fill=GFILL)
        assert rc == 0, (xm, name, gpu.lib().zpq_last_error().decode())
        assert size == len(want) and out == want + bytes([GFILL]) * GUARD, (xm, codes, name, size, len(want))
        assert buf.tobytes() == filtered, (xm, name)


# ---- through zpq_compress_blocks, in fresh child processes ----
CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import zpaq_amd as z
spec = json.loads(open(sys.argv[2]).read())
z.init(0)
blocks = [np.fromfile(p, np.uint8) for p in spec["blocks"]]
out = {}
for run in spec["runs"]:
    use = [blocks[i].copy() for i in run["blocks"]]
    if run.get("budget"):
        z.set_state_budget(run["budget"])
    try:
        arch = z.compress_blocks(use, run["method"])
    finally:
        if run.get("budget"):
            z.set_state_budget(0)
    res = {"wide": z.last_wide_sort_blocks(), "wide_parse": z.last_wide_parse_blocks(), "pieces": list(z.last_wide_parse_pieces())}
    for k, a in enumerate(arch):
        open(os.path.join(spec["dir"], run["name"] + "." + str(k)), "wb").write(bytes(a))
    if run.get("round_trip"):
        res["round_trip"] = z.decompress(b"".join(bytes(a) for a in arch)) == b"".join(b.tobytes() for b in use)
    out[run["name"]] = res
z.shutdown()
print("RESULT " + json.dumps(out))
"""


def _child(tmp_path, tag, block_paths, runs, env_extra):
    """One fresh process: the runs of `runs` over the blocks in the files `block_paths`; (counters and flags per run, archives per run)."""
    d = tmp_path / tag
    d.mkdir()
    spec = d / "spec.json"
    spec.write_text(json.dumps({"dir": str(d), "blocks": [str(p) for p in block_paths], "runs": runs}))
    env = dict(os.environ)
    for k in KNOBS:
        env.pop(k, None)
    env.update(env_extra)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", CHILD, ROOT, str(spec)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=240)
    assert r.returncode == 0, (tag, r.stdout[-3000:])
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    arch = {run["name"]: [(d / f"{run['name']}.{k}").read_bytes() for k in range(len(run["blocks"]))] for run in runs}
    return got, arch


SMALL_METHODS = STAGE_METHODS + ("x0,3",)
SMALL_PARSED = (6, 6, 6, 0)
SMALL_SIZES = (70001, 33333, 100003, 4097, 65537, 12345)
FORCED = {"ZPAQ_AMD_SORT_WIDE_FROM": "1", "ZPAQ_AMD_DEVICE_SORT_WIDE": "1", "ZPAQ_AMD_DEVICE_PARSE_WIDE": "1", "ZPAQ_AMD_LZ_WIDE_PIECE": "4096"}


@pytest.fixture(scope="module")
def small_runs(gpu, tmp_path_factory):
    """Six ragged blocks of text and records, every method: the wide route with the device parse forced on, the wide route forced
    off, and the first with ZPAQ_AMD_DEVICE_PARSE=0 added (sort only: the host parses with the device's arrays)."""
    from zpaq_amd import corpus
    tmp = tmp_path_factory.mktemp("lz_wide_small")
    paths = []
    for i, n in enumerate(SMALL_SIZES):
        p = tmp / f"block{i}"
        corpus.block("text" if i % 2 == 0 else "records", n, corpus.BASE_SEED + i).tofile(p)
        paths.append(p)
    runs = [{"name": f"m{k}", "method": m, "blocks": list(range(len(paths))), "round_trip": True} for k, m in enumerate(SMALL_METHODS)]
    on = _child(tmp, "on", paths, runs, FORCED)
    off = _child(tmp, "off", paths, runs, {"ZPAQ_AMD_DEVICE_SORT_WIDE": "0"})
    sort_only = _child(tmp, "sort_only", paths, runs, dict(FORCED, ZPAQ_AMD_DEVICE_PARSE="0"))
    return on, off, sort_only


@pytest.mark.parametrize("k", range(len(SMALL_METHODS)))
def test_small_blocks_through_the_device_parse(small_runs, k):
    (on, arch_on), (off, arch_off), (so, arch_so) = small_runs
    name, xm = f"m{k}", SMALL_METHODS[k]
    assert on[name]["wide"] == len(SMALL_SIZES) and on[name]["wide_parse"] == SMALL_PARSED[k], (xm, on[name])
    assert off[name]["wide"] == 0 and off[name]["wide_parse"] == 0, (xm, off[name])
    assert so[name]["wide"] == len(SMALL_SIZES) and so[name]["wide_parse"] == 0, (xm, "ZPAQ_AMD_DEVICE_PARSE=0", so[name])
    assert arch_on[name] == arch_off[name], xm
    assert arch_so[name] == arch_off[name], (xm, "ZPAQ_AMD_DEVICE_PARSE=0")
    assert on[name]["round_trip"] and off[name]["round_trip"] and so[name]["round_trip"], xm


LARGE = (1 << 24) + 4097
LARGE_METHOD = "x5,1,4,0,7,26,1"


@pytest.fixture(scope="module")
def large_runs(gpu, tmp_path_factory):
    """One real block (2^24 + 4097 bytes of text), no model: the LZ77 stream is the archive.  Forced on: the block alone; under a
    budget halfway between zpq_wide_stage_bytes' two sums (the sort fits, the parse does not); under 256 MiB (neither fits).
    Forced off: the parent commit's path."""
    from zpaq_amd import corpus
    tmp = tmp_path_factory.mktemp("lz_wide_large")
    paths = [tmp / "large"]
    corpus.block("text", LARGE, 777).tofile(paths[0])
    sort, both = gpu.wide_stage_bytes(LARGE_METHOD, LARGE)
    assert sort < both
    on = _child(tmp, "on", paths, [{"name": "alone", "method": LARGE_METHOD, "blocks": [0], "round_trip": True},
                                   {"name": "half", "method": LARGE_METHOD, "blocks": [0], "budget": (sort + both) // 2},
                                   {"name": "budget", "method": LARGE_METHOD, "blocks": [0], "budget": 256 << 20}],
                {"ZPAQ_AMD_DEVICE_SORT_WIDE": "1", "ZPAQ_AMD_DEVICE_PARSE_WIDE": "1"})
    off = _child(tmp, "off", paths, [{"name": "alone", "method": LARGE_METHOD, "blocks": [0]}], {"ZPAQ_AMD_DEVICE_SORT_WIDE": "0"})
    return on, off


def test_one_large_block(large_runs):
    (on, arch_on), (off, arch_off) = large_runs
    assert on["alone"]["wide"] == 1 and on["alone"]["wide_parse"] == 1, on["alone"]
    assert off["alone"]["wide"] == 0 and off["alone"]["wide_parse"] == 0, off["alone"]
    assert arch_on["alone"][0] == arch_off["alone"][0]
    assert on["alone"]["round_trip"]
    pieces = on["alone"]["pieces"]
    assert pieces[0] == -(-LARGE // 65536) and sum(pieces[1:]) == pieces[0], pieces


def test_a_large_block_whose_parse_is_over_the_budget(large_runs):
    """The sort runs on the device, the array comes back and the host parses: the same archive."""
    (on, arch_on), (off, arch_off) = large_runs
    assert on["half"]["wide"] == 1 and on["half"]["wide_parse"] == 0, on["half"]
    assert arch_on["half"][0] == arch_off["alone"][0]


def test_a_large_block_over_the_budget(large_runs):
    """The device declines before anything is launched, the host sorts and parses: the same archive."""
    (on, arch_on), (off, arch_off) = large_runs
    assert on["budget"]["wide"] == 0 and on["budget"]["wide_parse"] == 0, on["budget"]
    assert arch_on["budget"][0] == arch_off["alone"][0]
