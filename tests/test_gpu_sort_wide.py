"""The wide suffix sort on the device (device/sa_wide_kernel.h, build_suffix_array_wide in device/sa_kernels.hip): one block of
any length below 2^31, no block id in the key.  Small sizes against the host sorter; sizes beyond the batched sorter's 2^24 on
inputs whose array is known without a host sort; the stage entry against zpq_preprocess_block; the route through
zpq_compress_blocks in fresh child processes, the wide sorter forced on against forced off."""
import ctypes as C
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
FILL = 0xA5A5A5A5
GUARD, GFILL = 64, 0xC3
UNSUPPORTED, OVERFLOW = 8, 3
EDGE = (1 << 24) + 1                      # one byte more than the batched sorter's first declined length


def _sort(gpu, d, name):
    """zpq_suffix_array_device_wide over one buffer with one spare entry behind the array, which must keep its fill value."""
    n = len(d)
    rc, out = gpu.suffix_array_device_wide(d, spare=1, fill=FILL)
    assert rc == 0, (name, gpu.lib().zpq_last_error().decode())
    assert out[n] == FILL, (name, "a store past the array")
    return out[:n]


# ---- small sizes ----
@pytest.mark.parametrize("n", sc.GPU_LENGTHS)
def test_every_hard_string(gpu, n):
    """Every hard string at this length, entry for entry against the host sorter."""
    for k, d in sc.strings(n):
        got, want = _sort(gpu, d, (k, n)), sc.expected(d)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (k, n, "differs from the host sorter first at", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


def test_blocks_of_one_two_and_three_bytes(gpu):
    """Narrower rank fields than round 0's ranks (byte + 1) need: the first round runs 9 bits wide."""
    for d in (b"\x00", b"\xff", b"ab", b"ba", b"\xff\xff", b"\xff\x00", b"aba", b"\xff\x00\xff", b"\xff\xff\xff"):
        assert (_sort(gpu, d, d) == sc.naive_suffix_array(d)).all(), d


def test_the_empty_buffer(gpu):
    rc, out = gpu.suffix_array_device_wide(b"", spare=1, fill=FILL)
    assert rc == 0 and (out == FILL).all()


# ---- across the boundary: arrays known without a host sort ----
def test_zeros_beyond_the_24_bit_fields(gpu):
    """2^24 + 1 zeros: ranks up to 2^24 + 1 in 25-bit fields.  The array of a run is n - 1 - j, found in ceil(log2 n) = 25 rounds."""
    n = EDGE
    got = _sort(gpu, np.zeros(n, np.uint8), "zeros")
    bad = np.flatnonzero(got != np.arange(n - 1, -1, -1, dtype=np.uint32))
    assert bad.size == 0, ("zeros", n, "first wrong entry", int(bad[0]), int(got[bad[0]]))
    assert gpu.last_wide_sort_rounds() == 25


@pytest.mark.parametrize("last", ["b>a", "b<a"])
def test_a_run_and_one_other_byte(gpu, last):
    """a^(n-1) b at n = 2^24 + 1.  b > a: a suffix is the smaller the more a's it has in front of the b, 0, 1, ..., n - 1.
    b < a: the b ends every comparison the earlier the shorter the suffix, n - 1, ..., 0."""
    n = EDGE
    d = np.full(n, 0x61 if last == "b>a" else 0x62, np.uint8)
    d[n - 1] = 0x62 if last == "b>a" else 0x61
    got = _sort(gpu, d, last)
    want = np.arange(n, dtype=np.uint32) if last == "b>a" else np.arange(n - 1, -1, -1, dtype=np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (last, n, "first wrong entry", int(bad[0]), int(got[bad[0]]))


def test_random_bytes_beyond_the_boundary(gpu):
    """2^24 + 5 random bytes, checked without sorting anything on the host: the output is a permutation of 0..n-1, and the
    big-endian 8-byte prefixes of neighbouring suffixes (zero-padded past the end) ascend -- strictly, except where one of the
    two suffixes is shorter than 8 bytes (its padding may tie with real zeros; the shorter one must then stand first)."""
    n = (1 << 24) + 5
    d = np.random.default_rng(2024).integers(0, 256, n, dtype=np.uint8)
    got = _sort(gpu, d, "random")
    seen = np.zeros(n, bool)
    assert int(got.max()) < n
    seen[got] = True
    assert seen.all(), "not a permutation"
    padded = np.concatenate([d, np.zeros(8, np.uint8)]).astype(np.uint64)
    pre = np.zeros(n, np.uint64)
    for k in range(8):
        pre = (pre << np.uint64(8)) | padded[k:k + n]
    key = pre[got]
    short = got > n - 8
    either = short[:-1] | short[1:]
    assert (key[:-1][~either] < key[1:][~either]).all(), "8-byte prefixes of neighbouring suffixes do not ascend strictly"
    assert (key[:-1][either] <= key[1:][either]).all(), "a short suffix is out of order"
    tie = either & (key[:-1] == key[1:])
    assert (got[:-1][tie] > got[1:][tie]).all(), "of two suffixes that tie through the padding the shorter stands first"


# ---- the stage ----
STAGE_METHODS = ("x0,3", "x0,7", "x0,2,5,0,7,21,1c0,0,511", "x0,2,4,0,7,21,3c0,0,511")


def _host_stream(gpu, xm, d):
    """zpq_preprocess_block's stream and the buffer as the call left it (E8E9 methods filter it in place)."""
    L = gpu.lib()
    L.zpq_preprocess_block.argtypes = [C.c_char_p, u8p, C.c_uint32, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    buf = np.frombuffer(bytes(d), np.uint8).copy() if len(d) else np.zeros(1, np.uint8)
    out = np.empty(2 * len(d) + 4096, np.uint8)
    ol = C.c_size_t(0)
    assert L.zpq_preprocess_block(xm.encode(), buf.ctypes.data_as(u8p), len(d), out.ctypes.data_as(u8p), out.size, C.byref(ol)) == 0
    return out[:ol.value].tobytes(), buf[:len(d)].tobytes()


@pytest.mark.parametrize("n", [4097, 65537])
@pytest.mark.parametrize("xm", STAGE_METHODS)
def test_the_stage_against_the_host(gpu, xm, n):
    """zpq_preprocess_block_device_wide gives zpq_preprocess_block's stream byte for byte into a buffer of exactly its size, the
    64 guard bytes behind it untouched; into a buffer one byte short it reports the size, writes nothing and leaves the block as
    it came."""
    for name, d in tuple(sc.strings(n)) + ((("empty", b""),) if n == 4097 else ()):
        want, filtered = _host_stream(gpu, xm, d)
        buf = np.frombuffer(bytes(d), np.uint8).copy()
        rc, out, size = gpu.preprocess_block_device_wide(xm, buf, len(want), guard=GUARD, fill=GFILL)
        assert rc == 0, (xm, name, gpu.lib().zpq_last_error().decode())
        assert size == len(want) and out == want + bytes([GFILL]) * GUARD, (xm, name, size, len(want))
        assert buf.tobytes() == filtered, (xm, name, "the block is not the host's filtered block")
        if not want:
            continue                                  # (an empty stream fits every buffer)
        buf = np.frombuffer(bytes(d), np.uint8).copy()
        rc, out, size = gpu.preprocess_block_device_wide(xm, buf, len(want) - 1, guard=GUARD, fill=GFILL)
        assert rc == OVERFLOW and size == len(want), (xm, name, rc, size)
        assert out == bytes([GFILL]) * (len(want) - 1 + GUARD), (xm, name, "a call that overflowed wrote something")
        assert buf.tobytes() == d, (xm, name, "a call that failed left the block filtered")


def test_the_stage_declines_a_method_that_does_not_sort(gpu):
    d = sc.lcg(1000, 9)
    for xm in ("x0,0", "x0,4", "x0,1,4,0,3,16,1"):
        rc, out, size = gpu.preprocess_block_device_wide(xm, d, 2000, guard=GUARD, fill=GFILL)
        assert rc == UNSUPPORTED and out == bytes([GFILL]) * (2000 + GUARD), xm
        assert "does not sort suffixes" in gpu.lib().zpq_last_error().decode(), xm


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
    res = {"wide": z.last_wide_sort_blocks()}
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
    for k in ("ZPAQ_AMD_DEVICE_SORT_WIDE", "ZPAQ_AMD_SORT_WIDE_FROM", "ZPAQ_AMD_DEVICE_PARSE"):
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


SMALL_METHODS = ("x0,3", "x0,7ci1", "3", "x0,2,5,0,7,21,1c0,0,511")
SMALL_SIZES = (70001, 33333, 100003, 4097, 65537, 12345)


@pytest.fixture(scope="module")
def small_runs(gpu, tmp_path_factory):
    """Six ragged blocks of text and records, every method, with ZPAQ_AMD_SORT_WIDE_FROM=1: the wide route forced on, forced off,
    and forced on with the host making the streams from the device's arrays (ZPAQ_AMD_DEVICE_PARSE=0)."""
    from zpaq_amd import corpus
    tmp = tmp_path_factory.mktemp("wide_small")
    paths = []
    for i, n in enumerate(SMALL_SIZES):
        p = tmp / f"block{i}"
        corpus.block("text" if i % 2 == 0 else "records", n, corpus.BASE_SEED + i).tofile(p)
        paths.append(p)
    runs = [{"name": f"m{k}", "method": m, "blocks": list(range(len(paths))), "round_trip": True} for k, m in enumerate(SMALL_METHODS)]
    on = _child(tmp, "on", paths, runs, {"ZPAQ_AMD_SORT_WIDE_FROM": "1", "ZPAQ_AMD_DEVICE_SORT_WIDE": "1"})
    off = _child(tmp, "off", paths, runs, {"ZPAQ_AMD_SORT_WIDE_FROM": "1", "ZPAQ_AMD_DEVICE_SORT_WIDE": "0"})
    sort_only = _child(tmp, "sort_only", paths, runs, {"ZPAQ_AMD_SORT_WIDE_FROM": "1", "ZPAQ_AMD_DEVICE_SORT_WIDE": "1", "ZPAQ_AMD_DEVICE_PARSE": "0"})
    return on, off, sort_only


@pytest.mark.parametrize("k", range(len(SMALL_METHODS)))
def test_small_blocks_through_the_wide_route(small_runs, k):
    (on, arch_on), (off, arch_off), (so, arch_so) = small_runs
    name = f"m{k}"
    assert on[name]["wide"] == len(SMALL_SIZES) and off[name]["wide"] == 0 and so[name]["wide"] == len(SMALL_SIZES), (SMALL_METHODS[k], on[name], off[name], so[name])
    assert arch_on[name] == arch_off[name], SMALL_METHODS[k]
    assert arch_so[name] == arch_off[name], (SMALL_METHODS[k], "ZPAQ_AMD_DEVICE_PARSE=0")
    assert on[name]["round_trip"] and off[name]["round_trip"] and so[name]["round_trip"], SMALL_METHODS[k]


LARGE = (1 << 24) + 4097


@pytest.fixture(scope="module")
def large_runs(gpu, tmp_path_factory):
    """One real large block (2^24 + 4097 bytes of text) and four blocks of 64 KiB, method x5,3 (no model: nothing is coded on the
    device).  Forced on: the block alone, the batch of five, and the block alone under a budget of 256 MiB -- less than the
    block's 32 bytes of workspace per byte.  Forced off: the batch, whose first archive is also that of the block alone
    (archives are made block by block)."""
    from zpaq_amd import corpus
    tmp = tmp_path_factory.mktemp("wide_large")
    paths = [tmp / "large"] + [tmp / f"small{i}" for i in range(4)]
    corpus.block("text", LARGE, 777).tofile(paths[0])
    for i in range(4):
        corpus.block("text" if i % 2 == 0 else "records", 64 << 10, 900 + i).tofile(paths[1 + i])
    on = _child(tmp, "on", paths, [{"name": "alone", "method": "x5,3", "blocks": [0], "round_trip": True},
                                   {"name": "batch", "method": "x5,3", "blocks": [0, 1, 2, 3, 4]},
                                   {"name": "budget", "method": "x5,3", "blocks": [0], "budget": 256 << 20}], {"ZPAQ_AMD_DEVICE_SORT_WIDE": "1"})
    off = _child(tmp, "off", paths, [{"name": "batch", "method": "x5,3", "blocks": [0, 1, 2, 3, 4]}], {"ZPAQ_AMD_DEVICE_SORT_WIDE": "0"})
    return on, off


def test_one_large_block(large_runs):
    (on, arch_on), (off, arch_off) = large_runs
    assert on["alone"]["wide"] == 1 and off["batch"]["wide"] == 0
    assert arch_on["alone"][0] == arch_off["batch"][0]
    assert on["alone"]["round_trip"]


def test_a_large_block_among_small_ones(large_runs):
    (on, arch_on), (off, arch_off) = large_runs
    assert on["batch"]["wide"] == 1
    assert arch_on["batch"] == arch_off["batch"]


def test_a_large_block_over_the_budget(large_runs):
    """The device declines before anything is launched, the host sorts: the call succeeds with the same archive."""
    (on, arch_on), (off, arch_off) = large_runs
    assert on["budget"]["wide"] == 0
    assert arch_on["budget"][0] == arch_off["batch"][0]
