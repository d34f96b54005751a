"""The batched suffix sort on the device (device/sa_kernels.hip) over the inputs of tests/sort_cases.py -- the strings prefix
doubling finds hard, at every batch shape -- against the host sorter and the reference's divsufsort; sizes up to the 24-bit rank
fields' edge; the pre-processors and the archives that stand on its arrays, against the host and the reference; round trips."""
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
u8p, u32p = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint32)
FILL = 0xA5A5A5A5


def _buf(d: bytes) -> np.ndarray:
    return np.frombuffer(bytes(d), np.uint8).copy() if len(d) else np.zeros(1, np.uint8)


def _sort_on_device(gpu, datas):
    """zpq_suffix_arrays_device over one batch: (return code, the output buffers -- pre-filled with FILL, one spare entry each)."""
    L = gpu.lib()
    L.zpq_suffix_arrays_device.argtypes = [C.POINTER(u8p), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(u32p)]
    n = len(datas)
    bufs = [d if isinstance(d, np.ndarray) else _buf(d) for d in datas]
    lens = [len(d) for d in datas]
    outs = [np.full(ln + 1, FILL, np.uint32) for ln in lens]
    IA = (u8p * n)(*[b.ctypes.data_as(u8p) for b in bufs])
    LN = (C.c_uint32 * n)(*lens)
    OA = (u32p * n)(*[o.ctypes.data_as(u32p) for o in outs])
    return L.zpq_suffix_arrays_device(IA, LN, n, OA), outs


def _check_shape(gpu, shape, blocks, ref=None):
    rc, outs = _sort_on_device(gpu, [d for _, d in blocks])
    assert rc == 0, (shape, gpu.lib().zpq_last_error().decode())
    for k, ((name, d), o) in enumerate(zip(blocks, outs)):
        want = sc.expected(d)
        bad = np.flatnonzero(o[:len(d)] != want)
        assert bad.size == 0, (shape, k, name, "differs from the host sorter first at", int(bad[0]), int(o[bad[0]]), int(want[bad[0]]))
        assert o[len(d)] == FILL, (shape, k, name, "a store past the block's array")
        if ref is not None and len(d):
            assert (o[:len(d)].astype(np.int64) == ref.divsufsort(d).astype(np.int64)).all(), (shape, k, name, "differs from divsufsort")


@pytest.mark.parametrize("n", sc.GPU_LENGTHS)
def test_every_hard_string_alone(gpu, ref, n):
    """One block per call: every hard string at this length, entry for entry against the host sorter and the reference's."""
    for shape, blocks in sc.alone((n,)):
        _check_shape(gpu, shape, blocks, ref)


@pytest.mark.parametrize("n", sc.GPU_LENGTHS)
def test_two_and_three_blocks(gpu, ref, n):
    for shape, blocks in sc.small_batches((n,)):
        _check_shape(gpu, shape, blocks, ref)


@pytest.mark.parametrize("shape", ["many256", "many257", "boundary", "boundary65537"])
def test_many_blocks_and_the_batch_edges(gpu, ref, shape):
    """256 and 257 blocks (8 and 9 bits of block id in the key), and the boundary batch: empty blocks first, in the middle and
    last, runs of zeros that meet runs of zeros, one hard string four times."""
    name, blocks = {"many256": lambda: sc.many(256), "many257": lambda: sc.many(257), "boundary": lambda: sc.boundary(4097),
                    "boundary65537": lambda: sc.boundary(65537)}[shape]()
    _check_shape(gpu, name, blocks, ref)


@pytest.mark.parametrize("which", ["period3", "fibonacci_ab"])
def test_four_mebibytes_in_one_block(gpu, which):
    """Sizes the suite has never sorted: 2^22 + 1 bytes of the period-3 repeat (22 rounds), 2^22 bytes of the Fibonacci word."""
    n = (1 << 22) + 1 if which == "period3" else 1 << 22
    d = sc.repeat(sc._lcg_pattern(3), n) if which == "period3" else sc.fibonacci(n, 0x61, 0x62)
    _check_shape(gpu, f"alone/{which}/{n}", ((f"{which}/{n}", d),))


def test_a_block_that_fills_both_rank_fields(gpu):
    """2^24 - 1 zeros: ranks up to 2^24 - 1 in both 24-bit fields of the key, 24 rounds.  The array of a run is n - 1 - j."""
    n = (1 << 24) - 1
    rc, outs = _sort_on_device(gpu, [np.zeros(n, np.uint8)])
    assert rc == 0, gpu.lib().zpq_last_error().decode()
    bad = np.flatnonzero(outs[0][:n] != np.arange(n - 1, -1, -1, dtype=np.uint32))
    assert bad.size == 0, ("zeros", n, "first wrong entry", int(bad[0]), int(outs[0][bad[0]]))
    assert outs[0][n] == FILL


def test_a_block_of_two_to_the_24_is_declined(gpu):
    """One entry more than the rank fields hold: the call says so and leaves the output as it was."""
    n = 1 << 24
    rc, outs = _sort_on_device(gpu, [b"abc", np.zeros(n, np.uint8)])
    assert rc != 0
    assert "outside the device sorter's range" in gpu.lib().zpq_last_error().decode()
    assert all((o == FILL).all() for o in outs), "a declined batch wrote something"


# ---- what stands on the arrays ----
PRE_METHODS = ("x0,2,5,0,7,21,1c0,0,511", "x0,1,4,0,3,21,1", "x0,2,4,0,7,21,3c0,0,511", "x0,3ci1")


@pytest.mark.parametrize("shape", ["boundary", "many257"])
@pytest.mark.parametrize("xm", PRE_METHODS)
def test_preprocessing_against_the_host(gpu, xm, shape):
    """zpq_preprocess_blocks_device (sort, LZ77 parse / BWT on the device) must give zpq_preprocess_block's stream, byte for byte."""
    L = gpu.lib()
    L.zpq_preprocess_blocks_device.argtypes = [C.c_char_p, C.POINTER(u8p), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(u8p), C.POINTER(C.c_size_t),
                                               C.POINTER(C.c_size_t)]
    L.zpq_preprocess_block.argtypes = [C.c_char_p, u8p, C.c_uint32, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    name, blocks = sc.boundary(4097) if shape == "boundary" else sc.many(257)
    n = len(blocks)
    dev_in = [np.concatenate([_buf(d)[:len(d)], np.zeros(8, np.uint8)]) for _, d in blocks]
    outs = [np.empty(len(d) + len(d) // 2 + 4096, np.uint8) for _, d in blocks]
    IA = (u8p * n)(*[b.ctypes.data_as(u8p) for b in dev_in])
    LN = (C.c_uint32 * n)(*[len(d) for _, d in blocks])
    OA = (u8p * n)(*[o.ctypes.data_as(u8p) for o in outs])
    CP = (C.c_size_t * n)(*[o.size for o in outs])
    OL = (C.c_size_t * n)()
    assert L.zpq_preprocess_blocks_device(xm.encode(), IA, LN, n, OA, CP, OL) == 0, (xm, name, L.zpq_last_error().decode())
    for k, (bname, d) in enumerate(blocks):
        host_in = _buf(d)
        want = np.empty(outs[k].size, np.uint8)
        wl = C.c_size_t(0)
        assert L.zpq_preprocess_block(xm.encode(), host_in.ctypes.data_as(u8p), len(d), want.ctypes.data_as(u8p), want.size, C.byref(wl)) == 0
        assert OL[k] == wl.value and (outs[k][:wl.value] == want[:wl.value]).all(), (xm, name, k, bname, OL[k], wl.value)


ARCHIVE_METHODS = ("3", "3,128,1", "2")         # byte-aligned LZ77 + ICM/ISSE, BWT + ICM/ISSE, bit-packed LZ77
ARCHIVE_STRINGS = ("run00", "a^(n-1)b,b>a", "period3", "period5+middle", "period257+last", "fibonacci_ab", "fibonacci_00FF", "thue_morse_ab",
                   "two_letters", "counting_up", "s+s", "zipf+zipf")


def archive_blocks():
    """12 hard strings of 96 to 160 KiB (odd lengths): 1.5 MiB, 12 sorting blocks -- a batch that takes the device path."""
    return [(f"{k}/{(96 << 10) + 5957 * i + 1}", sc.string((96 << 10) + 5957 * i + 1, k)) for i, k in enumerate(ARCHIVE_STRINGS)]


@pytest.fixture(scope="module")
def archives(gpu):
    """The archives of the batch, one list per method, with slot 7 of zpq_last_api_timing (blocks sorted on the device) beside it."""
    blocks = archive_blocks()
    assert all((96 << 10) <= len(d) <= (160 << 10) for _, d in blocks)
    ph = (C.c_double * 8)()
    out = {}
    for m in ARCHIVE_METHODS:
        arch = gpu.compress_blocks([_buf(d) for _, d in blocks], m)
        gpu.lib().zpq_last_api_timing(ph)
        out[m] = (arch, int(ph[7]))
    return blocks, out


@pytest.mark.parametrize("method", ARCHIVE_METHODS)
def test_archives_against_the_reference(gpu, ref, archives, method):
    blocks, out = archives
    arch, sorted_on_device = out[method]
    assert sorted_on_device == len(blocks), (method, sorted_on_device)          # every block's suffix array came from the device
    for (name, d), a in zip(blocks, arch):
        assert a == ref.compress_block(d, method), (method, name)


def test_archives_round_trip(gpu, archives):
    blocks, out = archives
    for m, (arch, _) in out.items():
        assert gpu.decompress(b"".join(arch)) == b"".join(d for _, d in blocks), m


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import zpaq_amd as z
z.init(0)
want = open(sys.argv[2], "rb").read()
out = {}
for m, path in json.loads(sys.argv[3]).items():
    back = z.decompress(open(path, "rb").read())
    out[m] = [back == want, z.last_device_unbwt_segments(), z.last_device_unlz_segments()]
z.shutdown()
print("RESULT " + json.dumps(out))
"""


def test_archives_round_trip_through_the_device_decoders(gpu, archives, tmp_path):
    """The same archives in a fresh process with the BWT and LZ77 decoders of the device switched on.  The bytes must be the
    inputs; the decoders may decline any stream, so of their segment counters only "not both zero" is asserted."""
    blocks, out = archives
    (tmp_path / "want").write_bytes(b"".join(d for _, d in blocks))
    paths = {}
    for k, (m, (arch, _)) in enumerate(out.items()):
        (tmp_path / f"arch{k}").write_bytes(b"".join(arch))
        paths[m] = str(tmp_path / f"arch{k}")
    env = dict(os.environ)
    env.pop("ZPAQ_AMD_PCOMP", None)
    env.update({"ZPAQ_AMD_DEVICE_UNBWT": "1", "ZPAQ_AMD_DEVICE_UNLZ": "1"})
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", CHILD, ROOT, str(tmp_path / "want"), json.dumps(paths)], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for m in ARCHIVE_METHODS:
        same, unbwt, unlz = got[m]
        assert same, (m, "segments decoded on the device: BWT", unbwt, "LZ77", unlz)
        assert unbwt or unlz, (m, "segments decoded on the device: BWT", unbwt, "LZ77", unlz)
