"""CPU: the host side of the boundary (no compute calls, no GPU): ABI exports,
SHA-1, constant tables, method expansion, ZPAQL assembler, container scan."""
import ctypes
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import pytest

from conftest import ROOT, gen_input
from oracle.oracle_py import parse_block
from zpaq_amd import corpus


def test_abi_exports_every_declared_symbol(zlib_):
    hdr = open(os.path.join(ROOT, "include", "zpaq_amd.h")).read()
    names = set(re.findall(r"\b(zpq_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 25
    L = zlib_.lib()
    missing = [n for n in sorted(names) if not hasattr(L, n)]
    assert not missing, missing


def test_library_fails_loudly_without_gpu(zlib_):
    if zlib_.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(zlib_.ZpaqError) as ei:
        zlib_.init(0)
    assert "no CPU fallback" in str(ei.value)
    with pytest.raises(zlib_.ZpaqError):
        zlib_.compress_block(b"hello world" * 10, "5")


def test_product_never_touches_the_oracle():
    """Nothing under zpaq_amd/ may import, link or load anything from oracle/."""
    bad = []
    for dp, _, fns in os.walk(os.path.join(ROOT, "zpaq_amd")):
        for fn in fns:
            if fn.endswith((".py", ".cpp", ".hpp", ".h", ".hip", "Makefile")):
                txt = open(os.path.join(dp, fn), errors="ignore").read()
                if re.search(r"oracle[/_.]|zpaq_oracle|libzpaq_ref", txt):
                    bad.append(os.path.join(dp, fn))
    assert not bad, bad


def test_sha1(zlib_):
    for n in [0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 1000, 70000]:
        d = corpus.lcg_bytes(n, 3)
        assert zlib_.sha1(d) == hashlib.sha1(d.tobytes()).digest()


def test_sha1_portable_path(zlib_):
    """sha1.cpp picks the x86 SHA-extension compression function at run time; the portable one must agree."""
    import hashlib
    lens = (0, 1, 55, 56, 63, 64, 65, 127, 128, 1000, 70001)
    try:
        for portable in (1, 0):
            zlib_.lib().zpq_sha1_force_portable(portable)
            assert all(zlib_.sha1(corpus.lcg_bytes(n, 9)) == hashlib.sha1(corpus.lcg_bytes(n, 9).tobytes()).digest() for n in lens)
    finally:
        zlib_.lib().zpq_sha1_force_portable(0)


def test_tables_match_oracle_and_checksums(zlib_, oracle):
    for name in ["squash", "stretch", "dt", "dt2k", "state"]:
        assert (zlib_.table(name) == oracle.table(name)).all(), name
    st = zlib_.table("stretch").astype(np.int64)
    sq = zlib_.table("squash").astype(np.int64)
    s1 = 0
    for v in st[::-1]:
        s1 = (s1 * 3 + int(v)) & 0xFFFFFFFF
    s2 = 0
    for v in sq[::-1]:
        s2 = (s2 * 3 + int(v)) & 0xFFFFFFFF
    assert s1 == 3887533746 and s2 == 2278286169      # libzpaq.cpp:1759-1760


def test_method_expansion_and_headers_vs_golden(zlib_, golden):
    """expand_method + make_config + assembler reproduce the header bytes stored in reference archives."""
    n = 0
    for e in golden["method_cases"]:
        d = gen_input(e)
        xm = zlib_.expand_method(e["method"], d)
        h, p, args = zlib_.method_to_header(xm)
        assert h.hex() == e["header"], (e["kind"], e["n"], e["method"], xm)
        assert p == b""
        n += 1
    assert n >= 60


def test_method_expansion_live(zlib_, ref):
    for kind in ["zeros", "text", "lcg", "records", "pattern"]:
        for n in [0, 5, 4097, 70000, 1 << 20]:
            d = corpus.block(kind, n, 4242)
            for method in ["5", "4", "0", "57", "5,128,0", "5,200,1", "4,100,0", "4,60,1", "8"]:
                xm = zlib_.expand_method(method, d)
                h, p, args = zlib_.method_to_header(xm)
                cfg, rargs = ref.make_config(xm)
                assert (h, p) == ref.compile(cfg, rargs) and args == rargs, (kind, n, method, xm)


def test_unsupported_methods_fail_loudly(zlib_):
    """What stays outside (index-block methods of the journaling archiver, undefined pre-processor codes) fails with a
    status, it does not produce a different archive.  (Levels 1-3 and the E8E9 hints did fail here in round 1: they
    are implemented now, see the pre-processing tests below.)"""
    for xm, code in [("i0,0", 8), ("x0,8", 9), ("x0,9ci1", 9)]:
        with pytest.raises(zlib_.ZpaqError) as ei:
            zlib_.method_to_header(xm)
        assert ei.value.code == code, xm
    d = corpus.block("text", 5000, 1)
    for method in ["1", "2", "3", "5,128,2"]:
        zlib_.method_to_header(zlib_.expand_method(method, d))


def test_assembler_vs_reference_compiler(zlib_, ref, golden):
    cfgs = [golden["config_cases"][0]["config"]]
    for xm in ["x0,1,4,0,3,20", "x1,1,5,0,3,21", "x0,2,12,0,7,21,1c0,0,511i2", "x0,3ci1", "x2,7ci1",
               "x0,5,4,0,3,20", "x0,6,5,0,7,21,1c0,0,511", "x6,1,6,0,3,26", "x0,0ci1,1,1,1,2awm",
               "x0,0c1000,0,255c0,1300,255,1500,255i2,13s16,32,255m12t8"]:
        cfg, args = ref.make_config(xm)
        assert zlib_.assemble(cfg, args) == ref.compile(cfg, args), xm
    cfgs.append("""comp 3 8 0 0 2 0 cm 12 20 1 icm 10 hcomp
      b<>a *c<>a c++ *c=a d=0 do a=*d a+=*c hashd d++ a=d a< 3 while
      a=c a== 0 ifnot a=r 3 else a= 5 r=a 3 endif do a-- a> 200 until
      a< 3 ifl b=0 elsel c=0 endif A=B a+= $2+7 Jmp 1 a++ halt
      pcomp cat ; a> 255 if halt endif out do a++ a== 9 if halt endif forever halt end""")
    for cfg in cfgs:
        assert zlib_.assemble(cfg, [1, 2, 3]) == ref.compile(cfg, [1, 2, 3])


def test_assembler_golden_all_types(zlib_, golden):
    e = golden["config_cases"][0]
    h, p = zlib_.assemble(e["config"])
    assert h.hex() == e["header"] and p == b""


def test_assembler_errors(zlib_):
    for bad in ["comp 0 0 0 0 0 hcomp foo end", "comp 0 0 0 0 1 0 cm 300 2 hcomp halt end", "comp 0 0",
                "comp 0 0 0 0 1 1 cm 3 2 hcomp halt end", "comp 0 0 0 0 0 hcomp endif end"]:
        with pytest.raises(zlib_.ZpaqError):
            zlib_.assemble(bad)


def test_plan_memory_and_roofline_bytes(zlib_, golden):
    for e in golden["method_cases"]:
        hdr = bytes.fromhex(e["header"])
        if hdr[6] == 0:
            continue
        p = zlib_.Plan(hdr)
        assert p.memory == e["memory"]                 # ZPAQL::memory() as findBlock reports it
        assert p.ncomp == hdr[6]
        assert p.state_bytes >= e["memory"] - 2 * 2 ** hdr[4] - 2 ** hdr[5] - 400
    # default -m5 chain at 1 MiB: A = 3626 B per input byte
    d = corpus.block("text", 1 << 20, corpus.BASE_SEED)
    h, _, _ = zlib_.method_to_header(zlib_.expand_method("5", d))
    p = zlib_.Plan(h)
    assert p.ncomp == 23 and p.algo_bytes_per_byte == 3626.0 and p.memory == 101699634.0


def test_plan_rejects_bad_headers(zlib_, golden):
    hdr = bytearray(bytes.fromhex(golden["method_cases"][0]["header"]))
    for mutate in (lambda h: h.__setitem__(7, 77), lambda h: h.__setitem__(0, h[0] ^ 1),
                   lambda h: h.__setitem__(len(h) - 1, 9)):
        h = bytearray(hdr)
        mutate(h)
        with pytest.raises(zlib_.ZpaqError):
            zlib_.Plan(bytes(h))


def test_stored_blocks_are_host_only_and_bit_exact(zlib_, golden):
    """Method "0" has no model: pure container plumbing, identical to the reference without a GPU."""
    e = [x for x in golden["method_cases"] if x["method"] == "0"][0]
    a = zlib_.compress_block(gen_input(e), "0", e["filename"], e["comment"])
    assert len(a) == e["len"] and hashlib.sha1(a).hexdigest() == e["sha1"]
    assert zlib_.decompress(a) == gen_input(e).tobytes()


def test_pcomp_postprocessing_decodes_reference_lz77_archives(zlib_, ref):
    """Methods 0/1/2 have no model (n = 0): the whole decode path -- container scan, stored framing,
    PCOMP post-processor running the LZ77 / E8E9 programs carried in the archive -- is host work."""
    for kind, n in [("text", 150000), ("zeros", 65536), ("lcg", 30000), ("records", 60000), ("text", 0), ("text", 1)]:
        d = corpus.block(kind, n, 321)
        for m in ["1", "2", "1,200,1", "2,128,3", "1,60,2", "0"]:
            a = ref.compress_block(d, m)
            assert zlib_.decompress(a) == d.tobytes(), (kind, n, m)
    # several blocks / methods in one stream
    parts = [corpus.block("text", 5000, 1), corpus.block("pattern", 7000, 2), corpus.block("lcg", 100, 3)]
    stream = b"".join(ref.compress_block(p, m) for p, m in zip(parts, ["1", "2", "0"]))
    assert zlib_.decompress(stream) == b"".join(p.tobytes() for p in parts)


def test_codegen_translates_random_hcomp_and_compiles_for_gfx950(zlib_, golden, tmp_path):
    """The per-header specialisation (HCOMP -> HIP source) handles arbitrary control flow, and the
    generated translation units cross-compile for gfx950 (no GPU needed)."""
    import ctypes as C
    import subprocess
    L = zlib_.lib()
    L.zpq_plan_spec_source.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p]
    L.zpq_spec_include_dir.restype = C.c_char_p
    inc = L.zpq_spec_include_dir().decode()
    built = 0
    for e in golden["vm_cases"] + golden["config_cases"]:
        plan = zlib_.Plan(bytes.fromhex(e["header"]))
        buf = C.create_string_buffer(4 << 20)
        ln = C.c_size_t(0)
        key = C.create_string_buffer(41)
        rc = L.zpq_plan_spec_source(plan._h, buf, len(buf), C.byref(ln), key)
        if plan.ncomp > 64:
            assert rc == 8          # ZPQ_E_UNSUPPORTED: generic one-lane kernel only
            continue
        assert rc == 0, L.zpq_last_error()
        src = buf.value.decode()
        assert "zpq_spec_encode" in src and "hcomp(" in src and len(key.value) == 40
        if built < 3:               # compiling every case would take a minute; three cover the shapes
            f = tmp_path / (key.value.decode() + ".hip")
            f.write_text(src)
            r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wno-unused-label",
                                "-I", inc, "--genco", str(f), "-o", str(f) + ".hsaco"],
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            assert r.returncode == 0, r.stdout[-3000:]
            built += 1
    assert built == 3


def test_hiprtc_compiles_a_generated_kernel_without_a_gpu(zlib_, golden):
    """The run-time specialisation path (hipRTC, used for headers nobody prebuilt) must compile on
    its own: hipRTC has no C library headers, so the kernel template may not depend on any."""
    import ctypes as C
    L = zlib_.lib()
    L.zpq_plan_spec_jit.restype = C.c_size_t
    L.zpq_plan_spec_jit.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    plan = zlib_.Plan(bytes.fromhex(golden["vm_cases"][3]["header"]))
    log = C.create_string_buffer(16384)
    n = L.zpq_plan_spec_jit(plan._h, log, len(log))
    assert n > 10000, log.value.decode(errors="replace")[:3000]


def test_unseen_headers_compile_side_by_side(zlib_, tmp_path, monkeypatch):
    """A batch that brings several headers nobody prebuilt (level-5 chains with data-dependent periodic models) must not
    pay one hipRTC compilation after the other: zpq_precompile (what the engine runs at the start of such a batch) compiles
    them in helper processes side by side into the code-object cache, where the loaders find them.  No GPU needed."""
    import ctypes as C
    import os
    import time
    L = zlib_.lib()
    L.zpq_precompile.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_int, C.c_int]
    monkeypatch.setenv("ZPAQ_AMD_SPEC_CACHE", str(tmp_path))
    assert os.access(os.path.join(os.path.dirname(zlib_.lib()._name), "zpq_jitc"), os.X_OK), "helper not built"
    plans = [zlib_.Plan(zlib_.method_to_header(f"x0,0ci2,1,1c0,{200 + i}m16s")[0]) for i in range(4)]
    arr = (C.c_void_p * len(plans))(*[p._h for p in plans])
    for decode in (0, 1):
        t0 = time.time()
        assert L.zpq_precompile(arr, len(plans), decode, 4) == 4, L.zpq_last_error()
        took = time.time() - t0
        files = sorted(os.listdir(tmp_path))
        assert len(files) == 4 * (decode + 1) and all(f.endswith(".hsaco") for f in files), files
        assert all(os.path.getsize(tmp_path / f) > 10000 for f in files)
        assert took < 60
        # the cache key the loader will look for is the one the source functions report
        src = C.create_string_buffer(1 << 21)
        key = C.create_string_buffer(41)
        ln = C.c_size_t()
        fn = L.zpq_plan_spec_source if decode else L.zpq_plan_pipe_source
        assert fn(plans[0]._h, src, len(src), C.byref(ln), key) == 0
        assert key.value.decode() + ".hsaco" in files
    assert L.zpq_precompile(arr, len(plans), 0, 4) == 0          # nothing left to do
    # one thread = no helper processes: the same code objects from hipRTC inside this process
    more = [zlib_.Plan(zlib_.method_to_header(f"x0,0ci2,1,1c0,{100 + i}m16s")[0]) for i in range(2)]
    arr2 = (C.c_void_p * len(more))(*[p._h for p in more])
    assert L.zpq_precompile(arr2, len(more), 0, 1) == 2, L.zpq_last_error()
    assert len(os.listdir(tmp_path)) == 10
    # a cache directory that cannot be written: the code objects stay in the process (the loaders look there first)
    monkeypatch.setenv("ZPAQ_AMD_SPEC_CACHE", "/proc/zpaq_amd_no_such_dir")
    extra = [zlib_.Plan(zlib_.method_to_header(f"x0,0ci2,1,1c0,{150 + i}m16s")[0]) for i in range(2)]
    arr3 = (C.c_void_p * len(extra))(*[p._h for p in extra])
    assert L.zpq_precompile(arr3, len(extra), 0, 2) == 2, L.zpq_last_error()
    assert L.zpq_precompile(arr3, len(extra), 0, 2) == 0


# ---------------------------------------------------------------------------------------------------------
# LZ77 / BWT / E8E9 on the compression side (host/preproc.cpp + the PCOMP generators of host/method.cpp):
# levels 1-3, the hinted branches of 4, and explicit "x" methods.  SURVEY section 8(f) row 1.

def _exe_like(n, seed):
    """bytes with many E8|E9 xx xx xx 00|FF patterns, so that the E8E9 filter has work to do"""
    r = np.random.default_rng(seed)
    b = r.integers(0, 256, n, dtype=np.uint8)
    for i in range(0, n - 8, 37):
        b[i] = 0xE8 if (i // 37) % 2 else 0xE9
        b[i + 4] = 0 if (i // 37) % 3 else 0xFF
    return b


def _preprocess(zlib_, xm, d):
    import ctypes as C
    L = zlib_.lib()
    L.zpq_preprocess_block.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    buf = np.array(d, dtype=np.uint8, copy=True)
    out = np.empty(len(d) * 2 + 4096, np.uint8)
    ln = C.c_size_t(0)
    assert L.zpq_preprocess_block(xm.encode(), buf.ctypes.data, len(buf), out.ctypes.data, out.size, C.byref(ln)) == 0
    return out[:ln.value].tobytes()


def test_preprocessing_methods_headers_and_pcomp_match_the_reference(zlib_, ref):
    """makeConfig for every branch compressBlock takes at levels 1-4 (block type x hint) and every block-size
    exponent: stored header and PCOMP bytes identical to the reference's (the PCOMP program is part of the archive)."""
    n = 0
    for kind, size in [("text", 30000), ("lcg", 20000), ("zeros", 10000), ("records", 25000)]:
        d = corpus.block(kind, size, 11)
        for level in "1234":
            for hint in ["", ",0,0", ",10,0", ",30,1", ",60,2", ",100,3", ",128,1", ",200,0", ",255,2", ",20,3", ",250,1"]:
                xm = zlib_.expand_method(level + hint, d)
                cfg, args = ref.make_config(xm)
                assert zlib_.method_to_header(xm)[:2] == ref.compile(cfg, args), (level + hint, xm)
                n += 1
    for a0 in range(0, 8):       # offsets with low bits (rb > 0), the two inverse-BWT variants
        for body in [",1,4,0,3,%d" % (19 + a0 + (a0 <= 6)), ",5,4,0,3,%d" % (19 + a0 + (a0 <= 6)), ",2,12,0,7,%d,1c0,0,511i2" % (21 + a0),
                     ",6,5,0,7,%d1c0,0,511" % (21 + a0), ",3ci1", ",7ci1", ",4ci1,1,1,1,2am"]:
            xm = "x%d%s" % (a0, body)
            cfg, args = ref.make_config(xm)
            assert zlib_.method_to_header(xm)[:2] == ref.compile(cfg, args), xm
            n += 1
    assert n > 200


def test_preprocessed_streams_match_the_reference(zlib_, ref, oracle):
    """What the coder is fed after LZ77 / BWT / E8E9 must be the reference's bytes: checked through the reference's
    archives -- stored payloads directly (methods without a model), modelled ones by coding our stream with the oracle."""
    inputs = [corpus.block("text", 40000, 3), corpus.block("lcg", 20000, 4), corpus.block("zeros", 12000, 5),
              corpus.block("records", 30000, 6), _exe_like(30000, 8), np.zeros(0, np.uint8), np.array([65], np.uint8),
              corpus.block("text", 7, 9)]
    methods = ["1", "2", "3", "4", "1,40,0", "1,100,0", "1,250,0", "2,40,0", "2,128,2", "3,30,0", "3,128,1", "3,160,3",
               "4,15,0", "4,30,2", "4,128,3", "4,230,2", "x0,4", "x0,5,4,0,3,20", "x0,6,8,0,4,21", "x0,7", "x0,1,4,6,3,18,1"]
    for di, d in enumerate(inputs):
        for m in methods:
            xm = zlib_.expand_method(m, d)
            a = ref.compress_block(d, m)
            f = parse_block(a)
            hdr, ps = f["header"], f["payload_start"]
            ours_hdr, pc, _ = zlib_.method_to_header(xm)
            assert ours_hdr == hdr, (di, m)
            body = ((b"\x01" + pc) if pc else b"\x00") + _preprocess(zlib_, xm, d)
            if hdr[6] == 0:
                want, pos = b"", 0
                while pos < len(body):
                    k = min(65536, len(body) - pos)
                    want += k.to_bytes(4, "big") + body[pos:pos + k]
                    pos += k
                assert a[ps:ps + len(want) + 4] == want + b"\0\0\0\0", (di, m, xm)
            else:
                coded = oracle.encode(hdr, body)
                assert a[ps:ps + len(coded) + 4] == coded + b"\0\0\0\0", (di, m, xm)


def test_suffix_array_against_naive_sort(zlib_):
    """host/preproc.cpp's SA-IS through the BWT it feeds: x0,3 over short strings with long repeats."""
    rng = np.random.default_rng(12)
    for trial in range(40):
        n = int(rng.integers(1, 300))
        d = rng.integers(0, int(rng.integers(1, 5)) + 1, n, dtype=np.uint8) + 97
        s = d.tobytes()
        sa = sorted(range(n), key=lambda i: s[i:])
        want = bytes([s[n - 1]]) + bytes(255 if p == 0 else s[p - 1] for p in sa)
        idx = sa.index(0) + 1
        want += idx.to_bytes(4, "little")
        assert _preprocess(zlib_, "x0,3", d) == want, trial


def test_methods_1_and_2_whole_archives_without_a_gpu(zlib_, ref):
    """Levels 1 and 2 have no context model: the whole compressBlock runs on the host.  Archives identical to the
    reference's, incl. BASELINE.md's known answer (64 KiB zeros, method 1 -> 394 bytes), and they decode."""
    a = zlib_.compress_blocks([np.zeros(65536, np.uint8)], "1")[0]
    assert len(a) == 394 and hashlib.sha1(a).hexdigest() == "20fb8eb50acb4e41a6a6d455e388ffde0c7ebe4a"
    blocks = [corpus.block("text", 50000, 21), corpus.block("records", 33333, 22), _exe_like(20000, 23), corpus.block("lcg", 9000, 24)]
    for m in ("1", "2", "1,128,2"):
        ours = zlib_.compress_blocks([b.copy() for b in blocks], m)
        for b, a in zip(blocks, ours):
            assert a == ref.compress_block(b, m), m
        assert zlib_.decompress(b"".join(ours)) == b"".join(b.tobytes() for b in blocks)


def test_host_batches_shard_contiguously_over_devices(zlib_):
    """zpq_shard_range: how the engine splits a host batch when it drives several GPUs -- contiguous, ordered,
    complete, balanced to within one block (same rule as zpaq_amd.dist.shard_range)."""
    import ctypes as C
    from zpaq_amd import dist as zd
    L = zlib_.lib()
    L.zpq_shard_range.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.zpq_shard_range.restype = None
    for n in (0, 1, 7, 8, 9, 1024, 8191, 8192):
        for parts in (1, 2, 3, 4, 8):
            prev = 0
            for k in range(parts):
                lo, hi = C.c_uint64(), C.c_uint64()
                L.zpq_shard_range(n, parts, k, C.byref(lo), C.byref(hi))
                assert lo.value == prev and hi.value >= lo.value and hi.value - lo.value in (n // parts, n // parts + 1)
                assert (lo.value, hi.value) == tuple(zd.shard_range(n, k, parts))
                prev = hi.value
            assert prev == n


# ---------------------------------------------------------------------------------------------------------
# Host post-processing: the standard PCOMP programs run as C++ translated at build time (tools/gen_pcomp_std.cpp);
# ZPAQ_AMD_PCOMP=interpret forces the interpreter.  Both must produce the same bytes, for valid and for damaged streams.

def _stored_block(header, segments):
    """A block without a model (n = 0) by hand: `segments` are the payloads (the first one starts with the PP header)."""
    out = bytearray(b"7kSt\xa01\x83\xd3\x8c\xb2\x28\xb0\xd3zPQ\x02\x01") + header
    for k, payload in enumerate(segments):
        out += b"\x01" + b"s%d" % k + b"\x00\x00\x00"          # segment, filename, empty comment, reserved 0
        for at in range(0, len(payload), 65536):
            chunk = payload[at:at + 65536]
            out += len(chunk).to_bytes(4, "big") + chunk
        out += b"\x00\x00\x00\x00" + b"\xfe"                      # end of the stored payload, no checksum
    return bytes(out + b"\xff")


def test_translated_pcomp_programs_equal_the_interpreter(zlib_, ref, monkeypatch):
    import ctypes as C
    L = zlib_.lib()
    L.zpq_preprocess_block.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]

    def stream(xm, data):
        buf = np.frombuffer(bytes(data), np.uint8).copy()
        out = np.empty(len(data) * 2 + 4096, np.uint8)
        ln = C.c_size_t(0)
        assert L.zpq_preprocess_block(xm.encode(), buf.ctypes.data, buf.size, out.ctypes.data, out.size, C.byref(ln)) == 0
        return out[:ln.value].tobytes()

    def both(archive, cap):
        monkeypatch.delenv("ZPAQ_AMD_PCOMP", raising=False)
        res = []
        for interp in (False, True):
            if interp:
                monkeypatch.setenv("ZPAQ_AMD_PCOMP", "interpret")
            try:
                res.append(zlib_.decompress(archive, cap))
            except zlib_.ZpaqError as e:
                res.append(("error", e.code))
        monkeypatch.delenv("ZPAQ_AMD_PCOMP", raising=False)
        return res

    rng = np.random.default_rng(11)
    datas = [corpus.block(k, n, 7 + i).tobytes() for i, (k, n) in enumerate([("text", 70000), ("records", 50000), ("zeros", 30000),
                                                                              ("lcg", 20000), ("pattern", 40000), ("text", 1)])]
    datas.append(bytes(_exe_like(60000, 3)))
    n_native = 0
    for xm in ("x0,1,4,0,3,20", "x0,5,4,0,3,20", "x0,2,12,0,7,21", "x0,6,5,0,7,21", "x1,1,4,0,3,21", "x0,4"):
        h, pc, _ = zlib_.method_to_header(xm)
        assert h[6] == 0 and pc                                   # no model: the block is stored, the program does the work
        assert L.zpq_pcomp_is_translated(bytes(pc[2:]), len(pc) - 2, h[4], h[5]) == 1, xm
        for d in datas:
            s = stream(xm, d) if xm != "x0,4" else None
            if s is None:                                           # E8E9 only: the filtered input itself
                buf = np.frombuffer(d, np.uint8).copy()
                out = np.empty(len(d) + 4096, np.uint8); ln = C.c_size_t(0)
                L.zpq_preprocess_block(xm.encode(), buf.ctypes.data, buf.size, out.ctypes.data, out.size, C.byref(ln))
                s = buf.tobytes()
            arc = _stored_block(h, [b"\x01" + pc + s])
            a, b = both(arc, len(d) + 64)
            assert a == b == d, (xm, len(d))
            assert ref.decompress(arc, len(d) + 64) == d
            n_native += 1
            # damaged streams: whatever the interpreter makes of them, the translated program makes the same
            for _ in range(3):
                t = bytearray(s)
                if len(t) > 8:
                    for _ in range(3):
                        t[int(rng.integers(0, len(t)))] ^= 1 << int(rng.integers(0, 8))
                    t = t[:int(rng.integers(len(t) // 2, len(t)))]
                x, y = both(_stored_block(h, [b"\x01" + pc + bytes(t)]), len(d) * 4 + 4096)
                assert x == y, (xm, "damaged")
        # two segments in one block share the machine: the first runs translated, the second makes the interpreter catch up
        d1, d2 = datas[0][:30000], datas[1][:20000]
        if xm != "x0,4":
            arc = _stored_block(h, [b"\x01" + pc + stream(xm, d1), stream(xm, d2)])
            a, b = both(arc, 60000)
            assert a == b == ref.decompress(arc, 60000), xm
    # BWT (and BWT + E8E9): the methods that use it also have a model, so the program is tested on a stored block of its own
    for xm in ("x0,3ci1", "x0,7ci1"):
        _, pc, _ = zlib_.method_to_header(xm)
        h, _ = zlib_.assemble("comp 0 0 20 20 0\nhcomp\nhalt\nend\n")
        assert L.zpq_pcomp_is_translated(bytes(pc[2:]), len(pc) - 2, 20, 20) == 1, xm
        for d in datas[:5] + [datas[6]]:
            arc = _stored_block(h, [b"\x01" + pc + stream(xm, d)])
            a, b = both(arc, len(d) + 64)
            assert a == b == d, (xm, len(d))
            assert ref.decompress(arc, len(d) + 64) == d
            n_native += 1
    assert n_native >= 50
    assert L.zpq_pcomp_is_translated(b"\x38\x00", 2, 0, 20) == 0          # anything else is interpreted


def test_preprocessing_with_a_supplied_suffix_array(zlib_):
    """zpq_compress_blocks hands the LZ77 / BWT pre-processors the suffix arrays the device built for the whole batch
    (device/sa_kernels.hip).  Here the array comes from the host sorter instead -- the plumbing is the same: the stream must
    equal what the pre-processor makes when it sorts by itself, for byte-aligned and bit-packed LZ77 through a suffix
    array, BWT, and their E8E9 variants (filter first, then sort the filtered bytes)."""
    import ctypes as C
    L = zlib_.lib()
    u8p, u32p = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint32)
    L.zpq_preprocess_block.argtypes = [C.c_char_p, u8p, C.c_uint32, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.zpq_preprocess_block_sa.argtypes = [C.c_char_p, u8p, C.c_uint32, u32p, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.zpq_suffix_array_host.argtypes = [u8p, C.c_uint32, u32p]
    L.zpq_e8e9.argtypes = [u8p, C.c_uint32]
    datas = [corpus.block("text", 70000, 3), corpus.block("records", 50000, 4), _exe_like(60000, 5), corpus.block("zeros", 5000, 1),
             corpus.block("lcg", 30000, 2), corpus.block("text", 1, 9)]
    for xm in ("x0,2,12,0,7,21,1c0,0,511i2", "x0,1,4,0,7,21,1", "x0,3ci1", "x0,6,12,0,7,21,1c0,0,511i2", "x0,7ci1"):
        e8 = int(xm.split(",")[1][0]) > 4
        for d in datas:
            a = np.array(d, dtype=np.uint8, copy=True)
            b = np.array(d, dtype=np.uint8, copy=True)
            out_a, out_b = np.empty(a.size * 2 + 4096, np.uint8), np.empty(a.size * 2 + 4096, np.uint8)
            la, lb = C.c_size_t(0), C.c_size_t(0)
            assert L.zpq_preprocess_block(xm.encode(), a.ctypes.data_as(u8p), a.size, out_a.ctypes.data_as(u8p), out_a.size, C.byref(la)) == 0
            if e8:
                L.zpq_e8e9(b.ctypes.data_as(u8p), b.size)
            sa = np.empty(max(b.size, 1), np.uint32)
            assert L.zpq_suffix_array_host(b.ctypes.data_as(u8p), b.size, sa.ctypes.data_as(u32p)) == 0
            assert L.zpq_preprocess_block_sa(xm.encode(), b.ctypes.data_as(u8p), b.size, sa.ctypes.data_as(u32p),
                                             out_b.ctypes.data_as(u8p), out_b.size, C.byref(lb)) == 0
            assert la.value == lb.value and (out_a[:la.value] == out_b[:lb.value]).all(), (xm, d.size)
            assert (a == b).all()          # E8E9 left both buffers in the same (filtered) state


def test_damaged_inputs_never_crash_the_host_paths(zlib_):
    """tests/fuzz_host.py, a short round: damaged archives (stored / LZ77 / BWT blocks, decoded on the host), damaged block
    headers, random ZPAQL configs and method strings all end in a result or a ZpaqError."""
    import fuzz_host
    st = fuzz_host.run(2400, 20260926)
    assert st["decoded"] and st["rejected"] and st["plans"] and st["bad_plans"] and st["asm_ok"] and st["asm_bad"]


def test_host_paths_agree_with_the_reference_on_random_and_damaged_inputs(zlib_, ref):
    """The same generator with the reference beside it: configs assemble to the same bytes or are refused by both, method
    strings give the same header and PCOMP, damaged archives that the reference decodes decode to the same bytes (the
    documented differences: SHA-1 trailers are verified here, pre-processor types > 7 are refused here)."""
    import fuzz_host
    st = fuzz_host.run(900, 7, ref=ref)
    assert st["differences"] == [], st["differences"][:3]
    assert st.get("ref_decoded", 0) > 0


def test_stray_semicolons_in_a_program_and_unmodeled_block_headers(zlib_, ref):
    """Two findings of the differential run: compile_comp ignores a ";" between instructions (libzpaq.cpp:2686 stores only
    op <= 255), and ZPAQL::read's header checks apply to blocks without components too."""
    cfg = "comp 3 3 0 0 1\n 0 icm 5\nhcomp\n a=b ; *d=a ; halt\nend"
    assert zlib_.assemble(cfg) == ref.compile(cfg)
    a = bytearray(zlib_.compress_block(b"stored bytes", "0", "f", None))
    i = a.find(b"zPQ") + 5
    assert a[i + 6] == 0 and a[i + 7] == 0          # n = 0, COMP END
    a[i + 7] = 0x80
    with pytest.raises(zlib_.ZpaqError, match="COMP END"):
        zlib_.decompress(bytes(a))
    with pytest.raises(Exception):
        ref.decompress(bytes(a), 1 << 16)


def test_random_pcomp_programs_three_ways(zlib_, ref):
    """tests/fuzz_pcomp.py, 25 programs: random PCOMP post-processors run by the reference, by this library's interpreter
    and by the translator that serves the device (its output compiled for the host): same bytes, same failures.
    (1500 programs of seed 2 were run when this was added.)"""
    import fuzz_pcomp
    assert fuzz_pcomp.run(25, 20260926, verbose=False) == 0


def test_random_pcomp_programs_with_until_and_forward_lj(zlib_, ref):
    """The same four ways (the fourth: the device's own text for the program, pcomp_body around the translation, on the wavefront
    emulator) with every second program from fuzz_pcomp.random_program_with_forms: do .. until, forward lj out of ifs, over
    pieces of the program and out of loops.  (200 programs of seed 7 were run when this was added.)"""
    import fuzz_pcomp
    assert fuzz_pcomp.run(16, 20261018, verbose=False, forms=True) == 0


def test_two_blocks_per_wavefront_decoder_compiles_with_hiprtc(zlib_):
    """A chain nobody prebuilt (method 5 on records: periodic models that depend on the data, 29 components) through the
    run-time compiler the engine would use for it (no GPU needed)."""
    import ctypes as C
    L = zlib_.lib()
    L.zpq_plan_spec_dual_jit.restype = C.c_size_t
    L.zpq_plan_spec_dual_jit.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    h = zlib_.method_to_header(zlib_.expand_method("5", corpus.block("records", 1 << 20, 3)))[0]
    p = zlib_.Plan(h)
    log = C.create_string_buffer(8192)
    assert 20 < p.ncomp <= 32
    assert L.zpq_plan_spec_dual_jit(p._h, log, 8192) > 10000, log.value.decode()[:2000]


def test_two_swaps_in_a_row_follow_the_interpreter(zlib_, ref):
    """Found by tests/fuzz_pcomp.py: the reference's x86 JIT runs "b<>a b<>a" as ONE swap, its own interpreter (-DNOJIT, the
    ZPAQ specification: ZPAQL::run, libzpaq.cpp:1027-1262) as two.  This library -- host interpreter and the translator
    that serves the device -- follows the interpreter."""
    from oracle.oracle_py import Ref
    interp = Ref(nojit=True)
    cfg = "comp 0 0 5 6 0 hcomp halt pcomp prog ; b<>a b<>a out halt end"
    a = ref.compress_config(b"ABCDEFG", cfg, None, "f", None, False)
    assert interp.decompress(a, 100) == b"ABCDEFG\xff"
    assert zlib_.decompress(a) == b"ABCDEFG\xff"


def test_host_suffix_sorter_against_the_references_divsufsort(zlib_, ref):
    """host/preproc.cpp's SA-IS against libzpaq's own sorter (divsufsort, libzpaq.cpp:4658-6434; the compiled reference exports
    it): entry for entry, on the inputs the device sorter is compared with the host's on (tests/test_gpu_parity.py) -- so the
    device's arrays are the reference's as well, not only the archives made from them."""
    import ctypes as C
    import numpy as np
    from zpaq_amd import corpus
    L = zlib_.lib()
    u8p, u32p = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint32)
    L.zpq_suffix_array_host.argtypes = [u8p, C.c_uint32, u32p]
    kinds = ["text", "lcg", "zeros", "records", "pattern"]
    for i, n in enumerate([70000, 65536, 40000, 50001, 30000, 1, 2, 3, 255, 256, 257, 1000, 99999]):
        b = corpus.block(kinds[i % 5], n, 70 + i)
        got = np.empty(max(n, 1), np.uint32)
        assert L.zpq_suffix_array_host(b.ctypes.data_as(u8p), n, got.ctypes.data_as(u32p)) == 0
        assert (got[:n].astype(np.int64) == ref.divsufsort(b.tobytes()).astype(np.int64)).all(), (kinds[i % 5], n)


def test_device_preprocessing_hands_the_buffers_back_as_they_came(zlib_):
    """zpq_preprocess_blocks_device applies E8E9 to the CALLER's buffers before the device sorts them (compressBlock does the same,
    libzpaq.cpp:7715); when the device then declines (here: no GPU) the buffers must come back unfiltered -- a caller that falls
    back to zpq_preprocess_block would otherwise filter twice and write a stream nothing restores.  Also: a null token buffer
    with a non-zero capacity is refused."""
    import ctypes as C
    if zlib_.device_count() > 0:
        pytest.skip("a GPU is present: the device does not decline")
    L = zlib_.lib()
    L.zpq_preprocess_blocks_device.argtypes = [C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_void_p),
                                               C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    rng = np.random.default_rng(3)
    bufs = []
    for i in range(3):
        b = rng.integers(0, 256, 200000, dtype=np.uint8)
        b[::37] = 0xE8; b[4::37] = 0; b[100::53] = 0xE9; b[104::53] = 0xFF; b[3::37] = 0xE8      # (overlapping candidates too)
        bufs.append(b)
    orig = [b.copy() for b in bufs]
    outs = [np.empty(400000, np.uint8) for _ in bufs]
    n = len(bufs)
    rc = L.zpq_preprocess_blocks_device(b"x0,6,12,0,7,21,1c0,0,511i2", (C.c_void_p * n)(*[b.ctypes.data for b in bufs]),
                                        (C.c_uint32 * n)(*[b.size for b in bufs]), n, (C.c_void_p * n)(*[o.ctypes.data for o in outs]),
                                        (C.c_size_t * n)(*[o.size for o in outs]), (C.c_size_t * n)())
    assert rc != 0
    assert all((a == b).all() for a, b in zip(bufs, orig))
    L.zpq_lz77_tokens_host.argtypes = [C.c_char_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    cnt = C.c_size_t(0)
    assert L.zpq_lz77_tokens_host(b"x0,2,12,0,7,21,1", bufs[0].ctypes.data, 1000, None, 16, C.byref(cnt)) != 0


def test_encoder_variant_table(zlib_, monkeypatch):
    """The launch policy (csrc/device/launch_policy.cpp) decides what the code before it decided: every row of
    tests/golden/encoder_variant_table.json -- recorded from that code, see its "_how" -- through zpq_encoder_variants."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "encoder_variant_table.json")) as fh:
        table = json.load(fh)
    plans = {name: zlib_.Plan(bytes.fromhex(h)) for name, h in table["plans"].items()}
    knobs = sorted({k for env in table["envs"].values() for k in env})
    assert len(table["rows"]) >= 300
    seen, demoted, kept, wrong = set(), 0, 0, []
    alone = {}
    for env, cus, xcds, persist_expected, chains, want in table["rows"]:
        for k in knobs + ["ZPAQ_AMD_PIPE_PROFILE", "ZPAQ_AMD_PIPE_TRACE"]:
            monkeypatch.delenv(k, raising=False)
        for k, v in table["envs"][env].items():
            monkeypatch.setenv(k, v)           # (read at every call: the same process sees every environment)
        got = zlib_.encoder_variants([plans[c[0]] for c in chains], [c[1] for c in chains], [c[2] for c in chains], cus, xcds,
                                     bool(persist_expected))
        if got != want:
            wrong.append((env, cus, xcds, persist_expected, chains, want, got))
        seen.update(want)
        if len(chains) == 1:
            alone[(env, cus, persist_expected, tuple(chains[0]))] = want[0]
        else:
            solo = [alone.get((env, cus, persist_expected, tuple(c))) for c in chains]
            if None not in solo:
                went = any(s in (1, 3) and w == 0 for s, w in zip(solo, want))
                demoted += went
                kept += not went
    assert not wrong, (len(wrong), wrong[:10])
    # the table means something: every variant occurs, chains that share the device are demoted in some rows and not in others
    assert seen == {0, 1, 2, 3}
    assert demoted >= 1 and kept >= 1, (demoted, kept)
