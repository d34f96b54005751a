"""The generic post-processor on the device: the archive's own PCOMP program, translated to HIP by host/codegen.cpp, compiled at
run time and run a lane per stream by device/pcomp_kernel.h through engine_pcomp.  zpq_pcomp_device against the host's
interpreter (zpq_pcomp_host) for hand-written programs the library has never seen -- ragged batches of 65 and 130 streams (a
second workgroup with one and two live lanes), hints that are exact, missing, too small and beyond 32 bits, outputs that force
the second attempt -- and for the standard methods' programs on valid and damaged streams; a program that stops; and the
routing of zpq_decompress over an archive that mixes everything.  Every program here ends by itself on every input: nothing
that loops or spends the device's budget of backward jumps is sent to a GPU (tests/test_emu_pcomp.py has those)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pcomp_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xC3
ROOT = os.path.dirname(HERE)
E_VM, E_UNSUPPORTED = 5, 8


@pytest.fixture(scope="module")
def wanted():
    """(program name, stream) -> the host interpreter's bytes, each computed once."""
    memo = {}

    def get(p, s):
        k = (p.name, s)
        if k not in memo:
            rc, w = pc.expected(p, s)
            assert rc == 0, (p.name, len(s), rc)
            memo[k] = w
        return memo[k]
    return get


def _decoded(gpu, code, ph, pm, streams, wants, hints, what):
    rc, bufs, sizes, status = gpu.pcomp_device(code, ph, pm, streams, [len(w) for w in wants], hints, guard=GUARD, fill=FILL)
    assert rc == 0, (what, gpu.lib().zpq_last_error().decode())
    assert status == [0] * len(streams), (what, gpu.lib().zpq_last_error().decode())
    assert sizes == [len(w) for w in wants], what
    for k, (b, w) in enumerate(zip(bufs, wants)):
        assert b[:len(w)] == w, (what, k, len(streams[k]), len(w))
        assert b[len(w):] == bytes([FILL]) * GUARD, (what, k, "a store past the capacity")


def _declined(gpu, code, ph, pm, streams, caps, hints, what):
    rc, bufs, sizes, status = gpu.pcomp_device(code, ph, pm, streams, caps, hints, guard=GUARD, fill=FILL)
    assert rc == 0, (what, rc, gpu.lib().zpq_last_error().decode())
    assert status == [1] * len(streams) and sizes == [0] * len(streams), (what, status)
    assert all(b == bytes([FILL]) * len(b) for b in bufs), (what, "a declined batch wrote something")
    return gpu.lib().zpq_last_error().decode()


@pytest.mark.parametrize("p", pc.GPU_PROGRAMS, ids=lambda p: p.name)
def test_a_program_the_library_has_not_seen(gpu, wanted, p):
    """One compile per program.  65 and 130 streams of 0 to 70 000 bytes with the hints exact, missing and too small in turn; a
    stream of 200 000 bytes whose hint is half its output (every program writes at least a byte per byte: beyond hint + 65 536,
    so the second attempt runs) beside short ones; a hint of 2^32, which the kernel's 32-bit counters cannot hold: declined."""
    code = pc.code(p)
    stop = pc.STOP_BYTE.get(p.name)
    for n in (65, 130):
        streams = list(pc.batch(n, 1, stop))
        wants = [wanted(p, s) for s in streams]
        _decoded(gpu, code, p.ph, p.pm, streams, wants, pc.hints_for(wants, "mixed"), (p.name, n))
    streams = [pc.batch(4, 1, stop)[0], pc.batch(1, 9, stop)[0] * 200, pc.batch(4, 1, stop)[3]]
    if p.name == "rle":
        streams[1] = pc.rle_forcing_a_retry()
    wants = [wanted(p, s) for s in streams]
    for kind in ("half", "zero"):
        hints = pc.hints_for(wants, kind)
        if kind == "half" or p.name == "rle":
            assert len(wants[1]) > pc.engine_cap(hints[1], len(streams[1])), (p.name, kind, "no second attempt")
        _decoded(gpu, code, p.ph, p.pm, streams, wants, hints, (p.name, "hints " + kind))
    hints = pc.hints_for(wants, "exact")
    hints[2] = pc.HINT_BEYOND_32_BITS
    assert "32-bit" in _declined(gpu, code, p.ph, p.pm, streams, [len(w) for w in wants], hints, (p.name, "hint 2^32"))


@pytest.mark.parametrize("method", pc.STD_METHODS)
def test_the_standard_programs_on_valid_and_damaged_streams(gpu, method):
    """Through the generic route (the decoders that have these programs to themselves are not asked): valid streams come back as
    their blocks; the damaged ones that tests/test_emu_pcomp.py saw end by themselves inside their arrays give the host's bytes."""
    xm, ph, pm, code = pc.std_program(method)
    streams, blocks = pc.std_valid(method)
    damaged = [(name, s) for name, s, on_gpu in pc.std_damaged(method) if on_gpu]
    assert damaged
    wants = list(blocks)
    for name, s in damaged:
        (rc, w), (rc2, w2) = pc.std_expected(method, name)
        assert rc == 0 and (rc2, w2) == (rc, w), (method, name, rc, rc2)
        wants.append(w)
    _decoded(gpu, code, ph, pm, list(streams) + [s for _, s in damaged], wants, None, method)
    _decoded(gpu, code, ph, pm, list(streams), list(blocks), [len(b) for b in blocks], (method, "exact hints"))


def test_a_batch_with_a_stream_that_stops_is_declined_as_a_whole(gpu, wanted):
    p = pc.by_name("error_on_ee")
    streams = list(pc.batch(65, 2, 0xEE))
    wants = [wanted(p, s) for s in streams]
    _decoded(gpu, pc.code(p), 0, 0, streams, wants, None, "without the byte")
    streams[37] = streams[37][:20] + b"\xee" + streams[37][20:]
    note = _declined(gpu, pc.code(p), 0, 0, streams, [len(s) + 8 for s in streams], None, "with the byte in one stream")
    assert "status 5" in note and "host" in note, note


def test_an_output_that_does_not_fit_reports_every_size(gpu, wanted):
    p = pc.by_name("delta")
    streams = [s for s in pc.batch(8) if len(s) < 70000]
    wants = [wanted(p, s) for s in streams]
    caps = [len(w) for w in wants]
    caps[0] -= 1
    rc, bufs, sizes, status = gpu.pcomp_device(pc.code(p), 0, 0, streams, caps, None, guard=GUARD, fill=FILL)
    assert rc == 3 and sizes == [len(w) for w in wants] and status == [1] * len(streams)
    assert all(b == bytes([FILL]) * len(b) for b in bufs), "an overflowing batch wrote something"


# ---- zpq_decompress ----
def test_a_program_that_stops_fails_the_call_as_the_host_alone_fails_it(gpu, monkeypatch):
    """Five blocks with the program, unforced: the device hands the group back, the host's interpreter gives the verdict."""
    good, want = pc.stopping_archive(False)
    bad, _ = pc.stopping_archive(True)
    for mode in (None, "host"):
        if mode:
            monkeypatch.setenv("ZPAQ_AMD_PCOMP", mode)
        else:
            monkeypatch.delenv("ZPAQ_AMD_PCOMP", raising=False)
        assert gpu.decompress(good) == want
        assert gpu.last_device_pcomp_segments() == (0 if mode else 5)
        with pytest.raises(gpu.ZpaqError) as ei:
            gpu.decompress(bad)
        assert ei.value.code == E_VM and "ZPAQL execution error" in str(ei.value), (mode, str(ei.value))
        assert gpu.last_device_pcomp_segments() == 0


CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import pcomp_cases as pc
import zpaq_amd as z
z.init(0)
out = {}
good, want = pc.stopping_archive(False)
out["good"] = [z.decompress(good) == want, z.last_device_pcomp_segments()]
try:
    z.decompress(pc.stopping_archive(True)[0])
    out["bad"] = [0, ""]
except z.ZpaqError as e:
    out["bad"] = [e.code, str(e)]
z.shutdown()
print("RESULT " + json.dumps(out))
"""


def test_forced_to_the_device_a_program_that_stops_is_unsupported(gpu):
    """ZPAQ_AMD_PCOMP=device leaves no host to fall back to (a fresh process: the variable is the process's)."""
    env = dict(os.environ)
    env["ZPAQ_AMD_PCOMP"] = "device"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", CHILD, ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert got["good"] == [True, 5], got
    assert got["bad"][0] == E_UNSUPPORTED and "status 5" in got["bad"][1], got


def test_routing_of_a_mixed_archive(gpu, monkeypatch):
    """Five blocks of one segment with program A, four with program B (two groups, two kernels), a block of two segments whose
    program counts in H across the boundary (one machine for both: the host's), two stored blocks without a program, interleaved:
    the nine go to the device unforced, the bytes come out in archive order and are the host route's.  Three qualifying segments
    and less than 256 KiB: none goes."""
    arch, want, n = pc.routing_archive(9)
    small, want_small, _ = pc.routing_archive(3)
    monkeypatch.setenv("ZPAQ_AMD_PCOMP", "host")
    host = gpu.decompress(arch)
    assert gpu.last_device_pcomp_segments() == 0
    assert host == want
    monkeypatch.delenv("ZPAQ_AMD_PCOMP", raising=False)
    assert gpu.decompress(arch) == host
    assert gpu.last_device_pcomp_segments() == 9
    assert gpu.decompress(small) == want_small
    assert gpu.last_device_pcomp_segments() == 0
    monkeypatch.setenv("ZPAQ_AMD_PCOMP", "device")
    assert gpu.decompress(small) == want_small
    assert gpu.last_device_pcomp_segments() == 3          # (the block of two segments stays on the host also when forced)
