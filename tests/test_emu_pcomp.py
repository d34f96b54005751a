"""The device's generic post-processor on the wavefront emulator (tests/emu/pcomp_emu_main.cpp): the text zpq_pcomp_source
generates for a PCOMP program -- device/pcomp_kernel.h's pcomp_body and PcompOut around the program as host/codegen.cpp
translates it -- must write, byte for byte, what the host's interpreter writes (zpq_pcomp_host), which is held here to the
reference's interpreter.  Every lane's M, H, R, input and output lie at their exact sizes between inaccessible pages; the
batches are ragged (0 to 70 000 bytes in one wavefront, 1 to 130 streams), the lanes run in order and reversed, the capacities
are the engine's, and where an output goes beyond its capacity the second attempt is made as the engine makes it.  No GPU."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))
import pcomp_cases as pc  # noqa: E402
import pcomp_emu  # noqa: E402

E_VM = 5            # ZPQ_E_VM, and the status the device program stops with


def _order(monkeypatch, order):
    if order:
        monkeypatch.setenv("ZPQ_EMU_ORDER", order)
    else:
        monkeypatch.delenv("ZPQ_EMU_ORDER", raising=False)


@pytest.fixture(scope="module")
def wanted():
    """(program name, stream) -> the host interpreter's bytes, each computed once."""
    memo = {}

    def get(p, s):
        k = (p.name, s)
        if k not in memo:
            memo[k] = pc.expected(p, s)
        return memo[k]
    return get


@pytest.mark.parametrize("p", pc.PROGRAMS, ids=lambda p: p.name)
def test_the_host_interpreter_is_the_reference_interpreter(zlib_, ref, p):
    """A stored block that carries the program, written by the reference: the reference's interpreter (built without its JIT: the
    JIT runs two swaps in a row as one, tests/fuzz_pcomp.py), zpq_decompress and zpq_pcomp_host give the same bytes -- or all fail."""
    from oracle.oracle_py import Ref
    interp = Ref(nojit=True)
    stop = pc.STOP_BYTE.get(p.name)
    b = pc.batch(4, 3, stop)
    datas = [b[0] + b[3] + b[2][:3000] + bytes(range(256)).replace(bytes([stop]) if stop is not None else b"-", b"") + b[0][:7], b""]
    if stop is not None:
        datas.append(b[0][:100] + bytes([stop]) + b[0][:50])
    for k, data in enumerate(datas):
        arch = ref.compress_config(data, pc.config(p), None, "f", None, False)
        try:
            want = interp.decompress(arch, 64 << 20)
        except Exception:
            want = None
        assert (want is None) == (stop is not None and k == 2), (p.name, k)
        rc, got = pc.expected(p, data)
        try:
            mine = zlib_.decompress(arch, cap=64 << 20)
        except zlib_.ZpaqError as e:
            assert e.code == E_VM, e
            mine = None
        assert mine == want, (p.name, k, "zpq_decompress")
        assert (rc, got) == ((0, want) if want is not None else (E_VM, b"")), (p.name, k, "zpq_pcomp_host", rc)


@pytest.mark.parametrize("order", ["", "reverse"])
@pytest.mark.parametrize("p", pc.PROGRAMS, ids=lambda p: p.name)
def test_every_program_writes_what_the_interpreter_writes(zlib_, monkeypatch, wanted, p, order):
    _order(monkeypatch, order)
    code = pc.code(p)
    exe = pcomp_emu.build(code, p.ph, p.pm)
    for n in pc.BATCHES if not order else pc.BATCHES[-2:]:
        streams = list(pc.batch(n, 1, pc.STOP_BYTE.get(p.name)))
        if n >= 4:
            assert {len(s) for s in streams} >= ({0, 1, 1000, 70000} if n == 4 else {0, 1, 2, 63, 64, 65, 1000, 70000})
        want = []
        for s in streams:
            rc, w = wanted(p, s)
            assert rc == 0, (p.name, len(s))
            want.append(w)
        hints = pc.hints_for(want, "mixed")
        outs, status, retried = pcomp_emu.run(code, p.ph, p.pm, streams, hints, exe=exe)
        assert outs is not None and status == [0] * n, (p.name, n, status)
        for k, (o, w) in enumerate(zip(outs, want)):
            assert len(o) == len(w) and o == w, (p.name, n, k, len(streams[k]), len(o), len(w))
        # the second attempt is made exactly where the first capacity was too small
        assert retried == [k for k in range(n) if len(want[k]) > pc.engine_cap(hints[k], len(streams[k]))], (p.name, n)


def test_the_expander_forces_the_second_attempt(zlib_, monkeypatch, wanted):
    """255 000 bytes from 2 000: beyond 8 * in_len + 65 536 without a hint and beyond half the size + 65 536 with a hint too small
    by half; an exact hint needs one attempt.  Beside a stream that fits."""
    _order(monkeypatch, "")
    p = pc.by_name("rle")
    s = pc.rle_forcing_a_retry()
    rc, w = wanted(p, s)
    assert rc == 0 and len(w) == 255000 and len(w) > 8 * len(s) + 65536
    small = pc.batch(4)[0]
    ws = wanted(p, small)[1]
    for kind, retry in (("zero", [1]), ("half", [1]), ("exact", [])):
        hints = pc.hints_for([ws, w, ws], kind)
        outs, status, retried = pcomp_emu.run(pc.code(p), p.ph, p.pm, [small, s, small], hints)
        assert status == [0, 0, 0] and outs == [ws, w, ws], kind
        assert retried == retry, kind
    assert pc.engine_declines_cap(pc.engine_cap(pc.HINT_BEYOND_32_BITS, len(s)))
    assert pcomp_emu.run(pc.code(p), p.ph, p.pm, [small, s], [0, pc.HINT_BEYOND_32_BITS])[0] is None


@pytest.mark.parametrize("name", ["cat", "rle", "reverse", "delta"])
def test_a_capacity_one_byte_short_reports_the_size_and_stores_nothing_beyond(zlib_, monkeypatch, wanted, name):
    """PcompOut counts what it does not store: result[0] is the whole size, the buffer holds its first cap bytes, and the byte
    behind the buffer is an inaccessible page."""
    _order(monkeypatch, "")
    p = pc.by_name(name)
    streams = [s for s in pc.batch(8) if len(s) and len(s) < 70000]
    streams = [s for s in streams if len(wanted(p, s)[1])]
    want = [wanted(p, s)[1] for s in streams]
    exe = pcomp_emu.build(pc.code(p), p.ph, p.pm)
    for short in (1, None):
        caps = [len(w) - short if short else 0 for w in want]
        res = pcomp_emu.launch(exe, p.ph, p.pm, streams, caps)
        for (n, status, kept), w, c in zip(res, want, caps):
            assert (n, status) == (len(w), 0) and kept == w[:c], (name, short, n, len(w))
    res = pcomp_emu.launch(exe, p.ph, p.pm, streams, [len(w) for w in want])          # exactly enough: all of it
    assert [r[2] for r in res] == want


@pytest.mark.parametrize("name", sorted(pc.STOP_BYTE))
def test_a_program_that_stops_is_reported_by_its_lane_alone(zlib_, monkeypatch, wanted, name):
    """`error` executed, or a jump out of the program: status 5 from the lane that met the byte, 0 and whole outputs from its
    neighbours -- the engine hands such a batch back -- and ZPQ_E_VM from the host."""
    _order(monkeypatch, "")
    p = pc.by_name(name)
    stop = pc.STOP_BYTE[name]
    streams = list(pc.batch(65, 2, stop))
    bad = 37
    streams[bad] = streams[bad][:20] + bytes([stop]) + streams[bad][20:]
    exe = pcomp_emu.build(pc.code(p), p.ph, p.pm)
    res = pcomp_emu.launch(exe, p.ph, p.pm, streams, [pc.engine_cap(0, len(s)) for s in streams])
    for k, (n, status, kept) in enumerate(res):
        if k == bad:
            assert status == E_VM and kept == streams[bad][:20], (name, status, n)
        else:
            assert status == 0 and kept == wanted(p, streams[k])[1], (name, k)
    assert pcomp_emu.run(pc.code(p), p.ph, p.pm, streams, exe=exe)[0] is None
    assert pc.expected(p, streams[bad]) == (E_VM, b"")


def test_a_loop_without_an_exit_ends_by_the_budget_here_and_by_the_step_limit_on_the_host(zlib_, monkeypatch):
    """CPU only: the translated program gives up after its budget of backward jumps (a backward lj counts as one), the interpreter
    at its step limit.  Neither is a verdict the other has to share; the engine sends a status to the host."""
    _order(monkeypatch, "")
    p = pc.NO_EXIT
    exe = pcomp_emu.build(pc.code(p), p.ph, p.pm)
    res = pcomp_emu.launch(exe, p.ph, p.pm, [b"x", b""], [16, 16], timeout=120)
    assert [(n, status) for n, status, _ in res] == [(0, E_VM), (0, E_VM)]
    L = zlib_.lib()
    import ctypes as C
    L.zpq_set_pcomp_step_limit.argtypes = [C.c_uint64]
    L.zpq_set_pcomp_step_limit.restype = None
    L.zpq_set_pcomp_step_limit(1 << 20)
    try:
        assert pc.expected(p, b"x") == (E_VM, b"")
    finally:
        L.zpq_set_pcomp_step_limit(0)


@pytest.mark.parametrize("order", ["", "reverse"])
@pytest.mark.parametrize("method", pc.STD_METHODS)
def test_the_standard_programs_on_valid_and_damaged_streams(zlib_, monkeypatch, method, order):
    """The programs of the standard methods as zpq_method_to_header gives them.  Valid streams come back as their blocks, as
    zpq_postprocess_block and zpq_pcomp_host give them.  Damaged streams stay inside every lane's arrays (the guard pages say so:
    every M and H index is masked), and those flagged for the GPU end with status 0 and the host's bytes; a lane that reports a
    status is the host's business."""
    _order(monkeypatch, order)
    xm, ph, pm, code = pc.std_program(method)
    exe = pcomp_emu.build(code, ph, pm)
    streams, blocks = pc.std_valid(method)
    for s, b in zip(streams, blocks):
        rc, out, _ = zlib_.postprocess_block(xm, s)
        assert rc == 0 and out == b
        assert zlib_.pcomp_host(code, ph, pm, s)[:2] == (0, b)
    outs, status, retried = pcomp_emu.run(code, ph, pm, list(streams), [len(b) for b in blocks], exe=exe)
    assert outs == list(blocks) and retried == []
    outs, status, retried = pcomp_emu.run(code, ph, pm, list(streams), None, exe=exe)
    assert outs == list(blocks)
    damaged = pc.std_damaged(method)
    ds = [s for _, s, _ in damaged]
    res = pcomp_emu.launch(exe, ph, pm, [streams[0]] + ds + [streams[-1]], [pc.engine_cap(0, len(s)) for s in [streams[0]] + ds + [streams[-1]]])
    assert res[0][1:] == (0, blocks[0]) and res[-1][1:] == (0, blocks[-1])
    for (name, s, gpu), (n, status, kept) in zip(damaged, res[1:-1]):
        (rc, want), (rc2, want2) = pc.std_expected(method, name)
        assert rc in (0, E_VM) and (rc2, want2) == (rc, want), (method, name, rc, rc2)
        assert status in (0, E_VM), (method, name, status)
        if status == 0:
            assert rc == 0 and n == len(want) and kept == want, (method, name, n, len(want))
        assert gpu == (status == 0), (method, name, "pcomp_cases.std_damaged flags it %s for the GPU, the device program's status is %d" % (gpu, status))


def test_the_entries_exist_and_decline_without_a_device(zlib_):
    z = zlib_
    assert isinstance(z.last_device_pcomp_segments(), int)
    p = pc.by_name("delta")
    streams = list(pc.batch(4))
    want = [pc.expected(p, s)[1] for s in streams]
    rc, bufs, sizes, status = z.pcomp_device(pc.code(p), p.ph, p.pm, streams, [len(w) for w in want])
    if rc == 0:
        assert status == [0] * 4 and bufs == want and sizes == [len(w) for w in want]
    else:
        assert rc == 8 and b"device" in z.lib().zpq_last_error(), (rc, z.lib().zpq_last_error())
        assert status == [1] * 4 and sizes == [0] * 4
    # the host entry: sizes also when the buffer is too small, the program's own error as ZPQ_E_VM
    assert z.pcomp_host(pc.code(p), p.ph, p.pm, streams[0], cap=10) == (3, b"", len(want[0]))
    e = pc.by_name("error_on_ee")
    assert z.pcomp_host(pc.code(e), 0, 0, b"ab\xeecd") == (E_VM, b"", 0)


def test_the_hand_built_archives_are_what_the_reference_decodes(zlib_, ref):
    """tests/pcomp_cases.py writes its archives of stored blocks byte by byte (blocks of one and of two segments, with and without
    a program, with and without checksums): the reference's interpreter and zpq_decompress read them alike, and the program
    that stops fails both."""
    from oracle.oracle_py import Ref
    interp = Ref(nojit=True)
    for arch, want in (pc.routing_archive(9)[:2], pc.routing_archive(3)[:2], pc.stopping_archive(False)):
        assert interp.decompress(arch, 1 << 20) == want
        assert zlib_.decompress(arch) == want
    bad = pc.stopping_archive(True)[0]
    with pytest.raises(RuntimeError, match="ZPAQL execution error"):
        interp.decompress(bad, 1 << 20)
    with pytest.raises(zlib_.ZpaqError) as ei:
        zlib_.decompress(bad)
    assert ei.value.code == E_VM
