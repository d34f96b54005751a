"""CPU (-m "not gpu"): what the device decoders of a modelled block do with a stream that is not valid, or with a capacity below
the block -- the catalogue of tests/decoder_contract_cases.py against Oracle.decode_limited.  Here: the oracle's new function
against the old one and, where oracle/_ref is built, its verdict "corrupt" against the reference's; the conditions that keep
the catalogue from hiding a failure; every chain's catalogue through the emulated one-block kernel in both workgroup shapes,
the dual and the lockstep decoder, good and damaged streams side by side in every workgroup; and the chain whose HCOMP stops
with an error through every emulated encoder.  tests/test_gpu_decoder_contract.py runs the same catalogue on the MI355X."""
import collections
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_contract_cases as dcc  # noqa: E402
import emu  # noqa: E402
import model_edge_cases as mec  # noqa: E402
from oracle.oracle_py import parse_block  # noqa: E402


@pytest.fixture(scope="module")
def book(zlib_, oracle):
    """name -> (header, inputs, coded, cases, {case name: decode_limited's answer}): once, shared by every test."""
    out = {}
    for name in dcc.CHAINS:
        h, hc = dcc.header(zlib_, name), dcc.header(zlib_, name, twin=True)
        ins, coded, cases = dcc.catalogue(name, h, lambda d: oracle.encode(hc, d))
        assert len({c.name for c in cases}) == len(cases)
        out[name] = (h, ins, coded, cases, {c.name: oracle.decode_limited(h, c.stream, c.max_out) for c in cases})
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle

@pytest.mark.parametrize("name", dcc.CHAINS)
def test_decode_limited_equals_decode_on_valid_streams(book, oracle, name):
    h, ins, coded, _, _ = book[name]
    for d, c in zip(ins + [b"", b"\0"], coded + [oracle.encode(h, b""), oracle.encode(h, b"\0")]):
        good = c + b"\0\0\0\0"
        plain, used = oracle.decode(h, good, len(d) + 8)
        assert (plain, used) == (d, len(good))
        assert oracle.decode_limited(h, good, len(d) + 8) == (0, d, len(good))
        assert oracle.decode_limited(h, good + b"\x55" * 9, len(d) + 1) == (0, d, len(good))
        for cap in sorted({0, 1, len(d) // 2, len(d) - 1, len(d)} & set(range(len(d) + 1))):
            assert oracle.decode_limited(h, good, cap) == (0, d[:cap], 0), cap      # the prefix; at cap == len(d): before the marker


def test_decode_limited_agrees_with_decode_outcome_on_damage(book, oracle):
    """Where the old yardstick has an opinion -- the status, and the bytes at status 0 -- the new one shares it."""
    for name in dcc.CHAINS:
        h, _, _, cases, _ = book[name]
        for c in cases:
            st, out, _ = oracle.decode_limited(h, c.stream, 1 << 16)
            if name == "vm_error" and st == 5:
                with pytest.raises(RuntimeError, match="zo_decode failed: -5"):
                    oracle.decode_outcome(h, c.stream, 1 << 16)
                continue
            if st == 0 and len(out) == 1 << 16:
                continue                                   # (the all-ff streams: no end within any capacity)
            old = oracle.decode_outcome(h, c.stream, 1 << 16)
            assert old[0] == st and (st != 0 or old[1] == out), (name, c.name)


def _ref_archive(zlib_, ref, name, data):
    if name in ("m5_text", "m5_records"):
        kind = "text" if name == "m5_text" else "records"
        return ref.compress_block(data, zlib_.expand_method("5", dcc.corpus.block(kind, 1 << 20, dcc.corpus.BASE_SEED)))
    if name == "deep_isse":
        return ref.compress_block(data, mec.DEEP_ISSE)
    return ref.compress_config(data, {"pipe_stress": mec.PIPE_STRESS_CFG, "one_word": mec.ONE_WORD_CFG, "vm_error": dcc.VM_ERROR_CFG}[name])


@pytest.mark.parametrize("name", dcc.CHAINS)
def test_corrupt_verdicts_against_the_reference(book, zlib_, ref, name):
    """Every case that the oracle ends with status 2, its first decoded byte (if any) 0 as the post-processor wants it: put in
    place of the good payload in the reference's own archive of the same data, it must make the reference raise "archive
    corrupted" (libzpaq.cpp:2108) or "decoding end of stream" (2134).  The reference meets the same bytes in the same order up
    to that point, so what follows the payload cannot matter.  (Status 6 and the capacities are not comparable this way: in a
    frame the reference reads the segment trailer where a bare payload ends.)"""
    h, ins, coded, cases, want = book[name]
    frames = []
    for d, c in zip(ins, coded):
        a = _ref_archive(zlib_, ref, name, d[1:])
        f = parse_block(a)
        ps, good = f["payload_start"], c + b"\0\0\0\0"
        assert f["header"] == h and a[ps:ps + len(good)] == good, name      # the same chain, the same stream
        assert ref.decompress(a, len(d) + 64) == d[1:]
        frames.append((a[:ps], a[ps + len(good):]))
    checked = 0
    for c in cases:
        st, out, _ = want[c.name]
        if st != 2 or (out and out[0] != 0):
            continue
        head, tail = frames[c.src if c.src is not None else 0]
        with pytest.raises(RuntimeError, match="archive corrupted|decoding end of stream"):
            ref.decompress(head + c.stream + tail, 1 << 16)
        checked += 1
    assert checked >= 5, checked


# ---------------------------------------------------------------------------------------------------------------------------
# the catalogue

def _verdict(fn, header):
    try:
        return fn(header)
    except RuntimeError as ex:
        return str(ex)


@pytest.mark.parametrize("name", dcc.CHAINS)
def test_which_decoders_take_the_chain(book, name):
    h = book[name][0]
    dual = _verdict(emu.dual_source, h)
    team = _verdict(emu.team_source, h)
    got = {"dual": True if "zpq_spec_decode2" in dual else dual, "team": emu.team_threads(team) if "zpq_spec_decode3" in team else team}
    assert got == dcc.TAKES[name]
    assert {dcc.TAKES[n]["team"] for n in dcc.CHAINS if n not in dcc.TEAM_DECLINES} == {384, 512}      # both workgroup shapes


@pytest.mark.parametrize("name", dcc.CHAINS)
def test_catalogue_conditions(book, name):
    h, ins, coded, cases, want = book[name]
    assert all(len(d) <= 1536 and d[:1] == b"\0" for d in ins) and all(len(c.stream) <= 1536 for c in cases)
    cl = collections.Counter(dcc.classify(c, ins, want[c.name]) for c in cases)
    print(name, len(cases), dict(cl))
    assert cl["corrupt"] and cl["end of input"] and cl["end of stream"] and cl["capacity"], cl
    assert cl["capacity, garbage"] >= 8, cl
    for c in cases:
        st, out, used = want[c.name]
        assert len(out) <= c.max_out
        if c.valid:                                        # exact, whatever follows the marker
            d = ins[c.src] if c.src is not None else b""
            n = len(coded[c.src]) + 4 if c.src is not None else 8
            assert (st, out, used) == (0, d[:c.max_out], n if c.max_out > len(d) else 0), c.name
    assert want["zeros600"] == (2, b"", 0)
    assert want["empty_block"] == (0, b"", 8)
    assert want["ff600.below"] == (0, bytes(20), 0) and want["ff600.cap1500"] == (0, bytes(1500), 0)
    assert want["ff4"][0] == 6 and 0 < len(want["ff4"][1]) < 1 << 15 and not any(want["ff4"][1])      # every bit 0 until the input ends
    if name in dcc.LOW_ZERO:                               # status 2 on the bit behind the shift, inside the input
        seed, emitted = dcc.LOW_ZERO[name]
        st, out, _ = want["low_zero"]
        assert st == 2 and out == dcc.low_zero_input(seed)[:len(out)] and 0 < len(out) < 48, (st, len(out))
    if name == "vm_error":
        planned = {f"hcomp{i}": (d, at) for i, (d, at) in enumerate(dcc.vm_error_inputs())}
        through_garbage = [c.name for c in cases if want[c.name][0] == 5 and c.name not in planned]
        assert through_garbage and all(not c.valid for c in cases if want[c.name][0] == 5), through_garbage
        assert all(dcc.ERROR_BYTE not in want[c.name][1] for c in cases)
        for key, (d, at) in planned.items():               # the catalogue's own outcomes: out_len = the index of the offending byte
            st, out, used = want[key]
            assert (st, out) == ((0, d) if at is None else (5, d[:at])), key
        assert {at for _, at in planned.values()} >= {None, 0, 1, 64, 65, 299}
        assert {len(d) for d, at in planned.values() if at is None} >= {0, 300}


# ---------------------------------------------------------------------------------------------------------------------------
# the emulated decoders

DECODERS = {"wavefront4": dict(waves=4), "wavefront8": dict(waves=8), "dual": dict(dual=True), "lockstep": dict(team=True)}
DECODER_PAIRS = [(n, k) for n in dcc.CHAINS for k in DECODERS
                 if not (k == "dual" and n in dcc.DUAL_DECLINES) and not (k == "lockstep" and n in dcc.TEAM_DECLINES)]


@pytest.mark.parametrize("name,decoder", DECODER_PAIRS)
def test_emulated_decoder(book, oracle, name, decoder):
    """One run holds the whole catalogue with a capacity per block, a valid stream in every fourth slot: every lockstep
    workgroup of 8 and every workgroup of the wavefront kernels holds both kinds, and every other dual wavefront."""
    h, ins, coded, cases, want = book[name]
    order = dcc.interleave(cases, ins, coded, every=4)
    res = emu.run(h, [c.stream for c in order], decode=True, out_cap=[c.max_out for c in order], **DECODERS[decoder])
    bad = []
    for c, (out, st, used) in zip(order, res):
        w = want.get(c.name) or oracle.decode_limited(h, c.stream, c.max_out)
        if (st, out) != (w[0], w[1]) or (st == 0 and used != w[2]):
            bad.append((c.name, (st, len(out), used), (w[0], len(w[1]), w[2])))
    assert not bad, bad[:8]


# ---------------------------------------------------------------------------------------------------------------------------
# HCOMP's error through the emulated encoders

@pytest.fixture(scope="module")
def vm_blocks(zlib_, oracle):
    h = dcc.header(zlib_, "vm_error")
    return h, [(d, at, None if at is not None else oracle.encode(h, d)) for d, at in dcc.vm_error_inputs()]


def _check_vm_encoder(res, blocks, what):
    for i, ((d, at, stream), (got, status, _)) in enumerate(zip(blocks, res)):
        if at is None:
            assert status == 0 and got == stream, (what, i, status)      # a neighbour's error changes nothing here
        else:
            assert status == 5, (what, i, status)


def test_vm_error_through_the_wavefront_encoder(vm_blocks):
    h, blocks = vm_blocks
    for waves in (4, 8):
        _check_vm_encoder(emu.run(h, [d for d, _, _ in blocks], waves=waves), blocks, waves)


@pytest.mark.parametrize("persist", [False, True], ids=["steps", "persistent"])
@pytest.mark.parametrize("mode", [0, 1], ids=["throughput", "latency"])
def test_vm_error_through_the_pipelined_encoder(vm_blocks, mode, persist):
    """The HCOMP unit stops for the block and idles from the next chunk on; the coder unit reads its status at the end.  In the
    persistent launch the other units must still finish: this run is where that shows, before any device sees the chain."""
    h, blocks = vm_blocks
    _check_vm_encoder(emu.pipe_run(h, [d for d, _, _ in blocks], chunk=64, mode=mode, persist=persist), blocks, (mode, persist))
