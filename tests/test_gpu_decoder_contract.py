"""GPU: the catalogue of tests/decoder_contract_cases.py -- damaged, truncated, extended and capped streams -- through every
device decoder of a modelled block on the MI355X, one (chain, kernel) per test, against Oracle.decode_limited: the status, the
number of bytes and the bytes of every block, and the bytes consumed where the status is 0.  One call holds the whole catalogue,
valid and damaged streams alternating, so that every lockstep workgroup and every dual wavefront holds both; a second call on
the same Plan holds it rotated by 3 (another slot of the workgroup, the other half of the wavefront); a third holds valid streams
only, into the arenas and the LDS that the damaged batch left behind.  decode_batch allocates each output at exactly its
capacity.  The kernel that ran is asserted, so a fall-back cannot count as coverage; tests/test_emu_decoder_contract.py has
run every shape on the emulator first, and holds the catalogue to the conditions that make it mean something."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_contract_cases as dcc  # noqa: E402
from test_gpu_model_edges import ENCODER_ROUTES  # noqa: E402

pytestmark = pytest.mark.gpu

# zpq_set_kernel's value -> (zpq_plan_kernel_kind3's answer, what its note says about the decoder).  These batches are not
# dense, so 3 and 0 both take the one-block kernel's 4-block shape; its 8-block shape and the engine's own choice of the
# lockstep decoder run in test_dense_launch.
KERNELS = {1: (1, None), 2: (2, None), 3: (3, ""), 5: (3, "zpq_spec_decode2"), 6: (3, "zpq_spec_decode3"), 0: (3, "")}
PAIRS = [(n, k) for n in dcc.CHAINS for k in KERNELS
         if not (k == 5 and n in dcc.DUAL_DECLINES) and not (k == 6 and n in dcc.TEAM_DECLINES)]


class Book:
    """One chain's header, catalogue and the oracle's answers (computed once per stream and capacity)."""

    def __init__(self, z, oracle, name):
        self.h, hc = dcc.header(z, name), dcc.header(z, name, twin=True)
        self.oracle = oracle
        self.ins, self.coded, self.cases = dcc.catalogue(name, self.h, lambda d: oracle.encode(hc, d))
        self._want = {}

    def want(self, case):
        key = (case.stream, case.max_out)
        if key not in self._want:
            self._want[key] = self.oracle.decode_limited(self.h, case.stream, case.max_out)
        return self._want[key]


@pytest.fixture(scope="module")
def books(zlib_, oracle):
    return {name: Book(zlib_, oracle, name) for name in dcc.CHAINS}


def _check_call(gpu, plan, book, order, what):
    res, st = gpu.decode_batch([plan] * len(order), [c.stream for c in order], [c.max_out for c in order], check=False)
    bad = []
    for i, (c, (out, used), s) in enumerate(zip(order, res, st)):
        w = book.want(c)
        if (s, out) != (w[0], w[1]) or (s == 0 and used != w[2]):
            bad.append((i, c.name, (s, len(out), used), (w[0], len(w[1]), w[2])))
        if c.valid and c.src is not None and c.max_out > len(book.ins[c.src]):      # a valid neighbour: exact, and read to its marker
            assert (s, out, used) == (0, book.ins[c.src], len(book.coded[c.src]) + 4), (what, i, c.name, s, len(out), used)
    assert not bad, (what, len(bad), bad[:8])


def _assert_kernel(gpu, plan, kernel, nblocks):
    note = C.create_string_buffer(4096)
    kind, word = KERNELS[kernel]
    assert gpu.lib().zpq_plan_kernel_kind3(plan._h, 1, nblocks, note, 4096) == kind, (kernel, note.value)
    if word:
        assert word.encode() in note.value, note.value
    elif word == "":
        assert b"zpq_spec_decode2" not in note.value and b"zpq_spec_decode3" not in note.value, note.value


@pytest.mark.parametrize("name,kernel", PAIRS)
def test_decoder_contract(gpu, books, name, kernel):
    book = books[name]
    plan = gpu.Plan(book.h)
    gpu.set_kernel(kernel)
    try:
        first = dcc.interleave(book.cases, book.ins, book.coded, every=2)
        for k in range(0, len(first), 2):                  # every pair, and so every group of 8, holds one of each
            assert {first[k].valid, first[k + 1].valid} == {True, False}, k
        _check_call(gpu, plan, book, first, "catalogue")
        _check_call(gpu, plan, book, dcc.interleave(book.cases, book.ins, book.coded, every=2, rotate=3), "rotated by 3")
        _check_call(gpu, plan, book, [c for c in first if c.valid], "valid streams behind the damaged batches")
        _assert_kernel(gpu, plan, kernel, len(first))
    finally:
        gpu.set_kernel(0)


def test_every_pair_left_out_is_a_recorded_decline():
    assert {(n, k) for n in dcc.CHAINS for k in KERNELS} - set(PAIRS) == {(n, 5) for n in dcc.DUAL_DECLINES} | {(n, 6) for n in dcc.TEAM_DECLINES}


def test_dense_launch(gpu, books, oracle):
    """1 100 blocks of the -m5 text chain, about 300 bytes each, every 8th a damaged stream of the catalogue in turn: more than
    4 x 256 compute units' worth, so the engine picks the lockstep decoder by itself."""
    book = books["m5_text"]
    plan = gpu.Plan(book.h)
    texts = [b"\0" + dcc.corpus.block("text", 280 + 5 * s, 60 + s).tobytes() for s in range(16)]
    good = [dcc.Case(f"text{s}", oracle.encode(book.h, d) + b"\0\0\0\0", len(d) + 64, True, None) for s, d in enumerate(texts)]
    bad = [c for c in book.cases if not c.valid]
    order = [bad[(i // 8) % len(bad)] if i % 8 == 3 else good[i % len(good)] for i in range(1100)]
    assert len({c.name for c in order if not c.valid}) == len(bad)      # every damaged case is in
    note = C.create_string_buffer(4096)
    gpu.set_kernel(0)
    res, st = gpu.decode_batch([plan] * len(order), [c.stream for c in order], [c.max_out for c in order], check=False)
    assert gpu.lib().zpq_plan_kernel_kind3(plan._h, 1, len(order), note, 4096) == 3 and b"zpq_spec_decode3" in note.value, note.value
    bad_blocks = []
    for i, (c, (out, used), s) in enumerate(zip(order, res, st)):
        w = book.want(c)
        if (s, out) != (w[0], w[1]) or (s == 0 and used != w[2]):
            bad_blocks.append((i, c.name, (s, len(out), used), (w[0], len(w[1]), w[2])))
        if c.valid:
            assert (w[0], w[1], w[2]) == (0, texts[i % len(good)], len(c.stream)), c.name
    assert not bad_blocks, (len(bad_blocks), bad_blocks[:8])


@pytest.mark.parametrize("route", list(ENCODER_ROUTES))
def test_hcomp_error_through_the_encoders(gpu, zlib_, oracle, monkeypatch, route):
    """The chain whose HCOMP stops with an error at byte 255, through both shapes of the pipelined encoder as the persistent
    launch and as step kernels and through the engine's own choice: status 5 exactly for the inputs that hold the byte, the
    oracle's stream for every other block of the same batch."""
    env, persistent = ENCODER_ROUTES[route]
    for k in ("ZPAQ_AMD_PIPE_MODE", "ZPAQ_AMD_PIPE_PERSIST"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = dcc.header(zlib_, "vm_error")
    blocks = dcc.vm_error_inputs()
    plan = gpu.Plan(h)
    for rnd in range(2):                                   # the second batch into what the first left behind
        got, st, _ = gpu.encode_batch([plan] * len(blocks), [d for d, _ in blocks], check=False)
        if persistent is not None:
            assert gpu.lib().zpq_last_persistent() == persistent, (route, rnd)
        for i, ((d, at), g, s) in enumerate(zip(blocks, got, st)):
            if at is None:
                assert s == 0 and g == oracle.encode(h, d), (route, rnd, i, s)
            else:
                assert s == 5, (route, rnd, i, s)
