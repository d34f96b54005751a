"""GPU: the chains of tests/model_edge_cases.py on the MI355X, one (chain, route) per test -- both shapes of the pipelined
encoder as the persistent launch and as step kernels, the engine's own choice, and the wavefront, dual and lockstep decoders
-- against the oracle.  What the emulator (tests/test_emu_model_edges.py: the same chains, the same inputs) cannot show is
what these are for: lanes that meet in memory run together here, tables stay resident in LDS from chunk to chunk, and the
second input set is coded with the same plan straight after the first, into state the first launch left behind.  A decoder
runs only the chains the module records as accepted (the CPU test holds the generator to those verdicts), and the kernel the
engine picked is asserted, so a silent fall-back to another decoder cannot count as coverage."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_edge_cases as mec  # noqa: E402

pytestmark = pytest.mark.gpu

# route -> (environment, persistent launch expected: 1 / 0 / None = the engine's choice)
ENCODER_ROUTES = {
    "latency-persistent": ({"ZPAQ_AMD_PIPE_MODE": "latency"}, 1),
    "throughput-persistent": ({"ZPAQ_AMD_PIPE_MODE": "throughput"}, 1),
    "latency-steps": ({"ZPAQ_AMD_PIPE_MODE": "latency", "ZPAQ_AMD_PIPE_PERSIST": "0"}, 0),
    "throughput-steps": ({"ZPAQ_AMD_PIPE_MODE": "throughput", "ZPAQ_AMD_PIPE_PERSIST": "0"}, 0),
    "auto": ({}, None),
}
FORCED_ROUTES = [r for r in ENCODER_ROUTES if r != "auto"]
# zpq_set_kernel's value -> what the note of zpq_plan_kernel_kind3 says about the decoder that was picked ("": the one-block
# wavefront kernel, whose note names neither of the other two).  These batches are not dense, so 3 and 0 both take its 4-block
# shape; the 8-block shape runs on the device in tests/test_gpu_parity.py, not here.
DECODER_ROUTES = {3: "", 5: "zpq_spec_decode2", 6: "zpq_spec_decode3", 0: ""}
MI355X_CUS, MI355X_XCDS = 256, 8          # the device of this suite, for the launch policy's own answer (zpq_encoder_variants)
DECODER_PAIRS = [(name, k) for name in mec.NAMES for k in DECODER_ROUTES
                 if not (k == 5 and name in mec.DUAL_DECLINES) and not (k == 6 and name in mec.TEAM_DECLINES)]


@pytest.fixture(scope="module")
def want(zlib_, oracle):
    """name -> (header, [first set coded by the oracle], [second set coded by the oracle]): once, shared by every route."""
    out = {}
    for name in mec.NAMES:
        h = mec.header(zlib_, name)
        out[name] = (h, [oracle.encode(h, d) for d in mec.first_inputs()], [oracle.encode(h, d) for d in mec.second_inputs()])
    return out


def _encode_route(gpu, monkeypatch, route, header, sets):
    """Every (inputs, expected streams) of `sets` through one Plan, one set straight after the other."""
    env, persistent = ENCODER_ROUTES[route]
    for k in ("ZPAQ_AMD_PIPE_MODE", "ZPAQ_AMD_PIPE_PERSIST"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = gpu.Plan(header)
    for s, (inputs, coded) in enumerate(sets):
        got = gpu.encode_batch([plan] * len(inputs), inputs)
        if persistent is not None:
            assert gpu.lib().zpq_last_persistent() == persistent, (route, s)
        for i, (g, w) in enumerate(zip(got, coded)):
            assert g == w, (route, s, i, len(g), len(w))
    return plan


def _decode_route(gpu, kernel, header, sets):
    note = C.create_string_buffer(4096)
    plan = gpu.Plan(header)
    gpu.set_kernel(kernel)
    try:
        for s, (inputs, coded) in enumerate(sets):
            back = gpu.decode_batch([plan] * len(inputs), [c + b"\0\0\0\0" for c in coded], [len(d) + 8 for d in inputs])
            for i, ((plain, used), d, c) in enumerate(zip(back, inputs, coded)):
                assert plain == d and used == len(c) + 4, (kernel, s, i, len(plain), len(d), used, len(c))
        # a per-header kernel, never the generic one (kind 2: what the engine falls to without a sound), and the wanted one
        assert gpu.lib().zpq_plan_kernel_kind3(plan._h, 1, len(sets[0][0]), note, 4096) == 3, note.value
        if DECODER_ROUTES[kernel]:
            assert DECODER_ROUTES[kernel].encode() in note.value, note.value
        else:
            assert b"zpq_spec_decode2" not in note.value and b"zpq_spec_decode3" not in note.value, note.value
    finally:
        gpu.set_kernel(0)
    return plan


@pytest.mark.parametrize("route", list(ENCODER_ROUTES))
@pytest.mark.parametrize("name", mec.NAMES)
def test_edge_chain_encoder(gpu, want, monkeypatch, name, route):
    header, c1, c2 = want[name]
    sets = [(mec.first_inputs(), c1), (mec.second_inputs(), c2)]
    plan = _encode_route(gpu, monkeypatch, route, header, sets)
    if route == "auto":
        # nothing forced: the pipelined encoder in the persistent launch, and -- the one shape no forced route reaches -- the
        # latency shape with a wavefront per SIMD (variant 3) for every chain that is not small (variant 1 is that shape there)
        note = C.create_string_buffer(4096)
        for inputs, _ in sets:
            assert gpu.lib().zpq_plan_kernel_kind3(plan._h, 0, len(inputs), note, 4096) == 4, note.value
            got = gpu.encoder_variants([plan], [len(inputs)], [max(len(d) for d in inputs)], MI355X_CUS, MI355X_XCDS)
            assert got == [1 if mec.FORMS[name]["small1"] else 3], (name, got)
        assert gpu.lib().zpq_last_persistent() == 1


@pytest.mark.parametrize("name,kernel", DECODER_PAIRS)
def test_edge_chain_decoder(gpu, want, name, kernel):
    header, c1, c2 = want[name]
    _decode_route(gpu, kernel, header, [(mec.first_inputs(), c1), (mec.second_inputs(), c2)])


def test_every_pair_left_out_is_a_recorded_decline():
    left_out = {(n, k) for n in mec.NAMES for k in DECODER_ROUTES} - set(DECODER_PAIRS)
    assert left_out == {("above", 6), ("h11", 6), ("wide_mix", 6), ("wide_mix", 5)}


def test_dense_decode_launch_takes_the_lockstep_decoder_for_a_one_word_cm(gpu, want):
    """A decode launch that fills the machine picks the lockstep decoder by itself (engine.cpp kernel_kind): the chains whose
    one-word CM it used to get wrong are among those it takes, so a valid archive was reported as damaged."""
    note = C.create_string_buffer(4096)
    for name in ("one_word", "tiny0"):
        plan = gpu.Plan(want[name][0])
        assert gpu.lib().zpq_plan_kernel_kind3(plan._h, 1, 2048, note, 4096) == 3, note.value
        assert b"zpq_spec_decode3" in note.value, note.value


@pytest.fixture(scope="module")
def stress(zlib_, oracle):
    h = zlib_.assemble(mec.PIPE_STRESS_CFG)[0]
    sets = [[b"\0" + d for d in part] for part in mec.stress_inputs()]
    return h, [(s, [oracle.encode(h, d) for d in s]) for s in sets]


@pytest.mark.parametrize("route", FORCED_ROUTES)
def test_stress_config_encoder(gpu, stress, monkeypatch, route):
    """PIPE_STRESS_CFG with its `datas`, `more` and `fit` inputs (tests/test_emu.py runs them on the emulator)."""
    _encode_route(gpu, monkeypatch, route, *stress)


@pytest.mark.parametrize("kernel", list(DECODER_ROUTES))
def test_stress_config_decoder(gpu, stress, kernel):
    _decode_route(gpu, kernel, *stress)


@pytest.mark.parametrize("route", FORCED_ROUTES)
def test_match_ring_config_encoder(gpu, zlib_, oracle, monkeypatch, route):
    """MATCH_RING_CFG with its eight blocks around the ring's end."""
    h = zlib_.assemble(mec.MATCH_RING_CFG)[0]
    datas = mec.match_ring_inputs()
    _encode_route(gpu, monkeypatch, route, h, [(datas, [oracle.encode(h, d) for d in datas])])
