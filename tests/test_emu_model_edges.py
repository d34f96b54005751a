"""CPU (-m "not gpu"): the chains of tests/model_edge_cases.py -- component parameters on both sides of every threshold at
which the generator and the device headers choose another unit form.  Per chain: the generated sources must show the forms
the module records (a threshold that moves fails here before a form drops out of what runs on the GPU), and the emulator must
give the oracle's bytes through both shapes of the pipelined encoder, as step kernels and as the persistent launch, and
through every decoder that takes the chain.  tests/test_gpu_model_edges.py runs the same chains on the MI355X."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emu  # noqa: E402
import model_edge_cases as mec  # noqa: E402


def _const(src, name):
    m = re.search(r"\b%s = (-?\w+)" % name, src)
    assert m, name
    v = m.group(1)
    return {"true": True, "false": False}.get(v, v if not v.lstrip("-").isdigit() else int(v))


def _array(src, name):
    m = re.search(r"\b%s\[\d+\] = \{([^}]*)\}" % name, src)
    assert m, name
    return [int(x) for x in m.group(1).split(",")]


def _verdict(fn, header):
    try:
        return fn(header)
    except RuntimeError as ex:
        return str(ex)


def forms(header):
    """What the generated sources say about the forms a chain takes (keys as in model_edge_cases.FORMS)."""
    src = {m: emu.pipe_source(header, 64, mode=m) for m in (0, 1, 3)}
    f = {}
    for key, name in (("lanes", "HCOMP_LANES"), ("h_lds", "HCOMP_H_LDS"), ("m_lds", "HCOMP_M_LDS")):
        vals = {_const(s, name) for s in src.values()}
        assert len(vals) == 1, (name, vals)              # HCOMP's form does not depend on the encoder's shape
        f[key] = vals.pop()
    for m, s in src.items():
        f["bits%d" % m] = tuple(sorted({k for k in _array(s, "LIGHT_KIND") if k >= 9}))      # 9 CM, 10 MIX2, 11 SSE with a lane per bit position
        f["mix_bits%d" % m] = _const(s, "MIX_BITS")
        assert "PIPE_PERSIST = true" in s, m             # every chain here packs into the persistent launch
    f["nh0"] = _const(src[0], "PS_MIX_NH")
    f["ql"] = tuple(_array(src[0], "MIX_QL")) if _const(src[0], "NMIXR") else ()
    f["waves1"] = _const(src[1], "PS_WAVES")
    # the latency shape of a chain that is NOT small says so in one line (codegen.cpp generate_pipe_source); the line is
    # looked for in both wordings it can have, so that a rewording fails here instead of turning every chain "small"
    assert _const(src[1], "PS_SMALL") is True
    halves = re.search(r"\bPS_ROW_HALVES = (true|false)", src[1])
    assert halves is None or halves.group(1) == "false", halves.group(0)
    f["small1"] = halves is None
    f["dec_h_lds"] = _const(emu.kernel_source(header, 8), "H_LDS") >= 0
    dual = _verdict(emu.dual_source, header)
    f["dual"] = True if "zpq_spec_decode2" in dual else dual
    team = _verdict(emu.team_source, header)
    f["team"] = emu.team_threads(team) if "zpq_spec_decode3" in team else team
    return f


@pytest.fixture(scope="module")
def headers(zlib_):
    return {name: mec.header(zlib_, name) for name in mec.NAMES}


@pytest.fixture(scope="module")
def coded(headers, oracle):
    """name -> [(input, the oracle's coded stream)] of the first input set: computed once, shared by the routes."""
    return {name: [(d, oracle.encode(h, d)) for d in mec.first_inputs()] for name, h in headers.items()}


@pytest.mark.parametrize("name", mec.NAMES)
def test_forms_and_verdicts(headers, name):
    got = forms(headers[name])
    assert got == mec.FORMS[name], {k: (got.get(k), mec.FORMS[name].get(k)) for k in set(got) | set(mec.FORMS[name]) if got.get(k) != mec.FORMS[name].get(k)}
    assert (mec.FORMS[name]["dual"] is True) == (name not in mec.DUAL_DECLINES)
    assert isinstance(mec.FORMS[name]["team"], int) == (name not in mec.TEAM_DECLINES)


def test_every_selector_is_covered_from_both_sides():
    """The selectors of the issue's table, each as a predicate over a chain's parameters and recorded forms: some chain on
    either side.  The LDS residency of a light unit's table inside the persistent launch (CM and MIX2 of 4 .. 512 words;
    device kPipeLightLdsMaxWords, codegen.cpp plan_persistent) is not named in the generated source: those selectors are
    held by the chains' PARAMETERS only, and a limit that moves there does not fail this test."""
    P, F = {n: mec.CHAINS[n][1] for n in mec.NAMES}, mec.FORMS

    def sides(what, pred, names=mec.NAMES):
        vals = {bool(pred(n)) for n in names}
        assert vals == {True, False}, (what, vals)

    with_cm = [n for n in mec.NAMES if "cm" in P[n]]
    sides("CM of one word (resident)", lambda n: 0 in P[n]["cm"], with_cm)
    sides("CM below 4 words (never in LDS)", lambda n: min(P[n]["cm"]) <= 1, with_cm)
    sides("CM of 4 .. 512 words (LDS inside the persistent launch)", lambda n: any(2 <= s <= 9 for s in P[n]["cm"]), with_cm)
    sides("CM from 512 words on: a lane per bit position", lambda n: 9 in F[n]["bits1"], with_cm)
    sides("every CM from 512 words on", lambda n: min(P[n]["cm"]) >= 9, with_cm)
    sides("CM above 512 words (not in LDS)", lambda n: max(P[n]["cm"]) >= 10, with_cm)
    with_m2 = [n for n in mec.NAMES if "mix2" in P[n]]
    sides("MIX2 with one weight", lambda n: P[n]["mix2"][0] == 0, with_m2)
    sides("MIX2 of 2 words (no LDS)", lambda n: P[n]["mix2"][0] == 1, with_m2)
    sides("MIX2 of 4 .. 512 words (LDS)", lambda n: 2 <= P[n]["mix2"][0] <= 9, with_m2)
    sides("MIX2 above 512 words", lambda n: P[n]["mix2"][0] >= 10, with_m2)
    sides("MIX2 with a lane per bit position", lambda n: 10 in F[n]["bits1"], with_m2)
    sides("masked MIX2 on a table of 256 words or more", lambda n: P[n]["mix2"][0] >= 8 and P[n]["mix2"][1] != 255, with_m2)
    with_sse = [n for n in mec.NAMES if "sse" in P[n]]
    sides("SSE from 8 bits on: a lane per bit position", lambda n: P[n]["sse"] >= 8, with_sse)
    for n in with_sse:
        assert (11 in F[n]["bits0"]) == (11 in F[n]["bits1"]) == (P[n]["sse"] >= 8), n
    with_mix = [n for n in mec.NAMES if "mix" in P[n]]
    sides("MIX with a lane per bit position (latency shape)", lambda n: F[n]["mix_bits1"] == 1, with_mix)
    sides("MIX in halves (throughput shape)", lambda n: F[n]["nh0"] == 2, with_mix)
    sides("masked MIX on a table of 256 rows or more", lambda n: P[n]["mix"][0] >= 8 and P[n]["mix"][1] != 255, with_mix)
    sides("MIX below 256 rows", lambda n: P[n]["mix"][0] < 8, with_mix)
    widths = {q for n in with_mix for q in F[n]["ql"]}
    assert widths >= {1, 2, 16}, widths                      # arities 1 and 4, 5 and 6, 40
    assert F["wide_mix"]["ql"] == (16,) and F["wide_mix"]["mix_bits1"] == 0      # width 16 rules out bit lanes on a big unmasked table
    assert {F[n]["lanes"] for n in mec.NAMES if F[n]["h_lds"]} >= {64, 32, 16, 8}
    sides("H in LDS in the encoder (hh <= 11)", lambda n: F[n]["h_lds"])
    sides("H in LDS in the wavefront decoders (hh <= 10)", lambda n: F[n]["dec_h_lds"])
    sides("encoder keeps H in LDS where the decoders do not (hh = 11)", lambda n: F[n]["h_lds"] and not F[n]["dec_h_lds"])
    sides("M in LDS (hm <= 8)", lambda n: F[n]["m_lds"])
    assert {P[n]["hm"] for n in mec.NAMES if "hm" in P[n]} >= {8, 9}
    sides("small chain in the latency shape", lambda n: F[n]["small1"])
    assert {F[n]["team"] for n in mec.NAMES if isinstance(F[n]["team"], int)} == {384, 512}
    sides("more than 32 components", lambda n: F[n]["dual"] is not True)
    assert {F[n]["team"] for n in mec.TEAM_DECLINES} == {"H does not fit the LDS", "more than 32 components"}
    assert F["wide_mix"]["dual"] == "more than 32 components"


def _check_encoder(header, pairs, **kw):
    res = emu.pipe_run(header, [d for d, _ in pairs], chunk=64, **kw)
    for i, ((d, want), (got, status, consumed)) in enumerate(zip(pairs, res)):
        assert status == 0 and consumed == len(d), (kw, i, status)
        assert got == want, (kw, i)


@pytest.mark.parametrize("persist", [False, True], ids=["steps", "persistent"])
@pytest.mark.parametrize("mode", [0, 1], ids=["throughput", "latency"])
@pytest.mark.parametrize("name", mec.NAMES)
def test_emulated_encoder(headers, coded, name, mode, persist):
    _check_encoder(headers[name], coded[name], mode=mode, persist=persist)


# (the declined pairs are left out: test_forms_and_verdicts holds the generator to the declines)
DECODER_PAIRS = [(name, d) for name in mec.NAMES for d in ("wavefront", "dual", "lockstep")
                 if not (d == "dual" and name in mec.DUAL_DECLINES) and not (d == "lockstep" and name in mec.TEAM_DECLINES)]


@pytest.mark.parametrize("name,decoder", DECODER_PAIRS)
def test_emulated_decoders(headers, coded, name, decoder):
    pairs = coded[name]
    kw = {"wavefront": dict(waves=8), "dual": dict(dual=True), "lockstep": dict(team=True)}[decoder]
    res = emu.run(headers[name], [c + b"\0\0\0\0" for _, c in pairs], decode=True, out_cap=max(len(d) for d, _ in pairs) + 8, **kw)
    for i, ((d, c), (plain, status, used)) in enumerate(zip(pairs, res)):
        assert status == 0 and plain == d and used == len(c) + 4, (decoder, i, status, len(plain), len(d))
