"""CPU (-m "not gpu"): where the packer of the persistent encoder launch (host/codegen.cpp plan_persistent) puts a workgroup's
wavefronts, read from the generated source.  In the throughput shape (mode 0) wavefront w of a workgroup of 8 runs on SIMD
w % 4: the MIX wavefronts, whose unit paces the launch, are spread over the SIMDs and sit at the lower wave index of theirs;
the latency shapes (modes 1 and 3) are generated as before.  (An issue priority per slot, PS_PRIO, was built and measured with
this placement and did not pay: no shape's source carries such a table.)"""
import os
import random
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)
import emu  # noqa: E402
import fuzz_emu  # noqa: E402

from zpaq_amd import corpus  # noqa: E402


def _table(src, name):
    m = re.search(r"static constexpr int %s\[\d+\] = \{([^}]*)\}" % name, src)
    return [int(x) for x in m.group(1).split(",")] if m else None


def _value(src, name):
    return int(re.search(r"\b%s = (\d+)" % name, src).group(1))


def _check_throughput_placement(src):
    """-> the number of MIX wavefronts of the chain's group."""
    kind = _table(src, "PS_KIND")
    waves, wpg = _value(src, "PS_WAVES"), _value(src, "PS_WPG")
    assert len(kind) == waves * wpg
    assert "PS_PRIO" not in src
    if waves != 8:
        return kind.count(5)
    for g in range(wpg):
        wk = kind[g * 8:(g + 1) * 8]
        mix_waves = [w for w in range(8) if wk[w] == 5]
        simds = {w % 4 for w in mix_waves}
        assert len(simds) == min(len(mix_waves), 4), (g, wk)
        for s in simds:
            assert wk[s] == 5, (g, wk)          # the SIMD's lower wave index (w < 4) is a MIX wavefront
    return kind.count(5)


def _h5(zlib_):
    return zlib_.method_to_header(zlib_.expand_method("5", corpus.block("text", 1 << 20, corpus.BASE_SEED)))[0]


def test_headline_chain_mixers_one_per_simd(zlib_):
    src = emu.pipe_source(_h5(zlib_), 64, mode=0)
    assert "PS_WAVES = 8, PS_WPG = 8" in src
    assert _check_throughput_placement(src) == 16       # two mixers in halves: 2 x 8 wavefronts per group of 32 blocks


@pytest.mark.parametrize("level", [2, 3])
def test_legacy_models(zlib_, level):
    src = emu.pipe_source(zlib_.builtin_model_header(level), 64, mode=0)
    assert "PS_WPG" in src
    assert _check_throughput_placement(src) >= 1


def test_random_models(zlib_):
    rng = random.Random(20)
    done = with_mix = 0
    while done < 20:
        cfg = fuzz_emu.random_model(rng, big=done % 2 == 1)
        try:
            header, _ = zlib_.assemble(cfg)
            zlib_.Plan(header)
        except zlib_.ZpaqError:
            continue
        src = emu.pipe_source(header, 64, mode=0)
        if "PS_WPG" not in src:
            continue
        with_mix += _check_throughput_placement(src) > 0
        done += 1
    assert with_mix >= 5


def test_latency_shapes_are_generated_as_before(zlib_):
    h5 = _h5(zlib_)
    src1, src3 = emu.pipe_source(h5, 64, mode=1), emu.pipe_source(h5, 64, mode=3)
    assert "PS_PRIO" not in src1 and "PS_PRIO" not in src3
    assert "PS_WAVES = 8, PS_WPG = 14" in src1 and "PS_WAVES = 4, PS_WPG = 28" in src3
    h3 = zlib_.method_to_header(zlib_.expand_method("3", corpus.block("lcg", 1 << 18, corpus.BASE_SEED)))[0]
    small = emu.pipe_source(h3, 64, mode=1)
    assert "PS_PRIO" not in small and "PS_CODER_FAST = true, PS_SMALL = true" in small and "PS_WAVES = 4" in small
    for level in (2, 3):
        assert "PS_PRIO" not in emu.pipe_source(zlib_.builtin_model_header(level), 64, mode=1)
