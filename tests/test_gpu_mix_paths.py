"""GPU: the throughput shape of the pipelined encoder, forced on a batch small enough to be quick, on the block lengths where
the MIX unit's per-byte loop changes path (tests/mix_paths_cases.py: chunk edges, a ragged group, a row forwarded from byte to
byte).  Through the persistent launch and through the step kernels: coded payloads identical to the oracle's, every block
decoded back."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_paths_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want(zlib_, oracle):
    header = cases.header(zlib_)
    return header, [oracle.encode(header, d) for d in cases.inputs()]


@pytest.mark.parametrize("persist", [True, False])
def test_mix_paths_of_the_throughput_shape(gpu, want, monkeypatch, persist):
    header, coded = want
    inputs = cases.inputs()
    monkeypatch.setenv("ZPAQ_AMD_PIPE_MODE", "throughput")       # (33 blocks alone would take the latency shape)
    if not persist:
        monkeypatch.setenv("ZPAQ_AMD_PIPE_PERSIST", "0")
    plan = gpu.Plan(header)
    got = gpu.encode_batch([plan] * len(inputs), inputs)
    assert gpu.lib().zpq_last_persistent() == (1 if persist else 0)
    for i, (g, w) in enumerate(zip(got, coded)):
        assert g == w, i
    back = gpu.decode_batch([plan] * len(inputs), [g + b"\0\0\0\0" for g in got], [len(d) + 8 for d in inputs])
    for i, ((plain, used), d, g) in enumerate(zip(back, inputs, got)):
        assert plain == d and used == len(g) + 4, i
