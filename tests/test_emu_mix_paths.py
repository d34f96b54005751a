"""CPU (-m "not gpu"): the throughput shape's persistent launch on the wavefront emulator, on the block lengths where the MIX
unit's per-byte loop changes path (tests/mix_paths_cases.py): 33 blocks of -m5 -- a full group and a ragged one -- in chunks
of 512 bytes as on the device, every coded stream against the oracle."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

import mix_paths_cases as cases  # noqa: E402


def test_mix_paths_of_the_throughput_shape(zlib_, oracle):
    header = cases.header(zlib_)
    src = emu.pipe_source(header, 512, mode=0)
    assert "PIPE_MODE = 0, MIX_BITS = 0" in src and "PS_MIX_NH = 2" in src and "PIPE_C = 512" in src
    inputs = cases.inputs()
    assert len(inputs) == 33
    res = emu.pipe_run(header, inputs, chunk=512, mode=0, persist=True)
    for i, (inp, (coded, status, consumed)) in enumerate(zip(inputs, res)):
        assert status == 0 and consumed == len(inp), (i, status)
        assert coded == oracle.encode(header, inp), i
