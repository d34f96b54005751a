"""The 33-block -m5 case of tests/test_emu_mix_paths.py (emulator) and tests/test_gpu_mix_paths.py (MI355X): one full group of
32 blocks plus a ragged one, for the throughput shape of the pipelined encoder.  What can go wrong in the MIX unit's
per-byte loop lies at chunk edges (lengths around 512, the chunk, and 1024), in a group that is not full and where a row is
forwarded from one byte to the next (the same context and the same rows at every byte) -- all below 2 KiB per block."""
from zpaq_amd import corpus

LENGTHS = [0, 1, 511, 512, 513, 1025]
KINDS = ["text", "records", "lcg", "pattern", "zeros"]


def header(z):
    return z.method_to_header(z.expand_method("5", corpus.block("text", 1 << 20, corpus.BASE_SEED)))[0]


def inputs():
    """33 inputs as the encoder takes them (the post-processing byte 0 in front)."""
    blocks = [corpus.block(KINDS[i % 5], LENGTHS[i % 6], 900 + i).tobytes() for i in range(33)]
    blocks[7] = b"\x55" * 1025          # one byte repeated: the same context and the same rows at every byte
    blocks[20] = b"ab" * 600
    return [b"\0" + d for d in blocks]
