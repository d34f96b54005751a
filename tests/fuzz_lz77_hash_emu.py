#!/usr/bin/env python3
"""Random hash-table LZ77 parameters and inputs through the device's parser on the host (tests/emu/lz77_hash_emu_main.cpp runs
zpaq_amd/csrc/device/lz77_hash_kernel.h lane by lane) against the host's parse of the same blocks: levels 1 / 2, a longer context
with look-ahead 0..7, buckets of 1..16 slots, tables of 2^1..2^24 slots, E8E9 in front, ragged batches.  The long-running form
of the seeded round in tests/test_emu_lz77_hash.py.  No GPU.

    python tests/fuzz_lz77_hash_emu.py [rounds] [seed]"""
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import zpaq_amd as z
    from test_emu_lz77_hash import fuzz_round
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    z.lib()
    for r in range(rounds):
        xm, ns = fuzz_round(z, rng)
        print("round %d ok: %s, lengths %s" % (r + 1, xm, ns), flush=True)
    print("rounds", rounds, "no mismatch")


if __name__ == "__main__":
    main()
