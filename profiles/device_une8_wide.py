#!/usr/bin/env python3
"""Where the LZ77 streams of LARGE blocks of the E8E9 methods (x.,5 / x.,6) should be decoded: end-to-end zpq_decompress time with
the device's decoder for long streams and the inverse filter behind it (ZPAQ_AMD_DEVICE_UNE8=1 and ZPAQ_AMD_DEVICE_UNLZ_WIDE=1:
device/lz77_decode_wide_kernel.h, device/e8e9_kernel.h), with ZPAQ_AMD_DEVICE_UNE8=1 alone (the yardstick: the decoder of a
wavefront per stream in front of the filter) and with the host's translated programs (ZPAQ_AMD_PCOMP=host), by a host clock
around the call, after one warm-up call per setting, the settings alternating `--reps` times in one process.  DESIGN 4.5.10 has
the table this prints.

    python profiles/device_une8_wide.py [--cases CASE ...] [--reps 3] [--settings both1,une8,host] [--out FILE]

Cases: <method>:<kind>:<block bytes>:<blocks>; kind x86 is 1 MiB of the seeded generator of tests/e8e9_cases.py (about 2 % e8 / e9
opcodes with displacements whose top byte is 00 or ff) repeated to the block's length, the others are zpaq_amd.corpus's.  One
block is compressed once with zpq_compress_blocks and its archive repeated to the count asked for.  The output of every call is
compared with the input.  Per case: the calls' milliseconds, MB/s of the best call, the segments each route decoded, the pieces'
counts and the jump rounds, and whether the new route was faster than both others in every alternation -- the rule behind
e8_unlz_wide_pays (device/engine.hpp), which this measurement does not change: the route stays behind its two knobs.

For kernel times run this under rocprofv3 --kernel-trace --stats in a run of its own."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MIB = 1 << 20
BLOCK = (1 << 24) + 4097
KINDS = ("x86", "text", "lcg")
METHODS = ("x5,5,4,0,3,24", "x5,6,4,0,3,24")
DEFAULT_CASES = [f"{m}:{k}:{BLOCK}:{nb}" for m in METHODS for k in KINDS for nb in (1, 4)]
SETTINGS = {
    "both1": {"ZPAQ_AMD_DEVICE_UNE8": "1", "ZPAQ_AMD_DEVICE_UNLZ_WIDE": "1"},
    "une8": {"ZPAQ_AMD_DEVICE_UNE8": "1"},
    "host": {"ZPAQ_AMD_PCOMP": "host"},
}
KNOBS = ("ZPAQ_AMD_DEVICE_UNE8", "ZPAQ_AMD_DEVICE_UNLZ_WIDE", "ZPAQ_AMD_UNLZ_WIDE_FROM", "ZPAQ_AMD_UNLZ_WIDE_PIECE", "ZPAQ_AMD_DEVICE_UNLZ",
         "ZPAQ_AMD_DEVICE_UNBWT", "ZPAQ_AMD_PCOMP")
u8p = C.POINTER(C.c_ubyte)


def block_of(kind: str, nbytes: int) -> np.ndarray:
    if kind == "x86":
        import e8e9_cases
        unit = np.frombuffer(e8e9_cases.x86_like(min(nbytes, MIB), 7100), np.uint8)
        return np.tile(unit, (nbytes + unit.size - 1) // unit.size)[:nbytes].copy()
    from zpaq_amd import corpus
    return corpus.block(kind, nbytes, 7100)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=DEFAULT_CASES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--settings", default="both1,une8,host")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import zpaq_amd as z
    L = z.lib()
    z.init(0)
    settings = tuple(a.settings.split(","))
    rows = []
    for case in a.cases:
        method, kind, nbytes, nb = case.split(":")
        nbytes, nb = int(nbytes), int(nb)
        block = block_of(kind, nbytes)
        arch = z.compress_blocks([block.copy()], method)[0]
        archive = np.frombuffer(bytes(arch) * nb, np.uint8)
        want = np.concatenate([block] * nb)
        out = np.empty(want.size + 64, np.uint8)
        ol = C.c_uint64(0)

        def call(name):
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(SETTINGS[name])
            t0 = time.perf_counter()
            rc = L.zpq_decompress(archive.ctypes.data_as(u8p), archive.size, out.ctypes.data_as(u8p), out.size, C.byref(ol))
            dt = time.perf_counter() - t0
            assert rc == 0, (case, name, L.zpq_last_error())
            assert ol.value == want.size and np.array_equal(out[:want.size], want), (case, name, "the output is not the input")
            return dt, [int(L.zpq_last_device_une8_wide_segments()), int(L.zpq_last_device_une8_segments())]

        for s in settings:                                     # warm-up: buffers, pinned staging, code objects
            call(s)
        times = {s: [] for s in settings}
        segs = {}
        extra = {}
        for _ in range(a.reps):
            for s in settings:
                dt, n = call(s)
                times[s].append(round(dt * 1e3, 2))
                segs[s] = n
                if n[0]:
                    extra = {"pieces": list(z.last_unlz_wide_pieces()), "jump_rounds": z.last_unlz_wide_rounds()}
        new, others = settings[0], settings[1:]
        row = {"method": method, "kind": kind, "block_bytes": nbytes, "blocks": nb, "archive_bytes": int(archive.size), "ms": times,
               "mb_per_s": {s: round(nbytes * nb / 1e6 / (min(times[s]) / 1e3), 1) for s in settings},
               "device_une8_wide_and_une8_segments": segs, **extra,
               "faster_than_both_in_every_alternation": all(all(x < y for x, y in zip(times[new], times[o])) for o in others)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(rows, fh, indent=1)
    L.zpq_shutdown()


if __name__ == "__main__":
    main()
