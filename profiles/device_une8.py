#!/usr/bin/env python3
"""Where the segments of the E8E9 methods should be decoded: end-to-end zpq_decompress time with the stage's decoder and the
inverse filter on the device (ZPAQ_AMD_DEVICE_UNE8=1: device/e8e9_kernel.h behind device/lz77_decode_kernel.h or
device/bwt_decode_kernel.h), with the route decompression had before it (ZPAQ_AMD_DEVICE_UNE8=0: the translated PCOMP program
on the device, a lane per segment, from 4 segments or 256 KiB on -- the yardstick) and with the host's translated programs
(ZPAQ_AMD_PCOMP=host), by a host clock around the call, after one warm-up call per setting, the settings alternating `--reps`
times in one process.  DESIGN 4.5.5 takes the table this prints.

    python profiles/device_une8.py [--cases CASE ...] [--reps 3] [--settings une81,une80,host] [--out FILE]

Cases: <method>:<kind>:<block bytes>:<blocks>; kind x86 is the seeded generator of tests/e8e9_cases.py (about 2 % e8 / e9 opcodes
with displacements whose top byte is 00 or ff, padding runs), any other one of zpaq_amd.corpus.  Inputs: up to 64 distinct blocks,
repeated to the count asked for, compressed once with zpq_compress_blocks.  The output of every call is compared with the input.
Per case: the calls' milliseconds, MB/s of the best call, the segments the new route decoded, and whether it was faster than both
others in every alternation -- the rule behind e8_une8_pays (device/engine.hpp).

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

BLOCK = (1 << 20) - 4096                                     # the largest block an x0 method compresses
# E8E9 in front of LZ77 level 1, level 2, the BWT, and alone
DEFAULT_CASES = [f"{m}:x86:{BLOCK}:{nb}" for m in ("x0,5,6,0,3,20", "x0,6,4,0,3,20", "x0,7", "x0,4") for nb in (64, 256, 1024)]
SETTINGS = {
    "une81": {"ZPAQ_AMD_DEVICE_UNE8": "1"},
    "une80": {"ZPAQ_AMD_DEVICE_UNE8": "0"},
    "host": {"ZPAQ_AMD_PCOMP": "host"},
}
u8p = C.POINTER(C.c_ubyte)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=DEFAULT_CASES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--settings", default="une81,une80,host")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import zpaq_amd as z
    from zpaq_amd import corpus
    L = z.lib()
    z.init(0)
    settings = tuple(a.settings.split(","))
    rows = []
    for case in a.cases:
        method, kind, nbytes, nb = case.split(":")
        nbytes, nb = int(nbytes), int(nb)
        if kind == "x86":
            import e8e9_cases
            distinct = [np.frombuffer(e8e9_cases.x86_like(nbytes, 7000 + i), np.uint8) for i in range(min(nb, 64))]
        else:
            distinct = [corpus.block(kind, nbytes, 7000 + i) for i in range(min(nb, 64))]
        arch = z.compress_blocks([d.copy() for d in distinct], method)
        archive = np.frombuffer(b"".join(arch[i % len(arch)] for i in range(nb)), np.uint8)
        want = np.concatenate([distinct[i % len(distinct)] for i in range(nb)])
        out = np.empty(want.size + 64, np.uint8)
        ol = C.c_uint64(0)

        def call(name):
            for k in ("ZPAQ_AMD_DEVICE_UNE8", "ZPAQ_AMD_PCOMP"):
                os.environ.pop(k, None)
            os.environ.update(SETTINGS[name])
            t0 = time.perf_counter()
            rc = L.zpq_decompress(archive.ctypes.data_as(u8p), archive.size, out.ctypes.data_as(u8p), out.size, C.byref(ol))
            dt = time.perf_counter() - t0
            assert rc == 0, (case, name, L.zpq_last_error())
            assert ol.value == want.size and np.array_equal(out[:want.size], want), (case, name, "the output is not the input")
            return dt, int(L.zpq_last_device_une8_segments())

        for s in settings:                                     # warm-up: buffers, pinned staging, code objects
            call(s)
        times = {s: [] for s in settings}
        segs = {}
        for _ in range(a.reps):
            for s in settings:
                dt, n = call(s)
                times[s].append(round(dt * 1e3, 2))
                segs[s] = n
        new, others = settings[0], settings[1:]
        row = {"method": method, "kind": kind, "block_bytes": nbytes, "blocks": nb, "archive_bytes": int(archive.size), "ms": times,
               "mb_per_s": {s: round(nbytes * nb / 1e6 / (min(times[s]) / 1e3), 1) for s in settings}, "device_une8_segments": segs,
               "faster_than_both_in_every_alternation": all(all(x < y for x, y in zip(times[new], times[o])) for o in others)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(rows, fh, indent=1)
    L.zpq_shutdown()


if __name__ == "__main__":
    main()
