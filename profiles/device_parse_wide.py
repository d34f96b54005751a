#!/usr/bin/env python3
"""Where the LZ77 parse of a block of 16 MiB and more should run: end-to-end zpq_compress_blocks time with the parse in pieces
on the device behind the wide sorter (ZPAQ_AMD_DEVICE_PARSE_WIDE=1, device/lz77_wide_kernel.h) and with the host's parse over the
device's array (=0, the path before the device parse existed: the yardstick), by a host clock around the call, after one warm-up
call per setting, the two settings alternating `--reps` times in one process.  DESIGN 4.5.9 has the table this prints and the
rule engine.hpp lz_wide_parse_pays follows.

    python profiles/device_parse_wide.py [--cases CASE ...] [--levels 1,2] [--reps 3] [--knobs 1,0] [--out FILE]

Cases: <kind>:<block bytes>, kinds of zpaq_amd.corpus (text, records, lcg, zeros) and `serial`: LCG bytes with one match of 64
bytes near the start (reported, not part of the rule).  It was meant as the walk's bad case -- literals pending at every piece's
start, no re-join, the stitch's one wavefront walks the block -- but 16 MiB of random bytes hold about a hundred chance repeats
of 5 bytes and more, which the parse takes at min_match 4 and at which the walk re-joins: the `pieces` column says how serial a
run was (all / adopted whole / re-joined / own tokens only).  One block per case.  Levels: 1 = x<N>,1,4,0,7,<21+N>,1 (no model: the LZ77 stream is stored, the parse is
the call), 2 = x<N>,2,12,0,7,<21+N>,1c0,0,511i2; N from the block size as the archiver chooses it.  One block of the largest size
is generated per kind; smaller blocks are its prefixes.  Archives of the two settings are compared with each other, every call.
Per case: the calls' milliseconds, front_ms of zpq_last_api_timing (everything in front of the coder: sort and parse are in it),
MB/s of the best call, the blocks parsed and coded on the device and the pieces of the last parse (all, adopted whole, re-joined, own).

For the kernels: rocprofv3 --kernel-trace --stats -- python profiles/device_parse_wide.py --knobs 1 --reps 1 --levels 1 --cases text:67104768"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIB = 1 << 20
SIZES = (16 * MIB + 4096, 32 * MIB, 64 * MIB - 4096)
KINDS = ("text", "records", "lcg", "zeros")
DEFAULT_CASES = [f"{kind}:{n}" for kind in KINDS for n in SIZES] + [f"serial:{SIZES[0]}"]
u8p = C.POINTER(C.c_ubyte)


def method(level: int, nbytes: int) -> str:
    n = 0
    while nbytes + 4096 > (MIB << n):
        n += 1
    return f"x{n},1,4,0,7,{21 + n},1" if level == 1 else f"x{n},2,12,0,7,{21 + n},1c0,0,511i2"


def block(corpus, kind: str, nbytes: int) -> np.ndarray:
    if kind != "serial":
        return corpus.block(kind, nbytes, 7000)
    d = corpus.block("lcg", nbytes, 7001)
    d[100:164] = d[0:64]
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=DEFAULT_CASES)
    ap.add_argument("--levels", default="1,2")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--knobs", default="1,0", help="settings to alternate: 1, 0, auto (the variable unset: lz_wide_parse_pays decides)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import zpaq_amd as z
    from zpaq_amd import corpus
    L = z.lib()
    z.init(0)
    knobs = tuple(a.knobs.split(","))
    levels = tuple(int(x) for x in a.levels.split(","))
    cases = [(c.split(":")[0], int(c.split(":")[1])) for c in a.cases]
    largest = {}
    for kind, nbytes in cases:
        largest[kind] = max(largest.get(kind, 0), nbytes)
    data = {}
    rows = []
    ph = (C.c_double * 8)()
    for level in levels:
        for kind, nbytes in cases:
            if kind not in data:
                data[kind] = block(corpus, kind, largest[kind])
            src = data[kind][:nbytes]
            xm = method(level, nbytes)
            ins = src.copy()
            cap = nbytes + nbytes // 32 + 8192
            out = np.empty(cap, np.uint8)
            IA = (u8p * 1)(ins.ctypes.data_as(u8p))
            IL = (C.c_uint32 * 1)(nbytes)
            OA = (u8p * 1)(out.ctypes.data_as(u8p))
            OC = (C.c_uint64 * 1)(cap)
            OL = (C.c_uint64 * 1)()

            def call(knob):
                if knob == "auto":
                    os.environ.pop("ZPAQ_AMD_DEVICE_PARSE_WIDE", None)
                else:
                    os.environ["ZPAQ_AMD_DEVICE_PARSE_WIDE"] = knob
                np.copyto(ins, src)
                t0 = time.perf_counter()
                rc = L.zpq_compress_blocks(xm.encode(), IA, IL, 1, None, None, 1, OA, OC, OL)
                dt = time.perf_counter() - t0
                assert rc == 0, (kind, nbytes, knob, L.zpq_last_error())
                L.zpq_last_api_timing(ph)
                return dt, hashlib.sha1(out[:OL[0]].tobytes()).hexdigest(), (z.last_wide_parse_blocks(), z.last_device_coded_blocks()), float(ph[1]), int(OL[0])

            digests = set()
            for k in knobs:                                        # warm-up: buffers, code objects
                digests.add(call(k)[1])
            times = {k: [] for k in knobs}
            fronts = {k: [] for k in knobs}
            parsed, coded, pieces = {}, {}, None
            size = 0
            for _ in range(a.reps):
                for k in knobs:
                    dt, dg, cnt, front, size = call(k)
                    times[k].append(round(dt * 1e3, 2))
                    fronts[k].append(round(front, 2))
                    parsed[k], coded[k] = cnt
                    digests.add(dg)
                    if cnt[0]:
                        pieces = list(z.last_wide_parse_pieces())
            assert len(digests) == 1, (kind, nbytes, xm, "the settings made different archives")
            row = {"method": xm, "kind": kind, "block_bytes": nbytes, "archive_bytes": size, "archives_sha1": digests.pop()[:12], "ms": times,
                   "front_ms": fronts, "mb_per_s": {k: round(nbytes / 1e6 / (min(times[k]) / 1e3), 1) for k in knobs}, "wide_parse_blocks": parsed,
                   "device_coded_blocks": coded, "pieces": pieces}
            if len(knobs) > 1:
                row["faster_in_every_alternation"] = all(x < y for x, y in zip(times[knobs[0]], times[knobs[-1]]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
    L.zpq_shutdown()


if __name__ == "__main__":
    main()
