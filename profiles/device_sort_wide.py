#!/usr/bin/env python3
"""Where the suffix sort of a block of 16 MiB and more should run: end-to-end zpq_compress_blocks time with the device's wide
sorter (ZPAQ_AMD_DEVICE_SORT_WIDE=1, device/sa_wide_kernel.h) and with the host's SA-IS (=0, the path before the wide sorter
existed: the yardstick), by a host clock around the call, after one warm-up call per setting, the two settings alternating
`--reps` times in one process.  DESIGN 4.5.7 has the table this prints and the rule engine.hpp sa_wide_pays follows.

    python profiles/device_sort_wide.py [--cases CASE ...] [--reps 3] [--knobs 1,0] [--method x6,3] [--out FILE]

Cases: <kind>:<block bytes>:<blocks>, kinds of zpaq_amd.corpus (text, records, lcg, zeros).  The default method x6,3 has no
model: the BWT stream is stored, so the sort (and, with the knob at 1, the last column made on the device) is the call.  One
block of the largest size is generated per kind; smaller blocks are its prefixes, and a case of several blocks sorts the same
block several times -- the device takes them one after another, the host one per core.  Archives of the two settings are
compared with each other, every call.  Per case: the calls' milliseconds, front_ms of zpq_last_api_timing (everything in front
of the coder: the sort is in it), MB/s of the best call, the blocks the wide sorter sorted and the rounds of the last one.

For the kernels: rocprofv3 --kernel-trace --stats -- python profiles/device_sort_wide.py --knobs 1 --reps 1 --cases text:67104768:1"""
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
DEFAULT_CASES = [f"{kind}:{n}:{nb}" for kind in KINDS for n in SIZES for nb in (1, 4)]
u8p = C.POINTER(C.c_ubyte)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=DEFAULT_CASES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--knobs", default="1,0", help="settings to alternate: 1, 0, auto (the variable unset: sa_wide_pays decides)")
    ap.add_argument("--method", default="x6,3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import zpaq_amd as z
    from zpaq_amd import corpus
    L = z.lib()
    z.init(0)
    knobs = tuple(a.knobs.split(","))
    cases = [(c.split(":")[0], int(c.split(":")[1]), int(c.split(":")[2])) for c in a.cases]
    largest = {}
    for kind, nbytes, _ in cases:
        largest[kind] = max(largest.get(kind, 0), nbytes)
    data = {}
    rows = []
    ph = (C.c_double * 8)()
    for kind, nbytes, nb in cases:
        if kind not in data:
            data[kind] = corpus.block(kind, largest[kind], 7000)
        src = data[kind][:nbytes]
        ins = [src.copy() for _ in range(nb)]
        caps = [nbytes + nbytes // 64 + 8192] * nb
        outs = [np.empty(c, np.uint8) for c in caps]
        IA = (u8p * nb)(*[x.ctypes.data_as(u8p) for x in ins])
        IL = (C.c_uint32 * nb)(*[nbytes] * nb)
        OA = (u8p * nb)(*[x.ctypes.data_as(u8p) for x in outs])
        OC = (C.c_uint64 * nb)(*caps)
        OL = (C.c_uint64 * nb)()

        def call(knob):
            if knob == "auto":
                os.environ.pop("ZPAQ_AMD_DEVICE_SORT_WIDE", None)
            else:
                os.environ["ZPAQ_AMD_DEVICE_SORT_WIDE"] = knob
            for k in range(nb):                                # (E8E9 methods rewrite the caller's buffers)
                np.copyto(ins[k], src)
            t0 = time.perf_counter()
            rc = L.zpq_compress_blocks(a.method.encode(), IA, IL, nb, None, None, 1, OA, OC, OL)
            dt = time.perf_counter() - t0
            assert rc == 0, (kind, nbytes, nb, knob, L.zpq_last_error())
            L.zpq_last_api_timing(ph)
            h = hashlib.sha1()
            for k in range(nb):
                h.update(outs[k][:OL[k]].tobytes())
            return dt, h.hexdigest(), z.last_wide_sort_blocks(), float(ph[1]), sum(int(x) for x in OL)

        digests = set()
        for k in knobs:                                        # warm-up: buffers, code objects
            digests.add(call(k)[1])
        times = {k: [] for k in knobs}
        fronts = {k: [] for k in knobs}
        wide = {}
        size = 0
        for _ in range(a.reps):
            for k in knobs:
                dt, dg, cnt, front, size = call(k)
                times[k].append(round(dt * 1e3, 2))
                fronts[k].append(round(front, 2))
                wide[k] = cnt
                digests.add(dg)
        assert len(digests) == 1, (kind, nbytes, nb, "the settings made different archives")
        row = {"method": a.method, "kind": kind, "block_bytes": nbytes, "blocks": nb, "archive_bytes": size, "archives_sha1": digests.pop()[:12],
               "ms": times, "front_ms": fronts, "mb_per_s": {k: round(nbytes * nb / 1e6 / (min(times[k]) / 1e3), 1) for k in knobs},
               "wide_sort_blocks": wide, "rounds": z.last_wide_sort_rounds()}
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
