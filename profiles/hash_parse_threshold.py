#!/usr/bin/env python3
"""Where the hash-table LZ77 parse (method 1, ...) should run: end-to-end zpq_compress_blocks time with the parse on the device
(ZPAQ_AMD_DEVICE_PARSE=1) and on the host (=0), by a host clock around the call, after one warm-up call per setting, the two
settings alternating `--reps` times in one process.  DESIGN 4.5 has the table this prints and the routing rule drawn from it.

    python profiles/hash_parse_threshold.py [--lib PATH] [--cases CASE ...] [--reps 3] [--knobs 1,0] [--out FILE]

--lib: another build of the library (e.g. the parent commit's, to show that the knob-off path costs what the parent costs; such a
build has no knob for these methods: give --knobs 0).  Cases: <method>:<kind>:<block bytes>:<blocks>; the default list is
the one DESIGN reports.  Inputs: 64 distinct blocks of zpaq_amd.corpus, repeated to the count asked for.  Archives of the two
settings are compared with each other, every call."""
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
DEFAULT_CASES = (
    [f"{m}:text:{MIB}:{nb}" for m in ("1", "x0,1,4,0,3,20") for nb in (4, 16, 64, 256, 1024)]
    + [f"1:zeros:{MIB}:256", f"1:records:{MIB}:256", f"14:text:{16 * MIB - 4096}:64"]
)
u8p = C.POINTER(C.c_ubyte)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--cases", nargs="*", default=DEFAULT_CASES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--knobs", default="1,0")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from zpaq_amd import corpus
    if a.lib is None:
        import zpaq_amd
        a.lib = zpaq_amd.library_path()
    L = C.CDLL(a.lib)
    L.zpq_last_error.restype = C.c_char_p
    assert L.zpq_init(0) == 0, L.zpq_last_error()
    counter = getattr(L, "zpq_last_hash_parse_blocks", None)
    if counter is not None:
        counter.restype = C.c_uint32
    knobs = a.knobs.split(",")
    rows = []
    for case in a.cases:
        method, kind, nbytes, nb = case.split(":")
        nbytes, nb = int(nbytes), int(nb)
        distinct = [corpus.block(kind, nbytes, 7000 + i) for i in range(min(nb, 64 if nbytes <= MIB else 8))]
        ins = [distinct[i % len(distinct)].copy() for i in range(nb)]
        caps = [nbytes + nbytes // 4 + 8192] * nb
        outs = [np.empty(c, np.uint8) for c in caps]
        IA = (u8p * nb)(*[x.ctypes.data_as(u8p) for x in ins])
        IL = (C.c_uint32 * nb)(*[nbytes] * nb)
        OA = (u8p * nb)(*[x.ctypes.data_as(u8p) for x in outs])
        OC = (C.c_uint64 * nb)(*caps)
        OL = (C.c_uint64 * nb)()

        def call(knob):
            os.environ["ZPAQ_AMD_DEVICE_PARSE"] = knob
            t0 = time.perf_counter()
            rc = L.zpq_compress_blocks(method.encode(), IA, IL, nb, None, None, 1, OA, OC, OL)
            dt = time.perf_counter() - t0
            assert rc == 0, (case, knob, L.zpq_last_error())
            h = hashlib.sha1()
            for k in range(nb):
                h.update(outs[k][:OL[k]].tobytes())
            return dt, h.hexdigest(), int(counter()) if counter is not None else -1, sum(int(x) for x in OL)

        digests = set()
        for k in knobs:                                    # warm-up: buffers, pinned staging, code objects
            digests.add(call(k)[1])
        times = {k: [] for k in knobs}
        parsed = {}
        size = 0
        for _ in range(a.reps):
            for k in knobs:
                dt, dg, cnt, size = call(k)
                times[k].append(round(dt * 1e3, 2))
                parsed[k] = cnt
                digests.add(dg)
        assert len(digests) == 1, (case, "the settings made different archives")
        row = {"lib": os.path.relpath(a.lib, ROOT), "method": method, "kind": kind, "block_bytes": nbytes, "blocks": nb, "archive_bytes": size,
               "archives_sha1": digests.pop()[:12], "ms": times, "device_parsed_blocks": parsed}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
    L.zpq_shutdown()


if __name__ == "__main__":
    main()
