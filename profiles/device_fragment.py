#!/usr/bin/env python3
"""Where files should be cut into fragments: zpq_fragment_device (device/fragment_kernel.h: a wavefront per piece, the host's
stitch, one SHA-1 job per fragment on the device; the upload is part of the call) against zpq_fragment_host on one thread, both
including the SHA-1s, by a host clock around the call, after one warm-up call each, alternating `--reps` times in one process.
DESIGN 4.5.6 takes the table this prints.

    python profiles/device_fragment.py [--shapes SHAPE ...] [--reps 3] [--fragment 6] [--out profiles/device_fragment.json]

Shapes: <kind>:<file bytes>:<files>; kind one of zpaq_amd.corpus.  A large file is made of seeded blocks of 1 MiB.  The results of
the two entries are compared field by field in every repetition.  No figure is promised: the script measures."""
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

MIB = 1 << 20
DEFAULT_SHAPES = [f"text:{MIB}:256", f"text:{256 * MIB}:1", f"zeros:{256 * MIB}:1"]
BLOCKSIZE = (1 << 24) - 4096                                 # the block of the archiver's default method
u8p = C.POINTER(C.c_ubyte)
u32p = C.POINTER(C.c_uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=DEFAULT_SHAPES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fragment", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_fragment.json"))
    a = ap.parse_args()
    import zpaq_amd as z
    from zpaq_amd import corpus
    L = z.lib()
    z.init(0)
    rows = []
    for shape in a.shapes:
        kind, nbytes, nfiles = shape.split(":")
        nbytes, nfiles = int(nbytes), int(nfiles)
        files = []
        for f in range(nfiles):
            parts = [corpus.block(kind, min(MIB, nbytes - at), 9000 + 1000 * f + at // MIB) for at in range(0, nbytes, MIB)]
            files.append(np.concatenate(parts) if len(parts) > 1 else parts[0])
        IA = (u8p * nfiles)(*[x.ctypes.data_as(u8p) for x in files])
        IL = (C.c_uint64 * nfiles)(*[x.size for x in files])
        total = C.c_size_t(0)
        nf = (C.c_uint32 * nfiles)()
        rc = L.zpq_fragment_host(IA, IL, nfiles, a.fragment, BLOCKSIZE, nf, None, None, None, None, 0, C.byref(total))
        assert rc in (0, 3), rc
        cap = int(total.value)

        def call(name):
            entry = L.zpq_fragment_device if name == "device" else L.zpq_fragment_host
            size, hits = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
            sha, o1 = np.zeros(20 * cap, np.uint8), np.zeros(256 * cap, np.uint8)
            t0 = time.perf_counter()
            rc = entry(IA, IL, nfiles, a.fragment, BLOCKSIZE, nf, size.ctypes.data_as(u32p), hits.ctypes.data_as(u32p), sha.ctypes.data_as(u8p),
                       o1.ctypes.data_as(u8p), cap, C.byref(total))
            dt = time.perf_counter() - t0
            assert rc == 0, (shape, name, rc, L.zpq_last_error())
            return dt, (list(nf), size, hits, sha, o1)

        for s in ("device", "host"):                           # warm-up: buffers, code objects
            call(s)
        times = {"device": [], "host": []}
        for _ in range(a.reps):
            got = {}
            for s in ("device", "host"):
                dt, got[s] = call(s)
                times[s].append(round(dt * 1e3, 2))
            assert got["device"][0] == got["host"][0] and all(np.array_equal(x, y) for x, y in zip(got["device"][1:], got["host"][1:])), \
                (shape, "the device's fragments are not the host's")
        row = {"kind": kind, "file_bytes": nbytes, "files": nfiles, "fragment": a.fragment, "fragments": cap, "ms": times,
               "fix_up_rounds": int(L.zpq_last_fragment_rounds()),
               "mb_per_s": {s: round(nbytes * nfiles / 1e6 / (min(times[s]) / 1e3), 1) for s in times},
               "device_faster_in_every_alternation": all(x < y for x, y in zip(times["device"], times["host"]))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")
    L.zpq_shutdown()


if __name__ == "__main__":
    main()
