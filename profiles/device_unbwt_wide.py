#!/usr/bin/env python3
"""Where the BWT streams of blocks of 16 MiB and more should be decoded: end-to-end zpq_decompress time with the device's wide
BWT decoder (ZPAQ_AMD_DEVICE_UNBWT=1: device/bwt_decode_wide_kernel.h), with the route decompression had before it
(ZPAQ_AMD_DEVICE_UNBWT=0: the translated PCOMP program on the device, a lane per segment -- the yardstick) and with the host's
translated programs (ZPAQ_AMD_PCOMP=host), by a host clock around the call, after one warm-up call per setting, the settings
alternating `--reps` times in one process.  DESIGN 4.5.8 has the table this prints.

    python profiles/device_unbwt_wide.py [--cases CASE ...] [--reps 3] [--settings unbwt1,unbwt0,host] [--limit 120] [--out FILE]

Cases: <method>:<kind>:<block bytes>:<blocks>, in the order given -- the smaller sizes first.  The output of every call is compared
with the input.  The yardsticks walk a list of 4 bytes per position one dependent load after the other, so a setting other than
the first is run on a case only while the time its calls would take -- its best seconds per byte so far on the same kind of
data, times the case's bytes, times 1 + reps calls -- stays within `--limit` seconds; otherwise "limit" is recorded in place of
its times, and the new route counts as beaten only by the settings that ran.  A setting whose warm-up call alone shows that its
`reps` calls would pass the limit keeps that one time ("single_call_ms_beyond_limit") and is not run again on the case.  Per
case: the calls' milliseconds, MB/s of the best call, the segments the new kernels decoded, and whether the new route was faster
than every other setting that ran in every alternation -- the rule behind bwt_unbwt_wide_pays (device/engine.hpp).

x.,7 methods are not among the cases and ZPAQ_AMD_DEVICE_UNE8 is not among the settings: bwt_une8_wide_pays stays false until they are.

For kernel times run this under rocprofv3 --kernel-trace --stats in a run of its own (--settings unbwt1)."""
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

SMALL = (1 << 24) + 4097                                     # the smallest block beyond the small decoder, and a tile more
DEFAULT_BLOCK = (64 << 20) - 4096                            # what the reference archiver cuts for -m2 .. -m5
DEFAULT_CASES = (
    [f"x6,3:{kind}:{SMALL}:1" for kind in ("text", "zeros", "records", "lcg")]
    + ["x6,3:text:4194304:16"]                               # small blocks under the large program
    + [f"x6,3:{kind}:{DEFAULT_BLOCK}:1" for kind in ("text", "zeros", "records")]
)
SETTINGS = {
    "unbwt1": {"ZPAQ_AMD_DEVICE_UNBWT": "1"},
    "unbwt0": {"ZPAQ_AMD_DEVICE_UNBWT": "0"},
    "host": {"ZPAQ_AMD_PCOMP": "host"},
}
u8p = C.POINTER(C.c_ubyte)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=DEFAULT_CASES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--settings", default="unbwt1,unbwt0,host")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds a yardstick setting may take on one case, predicted from smaller ones")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import zpaq_amd as z
    from zpaq_amd import corpus
    L = z.lib()
    z.init(0)
    settings = tuple(a.settings.split(","))
    os.environ["ZPAQ_AMD_DEVICE_SORT_WIDE"] = "1"            # (the archives are made once; how does not matter here)
    rows = []
    per_byte = {}                                            # (setting, kind) -> best seconds per byte seen
    for case in a.cases:
        method, kind, nbytes, nb = case.split(":")
        nbytes, nb = int(nbytes), int(nb)
        distinct = [corpus.block(kind, nbytes, 7000 + i) for i in range(min(nb, 16))]
        arch = z.compress_blocks([d.copy() for d in distinct], method)
        archive = np.frombuffer(b"".join(arch[i % len(arch)] for i in range(nb)), np.uint8)
        want = np.concatenate([distinct[i % len(distinct)] for i in range(nb)])
        out = np.empty(want.size + 64, np.uint8)
        ol = C.c_uint64(0)

        def call(name):
            for k in ("ZPAQ_AMD_DEVICE_UNBWT", "ZPAQ_AMD_PCOMP"):
                os.environ.pop(k, None)
            os.environ.update(SETTINGS[name])
            t0 = time.perf_counter()
            rc = L.zpq_decompress(archive.ctypes.data_as(u8p), archive.size, out.ctypes.data_as(u8p), out.size, C.byref(ol))
            dt = time.perf_counter() - t0
            assert rc == 0, (case, name, L.zpq_last_error())
            assert ol.value == want.size and np.array_equal(out[:want.size], want), (case, name, "the output is not the input")
            return dt, int(L.zpq_last_device_unbwt_segments())

        ran, limited = [], {}
        for s in settings:
            known = per_byte.get((s, kind))
            predicted = None if known is None else known * want.size * (1 + a.reps)
            if s != settings[0] and predicted is not None and predicted > a.limit:
                limited[s] = round(predicted, 1)
                print(f"# {case}: {s} not run, its {1 + a.reps} calls are predicted at {predicted:.0f} s (limit {a.limit:.0f} s)", flush=True)
                continue
            ran.append(s)
        once = {}
        for s in list(ran):                                    # warm-up: buffers, pinned staging, code objects
            dt, _ = call(s)
            per_byte[(s, kind)] = min(per_byte.get((s, kind), 1e9), dt / want.size)
            if s != settings[0] and dt * a.reps > a.limit:     # one call is all this setting gets here
                once[s] = round(dt * 1e3, 2)
                ran.remove(s)
                print(f"# {case}: {s} took {dt:.1f} s once, {a.reps} more calls would pass the limit of {a.limit:.0f} s", flush=True)
        times = {s: [] for s in ran}
        segs = {}
        for _ in range(a.reps):
            for s in ran:
                dt, n = call(s)
                times[s].append(round(dt * 1e3, 2))
                segs[s] = n
                per_byte[(s, kind)] = min(per_byte.get((s, kind), 1e9), dt / want.size)
        new, others = settings[0], [s for s in ran[1:]]
        row = {"method": method, "kind": kind, "block_bytes": nbytes, "blocks": nb, "archive_bytes": int(archive.size),
               "ms": {s: (times[s] if s in times else "limit") for s in settings}, "predicted_s_beyond_limit": limited, "single_call_ms_beyond_limit": once,
               "mb_per_s": {s: round(nbytes * nb / 1e6 / (min(times[s]) / 1e3), 1) for s in ran}, "device_unbwt_segments": segs,
               "faster_than_every_setting_that_ran_in_every_alternation":
                   bool(others) and all(all(x < y for x, y in zip(times[new], times[o])) for o in others)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(rows, fh, indent=1)
    L.zpq_shutdown()


if __name__ == "__main__":
    main()
