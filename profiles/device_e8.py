#!/usr/bin/env python3
"""Where the forward E8E9 filter of a block that takes a device route should run: end-to-end zpq_compress_blocks time with the
filter on the device (ZPAQ_AMD_DEVICE_E8=1: device/e8e9_forward_kernel.h over the uploaded copy, the filtered bytes downloaded
into the caller's buffer) and on the host before the upload (ZPAQ_AMD_DEVICE_E8=0: the route compression had before -- the
yardstick), by a host clock around the call, after one warm-up call per setting, the two alternating `--reps` times in one
process per case.  DESIGN 4.5.11 takes the table this prints.

    python profiles/device_e8.py [--cases CASE ...] [--reps 3] [--out FILE] [--budget-s SECONDS]

Cases: <method>:<kind>:<block bytes>:<blocks>.  Kinds: x86 -- random bytes with an e8 / e9 opcode planted at about 2 % of the
positions and 00 / ff four bytes behind it (what tests/e8e9_cases.py x86_like makes, vectorised: 64 MiB of it are needed) --,
random (no structure: about 0.8 % of the positions are opcodes, one in 128 of them hits) and zeros (no candidate: the pure cost
of the extra download).  The methods have no model, so that the call is the pre-processing stage and little else.  Inputs: up
to 8 distinct blocks, repeated to the count asked for.  Every call's archives are compared with the first call's, and the
caller's buffers with the host filter's.  Per case: the calls' milliseconds, the blocks the device filtered, and whether =1
beat =0 in every alternation -- the rule behind e8_forward_pays and e8_forward_wide_pays (device/engine.hpp).  --budget-s: no new
case is started after that many seconds; what was not measured is listed as such, not guessed.

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

KINDS = ("x86", "random", "zeros")
BATCH_METHODS = ("x0,5,6,0,3,20", "x0,6,5,0,7,21,1", "x0,7")         # the hash parse; LZ77 through the suffix array; the BWT
WIDE_METHODS = ("x6,7", "x6,6,5,0,7,27,1")
WIDE_SIZES = ((16 << 20) + 4096, (64 << 20) - 4096)
DEFAULT_CASES = (
    [f"{m}:{k}:{n}:{nb}" for n in (256 << 10, (1 << 20) - 4096) for nb in (64, 256) for m in BATCH_METHODS for k in KINDS]
    + [f"{m}:{k}:{n}:1" for n in WIDE_SIZES for m in WIDE_METHODS for k in KINDS]
)
u8p = C.POINTER(C.c_ubyte)


def make(kind: str, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    b = rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "x86":
        at = np.flatnonzero(rng.random(n) < 0.02)
        at = at[at + 4 < n]
        b[at] = 0xe8 + (at & 1).astype(np.uint8)
        b[at + 4] = np.where(rng.random(at.size) < 0.5, 0x00, 0xff).astype(np.uint8)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=DEFAULT_CASES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--budget-s", type=float, default=0.0)
    a = ap.parse_args()
    import zpaq_amd as z
    L = z.lib()
    z.init(0)
    started = time.perf_counter()
    rows, skipped = [], []

    def dump():
        if a.out:
            with open(a.out, "w") as fh:
                json.dump({"measured": rows, "not_measured": skipped}, fh, indent=1)

    for case in a.cases:
        if a.budget_s and time.perf_counter() - started > a.budget_s:
            skipped.append(case)
            dump()
            continue
        method, kind, nbytes, nb = case.split(":")
        nbytes, nb = int(nbytes), int(nb)
        distinct = [make(kind, nbytes, 7000 + i) for i in range(min(nb, 8))]
        want = []
        for d in distinct:
            f = d.copy()
            L.zpq_e8e9(f.ctypes.data_as(u8p), f.size)
            want.append(f)
        ins = [None] * nb
        caps = [nbytes + nbytes // 4 + 8192] * nb
        outs = [np.empty(c, np.uint8) for c in caps]
        IL = (C.c_uint32 * nb)(*[nbytes] * nb)
        OA = (u8p * nb)(*[o.ctypes.data_as(u8p) for o in outs])
        OC = (C.c_uint64 * nb)(*caps)
        OL = (C.c_uint64 * nb)()
        first = []

        def call(knob):
            for i in range(nb):
                ins[i] = distinct[i % len(distinct)].copy()
            IA = (u8p * nb)(*[x.ctypes.data_as(u8p) for x in ins])
            os.environ["ZPAQ_AMD_DEVICE_E8"] = knob
            t0 = time.perf_counter()
            rc = L.zpq_compress_blocks(method.encode(), IA, IL, nb, None, None, 1, OA, OC, OL)
            dt = time.perf_counter() - t0
            assert rc == 0, (case, knob, L.zpq_last_error())
            got = [outs[i][:OL[i]].tobytes() for i in range(min(nb, 8))]
            if not first:
                first.extend(got)
            assert got == first, (case, knob, "the archives differ between the settings")
            for i in range(nb):
                assert np.array_equal(ins[i], want[i % len(want)]), (case, knob, i, "the caller's buffer is not the filtered block")
            return dt, int(L.zpq_last_device_e8_blocks())

        for knob in ("0", "1"):                                # warm-up: buffers, pinned staging
            call(knob)
        ms = {"0": [], "1": []}
        there = 0
        for _ in range(a.reps):
            for knob in ("0", "1"):
                dt, n = call(knob)
                ms[knob].append(round(dt * 1e3, 2))
                if knob == "1":
                    there = n
        row = {"method": method, "kind": kind, "block_bytes": nbytes, "blocks": nb, "ms": ms, "device_e8_blocks": there,
               "device_won_every_alternation": all(x < y for x, y in zip(ms["1"], ms["0"]))}
        rows.append(row)
        print(json.dumps(row), flush=True)
        dump()
    if skipped:
        print(json.dumps({"not_measured": skipped}), flush=True)
    os.environ.pop("ZPAQ_AMD_DEVICE_E8", None)
    L.zpq_shutdown()


if __name__ == "__main__":
    main()
