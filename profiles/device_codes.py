#!/usr/bin/env python3
"""Where LZBuffer's codes of a device-parsed batch should be written: end-to-end zpq_compress_blocks time with the coder on the
device (ZPAQ_AMD_DEVICE_CODES=1) and on the host (=0, the previous path: the list of matches comes back and a host core writes
the stream), by a host clock around the call, after one warm-up call per setting, the two settings alternating `--reps` times in
one process.  DESIGN 4.5.2 has the table this prints.

    python profiles/device_codes.py [--cases CASE ...] [--reps 3] [--knobs 1,0] [--out FILE]

Cases: <method>:<kind>:<block bytes>:<blocks>.  Inputs: up to 64 distinct blocks of zpaq_amd.corpus, repeated to the count asked
for.  Archives of the two settings are compared with each other, every call.  Per case: the calls' milliseconds, front_ms of
zpq_last_api_timing (everything in front of the coder's device batch: the parse and the codes are in it), MB/s of the best call,
the blocks coded on the device, and the bytes that came back over PCIe behind the parse -- 16 per match with the knob at 0, the
stream with it at 1 -- counted from the host's parse of the distinct blocks (the device's list is the host's)."""
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
    [f"1:text:{MIB}:{nb}" for nb in (4, 64, 256, 1024)]
    + [f"x0,1,4,0,3,20:text:{MIB - 4096}:{nb}" for nb in (4, 64, 256, 1024)]      # (x0: blocks of at most 1 MiB - 4 KiB)
    + [f"3:lcg:{256 * 1024}:256", f"1:zeros:{MIB}:256", f"1:records:{MIB}:256"]
)
u8p = C.POINTER(C.c_ubyte)
u32p = C.POINTER(C.c_uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=DEFAULT_CASES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--knobs", default="1,0", help="settings to alternate: 1, 0, auto (the variable unset: the engine decides per batch)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import zpaq_amd as z
    from zpaq_amd import corpus
    L = z.lib()
    z.init(0)
    L.zpq_lz77_tokens_host.argtypes = [C.c_char_p, u8p, C.c_uint32, u32p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.zpq_preprocess_block.argtypes = [C.c_char_p, u8p, C.c_uint32, u8p, C.c_size_t, C.POINTER(C.c_size_t)]
    knobs = tuple(a.knobs.split(","))
    rows = []
    ph = (C.c_double * 8)()
    for case in a.cases:
        method, kind, nbytes, nb = case.split(":")
        nbytes, nb = int(nbytes), int(nb)
        distinct = [corpus.block(kind, nbytes, 7000 + i) for i in range(min(nb, 64))]
        # what crosses PCIe back behind the parse, per distinct block: the list (16 bytes per match) or the stream
        back = {"1": [], "0": []}                          # (auto: whichever of the two the engine took)
        for d in distinct:
            args = z.method_to_header(z.expand_method(method, d))[2]
            if (args[1] & 3) not in (1, 2) or args[1] > 7:
                back["1"].append(0)
                back["0"].append(0)
                continue
            xm = z.expand_method(method, d)
            buf = d.copy()
            toks = np.zeros(4 * (nbytes + 4), np.uint32)
            cnt = C.c_size_t(0)
            assert L.zpq_lz77_tokens_host(xm.encode(), buf.ctypes.data_as(u8p), nbytes, toks.ctypes.data_as(u32p), nbytes + 4, C.byref(cnt)) == 0
            out = np.empty(2 * nbytes + 4096, np.uint8)
            ol = C.c_size_t(0)
            buf = d.copy()
            assert L.zpq_preprocess_block(xm.encode(), buf.ctypes.data_as(u8p), nbytes, out.ctypes.data_as(u8p), out.size, C.byref(ol)) == 0
            back["0"].append(16 * cnt.value)
            back["1"].append(ol.value)
        ins = [distinct[i % len(distinct)].copy() for i in range(nb)]
        caps = [nbytes + nbytes // 4 + 8192] * nb
        outs = [np.empty(c, np.uint8) for c in caps]
        IA = (u8p * nb)(*[x.ctypes.data_as(u8p) for x in ins])
        IL = (C.c_uint32 * nb)(*[nbytes] * nb)
        OA = (u8p * nb)(*[x.ctypes.data_as(u8p) for x in outs])
        OC = (C.c_uint64 * nb)(*caps)
        OL = (C.c_uint64 * nb)()

        def call(knob):
            if knob == "auto":
                os.environ.pop("ZPAQ_AMD_DEVICE_CODES", None)
            else:
                os.environ["ZPAQ_AMD_DEVICE_CODES"] = knob
            for k in range(nb):                                # (E8E9 methods rewrite the caller's buffers)
                np.copyto(ins[k], distinct[k % len(distinct)])
            t0 = time.perf_counter()
            rc = L.zpq_compress_blocks(method.encode(), IA, IL, nb, None, None, 1, OA, OC, OL)
            dt = time.perf_counter() - t0
            assert rc == 0, (case, knob, L.zpq_last_error())
            L.zpq_last_api_timing(ph)
            h = hashlib.sha1()
            for k in range(nb):
                h.update(outs[k][:OL[k]].tobytes())
            return dt, h.hexdigest(), int(L.zpq_last_device_coded_blocks()), float(ph[1]), sum(int(x) for x in OL)

        digests = set()
        for k in knobs:                                        # warm-up: buffers, pinned staging, code objects
            digests.add(call(k)[1])
        times = {k: [] for k in knobs}
        fronts = {k: [] for k in knobs}
        coded = {}
        size = 0
        for _ in range(a.reps):
            for k in knobs:
                dt, dg, cnt, front, size = call(k)
                times[k].append(round(dt * 1e3, 2))
                fronts[k].append(round(front, 2))
                coded[k] = cnt
                digests.add(dg)
        assert len(digests) == 1, (case, "the settings made different archives")
        for k in knobs:
            back.setdefault(k, back["1"] if coded[k] else back["0"])
        row = {"method": method, "kind": kind, "block_bytes": nbytes, "blocks": nb, "archive_bytes": size, "archives_sha1": digests.pop()[:12],
               "ms": times, "front_ms": fronts, "mb_per_s": {k: round(nbytes * nb / 1e6 / (min(times[k]) / 1e3), 1) for k in knobs},
               "device_coded_blocks": coded,
               "pcie_back_bytes": {k: sum(back[k][i % len(distinct)] for i in range(nb)) for k in knobs},
               "not_slower_in_any_alternation": all(x <= y for x, y in zip(times[knobs[0]], times[knobs[-1]]))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
    L.zpq_shutdown()


if __name__ == "__main__":
    main()
