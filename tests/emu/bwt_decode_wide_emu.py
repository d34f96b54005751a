"""TEST INFRASTRUCTURE: build and run the emulator executable of the device's wide BWT decoder
(device/bwt_decode_wide_kernel.h through tests/emu/bwt_decode_wide_emu_main.cpp) with the helpers of bwt_decode_emu.py.  Used by
tests/test_emu_bwt_decode_wide.py."""
from __future__ import annotations

import subprocess
from typing import Optional, Sequence

import bwt_decode_emu


def build() -> str:
    return bwt_decode_emu.build(wide=True)


def run(mbits: int, streams: Sequence[bytes], caps: Optional[Sequence[Optional[int]]] = None, admit_only: bool = False, out_limit: int = 0):
    """One batch of streams of a BWT method whose program has pm = ph = mbits (25 .. 31) through the device's wide decoder:
    (overflow, [(status, out_len, output or None)] per stream, sub-batches that ran).  caps[k]: the room the caller has for stream
    k (None: enough); when an admitted stream does not fit, overflow is True and nothing runs, as in the engine.  out_limit: the
    bytes of output a sub-batch may hold (0: the engine's 2 GiB).  admit_only: the host's step alone."""
    return bwt_decode_emu.run_form(True, mbits, streams, caps, admit_only, out_limit)


def admitted(mbits: int, n: int):
    """The host's admission of a stream of n + 1 zeros with S[1] = 255 and idx = 1, which is never written out: (the wide form
    takes it, the small form takes it)."""
    r = subprocess.run([build(), "range", str(mbits), str(n)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"wide bwt decode emulator failed ({r.returncode}):\n" + r.stdout[-4000:])
    w = r.stdout.split()
    assert w[0] == "admitted" and w[2] == "small", r.stdout
    return w[1] == "1", w[3] == "1"
