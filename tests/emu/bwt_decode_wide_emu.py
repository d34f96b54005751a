"""TEST INFRASTRUCTURE: build and run the emulator executable of the device's wide BWT decoder
(device/bwt_decode_wide_kernel.h through tests/emu/bwt_decode_wide_emu_main.cpp).  Used by tests/test_emu_bwt_decode_wide.py."""
from __future__ import annotations

import hashlib
import os
import subprocess
import tempfile
from typing import Optional, Sequence

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EMU = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(ROOT, "build", "emu")


def build() -> str:
    dev = os.path.join(ROOT, "zpaq_amd", "csrc", "device")
    srcs = (os.path.join(EMU, "wave_emu.h"), os.path.join(EMU, "wave_emu.cpp"), os.path.join(EMU, "guard_alloc.h"),
            os.path.join(EMU, "bwt_decode_wide_emu_main.cpp"), os.path.join(dev, "bwt_decode_wide_kernel.h"),
            os.path.join(dev, "bwt_decode_kernel.h"), os.path.join(dev, "layout.h"))
    flags = ("-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-g") if os.environ.get("ZPQ_EMU_SANITIZE") == "1" else ()
    key = hashlib.sha1(b"".join(open(p, "rb").read() for p in srcs) + " ".join(flags).encode()).hexdigest()[:20]
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"bwt_decode_wide_{key}")
    if os.path.exists(exe):
        return exe
    tmp = f"{exe}.{os.getpid()}.tmp"
    cmd = ["g++", "-O2", "-std=c++17", "-w", *flags, "-I", EMU, "-I", dev, "-I", os.path.join(ROOT, "include"),
           os.path.join(EMU, "bwt_decode_wide_emu_main.cpp"), os.path.join(EMU, "wave_emu.cpp"), "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("wide bwt decode emulator build failed:\n" + r.stdout[-6000:])
    os.replace(tmp, exe)
    return exe


def run(mbits: int, streams: Sequence[bytes], caps: Optional[Sequence[Optional[int]]] = None, admit_only: bool = False, out_limit: int = 0):
    """One batch of streams of a BWT method whose program has pm = ph = mbits (25 .. 31) through the device's wide decoder:
    (overflow, [(status, out_len, output or None)] per stream, sub-batches that ran).  caps[k]: the room the caller has for stream
    k (None: enough); when an admitted stream does not fit, overflow is True and nothing runs, as in the engine.  out_limit: the
    bytes of output a sub-batch may hold (0: the engine's 2 GiB).  admit_only: the host's step alone."""
    exe = build()
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for k, s in enumerate(streams):
            pth = os.path.join(td, f"in{k}")
            with open(pth, "wb") as fh:
                fh.write(bytes(s))
            paths.append(pth if not caps or caps[k] is None else f"{pth}:{caps[k]}")
        prefix = os.path.join(td, "out")
        r = subprocess.run([exe, "admit" if admit_only else "run", str(mbits), str(out_limit), prefix, *paths], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"wide bwt decode emulator failed ({r.returncode}):\n" + r.stdout[-4000:])
        lines = r.stdout.splitlines()
        overflow = "overflow" in lines
        batches = next((int(ln.split()[1]) for ln in lines if ln.startswith("batches ")), 0)
        res = []
        for k in range(len(streams)):
            w = lines[k].split()
            assert w[0] == "stream" and int(w[1]) == k, r.stdout[:400]
            status, out_len = int(w[3]), int(w[5])
            out = None
            pth = f"{prefix}.{k}"
            if os.path.exists(pth):
                assert status == 0 and not overflow and not admit_only
                out = open(pth, "rb").read()
                assert len(out) == out_len
            else:
                assert status != 0 or overflow or admit_only
            res.append((status, out_len, out))
        return overflow, res, batches


def admitted(mbits: int, n: int):
    """The host's admission of a stream of n + 1 zeros with S[1] = 255 and idx = 1, which is never written out: (the wide form
    takes it, the small form takes it)."""
    r = subprocess.run([build(), "range", str(mbits), str(n)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"wide bwt decode emulator failed ({r.returncode}):\n" + r.stdout[-4000:])
    w = r.stdout.split()
    assert w[0] == "admitted" and w[2] == "small", r.stdout
    return w[1] == "1", w[3] == "1"
