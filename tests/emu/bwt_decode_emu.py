"""TEST INFRASTRUCTURE: build and run the emulator executables of the device's BWT decoders (device/bwt_decode_kernel.h through
tests/emu/bwt_decode_emu_main.cpp, device/bwt_decode_wide_kernel.h through tests/emu/bwt_decode_wide_emu_main.cpp; both are
tests/emu/bwt_decode_emu_driver.h).  Used by tests/test_emu_bwt_decode.py and, through bwt_decode_wide_emu.py, by
tests/test_emu_bwt_decode_wide.py."""
from __future__ import annotations

import hashlib
import os
import subprocess
import tempfile
from typing import Optional, Sequence

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EMU = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(ROOT, "build", "emu")


def build(wide: bool = False) -> str:
    dev = os.path.join(ROOT, "zpaq_amd", "csrc", "device")
    name = "bwt_decode_wide" if wide else "bwt_decode"
    main = os.path.join(EMU, f"{name}_emu_main.cpp")
    srcs = (os.path.join(EMU, "wave_emu.h"), os.path.join(EMU, "wave_emu.cpp"), os.path.join(EMU, "guard_alloc.h"), main,
            os.path.join(EMU, "bwt_decode_emu_driver.h"), os.path.join(dev, "bwt_decode_wide_kernel.h"),
            os.path.join(dev, "bwt_decode_kernel.h"), os.path.join(dev, "layout.h"))
    flags = ("-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-g") if os.environ.get("ZPQ_EMU_SANITIZE") == "1" else ()
    key = hashlib.sha1(b"".join(open(p, "rb").read() for p in srcs) + " ".join(flags).encode()).hexdigest()[:20]
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"{name}_{key}")
    if os.path.exists(exe):
        return exe
    tmp = f"{exe}.{os.getpid()}.tmp"
    cmd = ["g++", "-O2", "-std=c++17", "-w", *flags, "-I", EMU, "-I", dev, "-I", os.path.join(ROOT, "include"),
           main, os.path.join(EMU, "wave_emu.cpp"), "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{name} emulator build failed:\n" + r.stdout[-6000:])
    os.replace(tmp, exe)
    return exe


def run_form(wide: bool, mbits: int, streams: Sequence[bytes], caps: Optional[Sequence[Optional[int]]], admit_only: bool, out_limit: int):
    """One batch of streams through the decoder of one form: (overflow, [(status, out_len, output or None)] per stream,
    sub-batches that ran)."""
    exe = build(wide)
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
            raise RuntimeError(f"bwt decode emulator failed ({r.returncode}):\n" + r.stdout[-4000:])
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


def run(mbits: int, streams: Sequence[bytes], caps: Optional[Sequence[Optional[int]]] = None, admit_only: bool = False):
    """One batch of streams of a BWT method whose program has pm = ph = mbits through the device's decoder:
    (overflow, [(status, out_len, output or None)] per stream).  caps[k]: the room the caller has for stream k (None: enough); when
    an admitted stream does not fit, overflow is True and nothing runs, as in the engine.  admit_only: the host's step alone."""
    overflow, res, _ = run_form(False, mbits, streams, caps, admit_only, 0)
    return overflow, res
