"""TEST INFRASTRUCTURE: build and run the emulator executable of the device's LZ77 decoder for streams parsed in pieces
(device/lz77_decode_wide_kernel.h through tests/emu/lz77_decode_wide_emu_main.cpp).  Used by tests/test_emu_lz77_decode_wide.py."""
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
            os.path.join(EMU, "lz77_decode_wide_emu_main.cpp"), os.path.join(dev, "lz77_decode_wide_kernel.h"),
            os.path.join(dev, "lz77_decode_kernel.h"), os.path.join(dev, "layout.h"))
    flags = ("-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-g") if os.environ.get("ZPQ_EMU_SANITIZE") == "1" else ()
    key = hashlib.sha1(b"".join(open(p, "rb").read() for p in srcs) + " ".join(flags).encode()).hexdigest()[:20]
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"lz77_decode_wide_{key}")
    if os.path.exists(exe):
        return exe
    tmp = f"{exe}.{os.getpid()}.tmp"
    cmd = ["g++", "-O2", "-std=c++17", "-w", *flags, "-I", EMU, "-I", dev, "-I", os.path.join(ROOT, "include"),
           os.path.join(EMU, "lz77_decode_wide_emu_main.cpp"), os.path.join(EMU, "wave_emu.cpp"), "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("lz77 wide decode emulator build failed:\n" + r.stdout[-6000:])
    os.replace(tmp, exe)
    return exe


def run(args9: Sequence[int], streams: Sequence[bytes], piece: int, caps: Optional[Sequence[Optional[int]]] = None):
    """One batch of streams of a method with these args (makeConfig's nine) through the decoder, in pieces of `piece` stream bytes:
    (overflow, [(status, out_len, ntok, output or None)] per stream, (pieces, entered, met, walked), jump rounds or None).
    caps[k]: the room the caller has for stream k (None: enough); when a decoded stream does not fit, overflow is True and no
    output is written, as in the engine."""
    exe = build()
    a = list(args9)
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for k, s in enumerate(streams):
            pth = os.path.join(td, f"in{k}")
            with open(pth, "wb") as fh:
                fh.write(bytes(s))
            paths.append(pth if not caps or caps[k] is None else f"{pth}:{caps[k]}")
        prefix = os.path.join(td, "out")
        r = subprocess.run([exe, str(a[1] & 3), str(max(a[0] - 4, 0)), str(a[2]), str(a[0] + 20), str(piece), prefix, *paths],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"lz77 wide decode emulator failed ({r.returncode}):\n" + r.stdout[-4000:])
        lines = r.stdout.splitlines()
        overflow = "overflow" in lines
        pieces = tuple(int(x) for x in lines[len(streams)].split()[1:])
        assert lines[len(streams)].startswith("pieces ") and len(pieces) == 4, r.stdout[-400:]
        rounds = None
        if not overflow:
            assert lines[len(streams) + 1].startswith("rounds "), r.stdout[-400:]
            rounds = int(lines[len(streams) + 1].split()[1])
        res = []
        for k in range(len(streams)):
            w = lines[k].split()
            assert w[0] == "stream" and int(w[1]) == k, r.stdout[:400]
            status, out_len, ntok = int(w[3]), int(w[5]), int(w[7])
            out = None
            pth = f"{prefix}.{k}"
            if os.path.exists(pth):
                assert status == 0 and not overflow
                out = open(pth, "rb").read()
                assert len(out) == out_len
            else:
                assert status != 0 or overflow
            res.append((status, out_len, ntok, out))
        return overflow, res, pieces, rounds
