"""TEST INFRASTRUCTURE: build and run the emulator executable of the device's decoder for long LZ77 streams with the inverse E8E9
filter behind it (device/lz77_decode_wide_kernel.h and device/e8e9_kernel.h through tests/emu/lz77_decode_wide_e8_emu_main.cpp).
Used by tests/test_emu_e8e9_decode_wide.py."""
from __future__ import annotations

import hashlib
import os
import subprocess
import tempfile
from typing import Sequence

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EMU = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(ROOT, "build", "emu")


def build() -> str:
    dev = os.path.join(ROOT, "zpaq_amd", "csrc", "device")
    srcs = (os.path.join(EMU, "wave_emu.h"), os.path.join(EMU, "wave_emu.cpp"), os.path.join(EMU, "guard_alloc.h"),
            os.path.join(EMU, "lz77_decode_wide_e8_emu_main.cpp"), os.path.join(dev, "lz77_decode_wide_kernel.h"),
            os.path.join(dev, "lz77_decode_kernel.h"), os.path.join(dev, "e8e9_kernel.h"), os.path.join(dev, "layout.h"))
    flags = ("-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-g") if os.environ.get("ZPQ_EMU_SANITIZE") == "1" else ()
    key = hashlib.sha1(b"".join(open(p, "rb").read() for p in srcs) + " ".join(flags).encode()).hexdigest()[:20]
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"lz77_decode_wide_e8_{key}")
    if os.path.exists(exe):
        return exe
    tmp = f"{exe}.{os.getpid()}.tmp"
    cmd = ["g++", "-O2", "-std=c++17", "-w", *flags, "-I", EMU, "-I", dev, "-I", os.path.join(ROOT, "include"),
           os.path.join(EMU, "lz77_decode_wide_e8_emu_main.cpp"), os.path.join(EMU, "wave_emu.cpp"), "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("lz77 wide decode + e8e9 emulator build failed:\n" + r.stdout[-6000:])
    os.replace(tmp, exe)
    return exe


def run(args9: Sequence[int], streams: Sequence[bytes], piece: int, max_steps: int = 0):
    """One batch of streams of an x.,5 / x.,6 method with these args (makeConfig's nine) through the decoder in pieces of `piece`
    stream bytes and the filter (max_steps: the walk's cap on serial steps, 0: the engine's):
    ([(status, out_len, output or None, listed)] per stream, (pieces, entered, met, walked), jump rounds, launches).
    listed: the stream's output was in the filter's list; launches: kernels started behind the host's placement."""
    exe = build()
    a = list(args9)
    assert a[1] in (5, 6), a
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for k, s in enumerate(streams):
            pth = os.path.join(td, f"in{k}")
            with open(pth, "wb") as fh:
                fh.write(bytes(s))
            paths.append(pth)
        prefix = os.path.join(td, "out")
        r = subprocess.run([exe, str(a[1] - 4), str(max(a[0] - 4, 0)), str(a[2]), str(a[0] + 20), str(piece), str(max_steps), prefix, *paths],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"lz77 wide decode + e8e9 emulator failed ({r.returncode}):\n" + r.stdout[-4000:])
        lines = r.stdout.splitlines()
        n = len(streams)
        assert lines[n].startswith("pieces ") and lines[n + 1].startswith("rounds ") and lines[n + 2].startswith("launches "), r.stdout[-400:]
        assert lines[n + 3] == "edges ok", r.stdout[-400:]
        pieces = tuple(int(x) for x in lines[n].split()[1:])
        rounds, launches = int(lines[n + 1].split()[1]), int(lines[n + 2].split()[1])
        res = []
        for k in range(n):
            w = lines[k].split()
            assert w[0] == "stream" and int(w[1]) == k, r.stdout[:400]
            status, out_len, listed = int(w[3]), int(w[5]), bool(int(w[9]))
            out = None
            pth = f"{prefix}.{k}"
            if os.path.exists(pth):
                assert status == 0
                out = open(pth, "rb").read()
                assert len(out) == out_len
            else:
                assert status != 0
            res.append((status, out_len, out, listed))
        return res, pieces, rounds, launches
