"""TEST INFRASTRUCTURE: build and run the emulator executable of the device's LZ77 coder (device/lz77_codes_kernel.h through
tests/emu/lz77_codes_emu_main.cpp).  Used by tests/test_emu_lz77_codes.py."""
from __future__ import annotations

import hashlib
import os
import subprocess
import tempfile
from typing import Sequence, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EMU = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(ROOT, "build", "emu")


def build() -> str:
    dev = os.path.join(ROOT, "zpaq_amd", "csrc", "device")
    srcs = (os.path.join(EMU, "wave_emu.h"), os.path.join(EMU, "wave_emu.cpp"), os.path.join(EMU, "lz77_codes_emu_main.cpp"),
            os.path.join(dev, "lz77_codes_kernel.h"), os.path.join(dev, "lz77_kernel.h"), os.path.join(dev, "layout.h"))
    flags = ("-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-g") if os.environ.get("ZPQ_EMU_SANITIZE") == "1" else ()
    key = hashlib.sha1(b"".join(open(p, "rb").read() for p in srcs) + " ".join(flags).encode()).hexdigest()[:20]
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"lz77_codes_{key}")
    if os.path.exists(exe):
        return exe
    tmp = f"{exe}.{os.getpid()}.tmp"
    cmd = ["g++", "-O2", "-std=c++17", "-w", *flags, "-I", EMU, "-I", dev, "-I", os.path.join(ROOT, "include"),
           os.path.join(EMU, "lz77_codes_emu_main.cpp"), os.path.join(EMU, "wave_emu.cpp"), "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("lz77 codes emulator build failed:\n" + r.stdout[-6000:])
    os.replace(tmp, exe)
    return exe


def run(args9: Sequence[int], blocks: Sequence[Tuple[bytes, bytes]]):
    """One batch of (block, token list) pairs of a method with these args (makeConfig's nine) through the device's coder:
    (error word, the streams -- None when the word is set: nothing is emitted then)."""
    exe = build()
    a = list(args9)
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for k, (data, toks) in enumerate(blocks):
            for name, content in ((f"in{k}", data), (f"tok{k}", toks)):
                pth = os.path.join(td, name)
                with open(pth, "wb") as fh:
                    fh.write(bytes(content))
                paths.append(pth)
        prefix = os.path.join(td, "out")
        r = subprocess.run([exe, str(a[1] & 3), str(a[2]), str(max(a[0] - 4, 0)), prefix, *paths], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"lz77 codes emulator failed ({r.returncode}):\n" + r.stdout[-4000:])
        first = r.stdout.splitlines()[0].split()
        assert first[0] == "error", r.stdout[:200]
        err = int(first[1])
        if err:
            assert not any(os.path.exists(f"{prefix}.{k}") for k in range(len(blocks)))
            return err, None
        return 0, [open(f"{prefix}.{k}", "rb").read() for k in range(len(blocks))]
