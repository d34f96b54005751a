"""TEST INFRASTRUCTURE: build and run the emulator executable of the hash-table LZ77 parse (device/lz77_hash_kernel.h through
tests/emu/lz77_hash_emu_main.cpp).  Used by tests/test_emu_lz77_hash.py and tests/fuzz_lz77_hash_emu.py."""
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
    import zpaq_amd as z
    dev = os.path.join(ROOT, "zpaq_amd", "csrc", "device")
    srcs = (os.path.join(EMU, "wave_emu.h"), os.path.join(EMU, "wave_emu.cpp"), os.path.join(EMU, "lz77_hash_emu_main.cpp"),
            os.path.join(dev, "lz77_hash_kernel.h"), os.path.join(dev, "lz77_kernel.h"), os.path.join(dev, "layout.h"))
    flags = ("-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-g") if os.environ.get("ZPQ_EMU_SANITIZE") == "1" else ()
    key = hashlib.sha1(b"".join(open(p, "rb").read() for p in srcs) + " ".join(flags).encode()).hexdigest()[:20]
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"lz77_hash_{key}")
    if os.path.exists(exe):
        return exe
    libdir = os.path.dirname(z.library_path())
    tmp = f"{exe}.{os.getpid()}.tmp"
    cmd = ["g++", "-O2", "-std=c++17", "-w", *flags, "-I", EMU, "-I", dev, "-I", os.path.join(ROOT, "include"),
           os.path.join(EMU, "lz77_hash_emu_main.cpp"), os.path.join(EMU, "wave_emu.cpp"), "-L", libdir, "-lzpaq_amd", f"-Wl,-rpath,{libdir}", "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("lz77 hash emulator build failed:\n" + r.stdout[-6000:])
    os.replace(tmp, exe)
    return exe


def run(args9: Sequence[int], inputs: Sequence[bytes], idx_bits: int = -1):
    """One batch of blocks of a method with these args (makeConfig's nine) through the device's parser; per input the token list
    (16 bytes per match) the device would hand back.  idx_bits: -1 = the index the engine builds, else that many bits."""
    exe = build()
    a = list(args9)
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for k, data in enumerate(inputs):
            pth = os.path.join(td, f"in{k}")
            with open(pth, "wb") as fh:
                fh.write(bytes(data))
            paths.append(pth)
        prefix = os.path.join(td, "out")
        r = subprocess.run([exe, str(a[1] & 3), str(a[2]), str(a[3]), str(a[6]), str((1 << a[4]) - 1), str(12 - a[0]), str(a[5]), str(idx_bits), prefix, *paths],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"lz77 hash emulator failed ({r.returncode}):\n" + r.stdout[-4000:])
        return [open(f"{prefix}.{k}", "rb").read() for k in range(len(inputs))]
