"""TEST INFRASTRUCTURE: build and run the emulator executable of fragmenting on the device (device/fragment_kernel.h and
device/fragment_stitch.hpp through tests/emu/fragment_emu_main.cpp).  Used by tests/test_emu_fragment.py."""
from __future__ import annotations

import hashlib
import os
import struct
import subprocess
import tempfile
from typing import Sequence

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EMU = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(ROOT, "build", "emu")


def build() -> str:
    dev = os.path.join(ROOT, "zpaq_amd", "csrc", "device")
    srcs = (os.path.join(EMU, "wave_emu.h"), os.path.join(EMU, "wave_emu.cpp"), os.path.join(EMU, "guard_alloc.h"),
            os.path.join(EMU, "fragment_emu_main.cpp"), os.path.join(dev, "fragment_kernel.h"), os.path.join(dev, "fragment_stitch.hpp"),
            os.path.join(dev, "layout.h"))
    flags = ("-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-g") if os.environ.get("ZPQ_EMU_SANITIZE") == "1" else ()
    key = hashlib.sha1(b"".join(open(p, "rb").read() for p in srcs) + " ".join(flags).encode()).hexdigest()[:20]
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"fragment_{key}")
    if os.path.exists(exe):
        return exe
    tmp = f"{exe}.{os.getpid()}.tmp"
    cmd = ["g++", "-O2", "-std=c++17", "-w", *flags, "-I", EMU, "-I", dev, "-I", os.path.join(ROOT, "include"),
           os.path.join(EMU, "fragment_emu_main.cpp"), os.path.join(EMU, "wave_emu.cpp"), "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("fragment emulator build failed:\n" + r.stdout[-6000:])
    os.replace(tmp, exe)
    return exe


def run(files: Sequence[bytes], piece: int, min_frag: int, max_frag: int, thresh: int):
    """One batch of files through the walk kernel and the stitch: (fix-up rounds, per file [(size, hits, o1)])."""
    exe = build()
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for k, s in enumerate(files):
            pth = os.path.join(td, f"in{k}")
            with open(pth, "wb") as fh:
                fh.write(bytes(s))
            paths.append(pth)
        out = os.path.join(td, "out")
        r = subprocess.run([exe, "run", str(piece), str(min_frag), str(max_frag), str(thresh), out, *paths], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"fragment emulator failed ({r.returncode}):\n" + r.stdout[-4000:])
        lines = r.stdout.splitlines()
        assert lines[0].split()[0] == "rounds", r.stdout[:400]
        rounds = int(lines[0].split()[1])
        blob = open(out, "rb").read()
        res, at = [], 0
        for k in range(len(files)):
            w = lines[1 + k].split()
            assert w[0] == "file" and int(w[1]) == k, r.stdout[:400]
            fr, start = [], 0
            for _ in range(int(w[3])):
                end, hits = struct.unpack_from("<II", blob, at)
                fr.append((end - start, hits, blob[at + 8:at + 264]))
                start = end
                at += 264
            res.append(fr)
        assert at == len(blob)
        return rounds, res
