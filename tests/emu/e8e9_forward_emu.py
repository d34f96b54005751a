"""TEST INFRASTRUCTURE: build and run the emulator executable of the device's forward E8E9 filter (device/e8e9_forward_kernel.h through
tests/emu/e8e9_forward_emu_main.cpp).  Used by tests/test_emu_e8e9_forward.py."""
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
            os.path.join(EMU, "e8e9_forward_emu_main.cpp"), os.path.join(dev, "e8e9_forward_kernel.h"), os.path.join(dev, "layout.h"))
    flags = ("-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-g") if os.environ.get("ZPQ_EMU_SANITIZE") == "1" else ()
    key = hashlib.sha1(b"".join(open(p, "rb").read() for p in srcs) + " ".join(flags).encode()).hexdigest()[:20]
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"e8e9_forward_{key}")
    if os.path.exists(exe):
        return exe
    tmp = f"{exe}.{os.getpid()}.tmp"
    cmd = ["g++", "-O2", "-std=c++17", "-w", *flags, "-I", EMU, "-I", dev, "-I", os.path.join(ROOT, "include"),
           os.path.join(EMU, "e8e9_forward_emu_main.cpp"), os.path.join(EMU, "wave_emu.cpp"), "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("e8e9 forward emulator build failed:\n" + r.stdout[-6000:])
    os.replace(tmp, exe)
    return exe


def run(blocks: Sequence[bytes], max_steps: int = 0):
    """One batch of blocks through the device's inverse filter: [(status, output or None)] per block.  max_steps: the walk's cap
    on serial steps (0: the engine's)."""
    exe = build()
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for k, s in enumerate(blocks):
            pth = os.path.join(td, f"in{k}")
            with open(pth, "wb") as fh:
                fh.write(bytes(s))
            paths.append(pth)
        prefix = os.path.join(td, "out")
        r = subprocess.run([exe, "run", str(max_steps), prefix, *paths], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"e8e9 forward emulator failed ({r.returncode}):\n" + r.stdout[-4000:])
        lines = r.stdout.splitlines()
        res = []
        for k in range(len(blocks)):
            w = lines[k].split()
            assert w[0] == "block" and int(w[1]) == k, r.stdout[:400]
            status = int(w[3])
            out = None
            pth = f"{prefix}.{k}"
            if os.path.exists(pth):
                assert status == 0
                out = open(pth, "rb").read()
                assert len(out) == int(w[5])
            else:
                assert status != 0
            res.append((status, out))
        return res
