"""TEST INFRASTRUCTURE: build and run the emulator executable of the device's wide suffix sort (device/sa_wide_kernel.h through
tests/emu/sa_wide_emu_main.cpp).  Used by tests/test_emu_sa_wide.py."""
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
            os.path.join(EMU, "sa_wide_emu_main.cpp"), os.path.join(dev, "sa_wide_kernel.h"), os.path.join(dev, "sa_kernel.h"))
    flags = ("-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-g") if os.environ.get("ZPQ_EMU_SANITIZE") == "1" else ()
    key = hashlib.sha1(b"".join(open(p, "rb").read() for p in srcs) + " ".join(flags).encode()).hexdigest()[:20]
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"sa_wide_{key}")
    if os.path.exists(exe):
        return exe
    tmp = f"{exe}.{os.getpid()}.tmp"
    cmd = ["g++", "-O1", "-std=c++17", "-w", *flags, "-I", EMU, "-I", dev, os.path.join(EMU, "sa_wide_emu_main.cpp"),
           os.path.join(EMU, "wave_emu.cpp"), "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("wide suffix sort emulator build failed:\n" + r.stdout[-6000:])
    os.replace(tmp, exe)
    return exe


def run(blocks: Sequence[bytes], rank_bits: int = 0, names: Sequence[str] | None = None):
    """Every block alone through the emulated wide sort, all in one process: per block (suffix array, final ranks -- numpy
    uint32 --, the BWT stream as bytes, rounds).  rank_bits: the forced field width (0: the natural one).  A guard page hit or
    a loop that does not end raises, naming the block."""
    import numpy as np
    exe = build()
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for k, data in enumerate(blocks):
            pth = os.path.join(td, f"in{k}")
            with open(pth, "wb") as fh:
                fh.write(bytes(data))
            paths.append(pth)
        prefix = os.path.join(td, "out")
        r = subprocess.run([exe, "sort", str(rank_bits), prefix, *paths], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
        lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("block ")]
        if r.returncode != 0:
            at = len(lines)
            raise RuntimeError(f"wide suffix sort emulator failed ({r.returncode}) in block {at}" + (f" ({names[at]})" if names and at < len(names) else "") +
                               ":\n" + r.stdout[-1000:])
        assert len(lines) == len(blocks), r.stdout[-1000:]
        res = []
        for k, w in enumerate(lines):
            assert int(w[1]) == k and int(w[3]) == len(blocks[k]), w
            res.append((np.fromfile(f"{prefix}.{k}.sa", "<u4"), np.fromfile(f"{prefix}.{k}.rank", "<u4"), open(f"{prefix}.{k}.bwt", "rb").read(),
                        int(w[7])))
        return res


def helper(*words) -> int:
    """The host helpers of device/sa_wide_kernel.h: helper("bits", n) = sa_wide_rank_bits(n), helper("field", r, h) = sa_wide_field_bits(r, h)."""
    r = subprocess.run([build(), *[str(w) for w in words]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"wide suffix sort emulator failed ({r.returncode}):\n" + r.stdout[-4000:])
    return int(r.stdout.split()[1])
