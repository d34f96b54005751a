"""TEST INFRASTRUCTURE: build and run the emulator executable of the device's LZ77 parse of one block in pieces
(device/lz77_wide_kernel.h through tests/emu/lz77_wide_emu_main.cpp).  Used by tests/test_emu_lz77_wide.py."""
from __future__ import annotations

import hashlib
import os
import subprocess
import tempfile
from typing import Sequence

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EMU = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(ROOT, "build", "emu")


def build(sanitize: bool = False) -> str:
    """sanitize: with -fsanitize=address,undefined (a program with its own main: it needs no preload)."""
    import zpaq_amd as z
    dev = os.path.join(ROOT, "zpaq_amd", "csrc", "device")
    srcs = (os.path.join(EMU, "wave_emu.h"), os.path.join(EMU, "wave_emu.cpp"), os.path.join(EMU, "guard_alloc.h"),
            os.path.join(EMU, "lz77_wide_emu_main.cpp"), os.path.join(dev, "lz77_wide_kernel.h"), os.path.join(dev, "lz77_kernel.h"),
            os.path.join(dev, "layout.h"), os.path.join(dev, "lz77_wide_layout.h"))
    flags = ("-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g") if sanitize or os.environ.get("ZPQ_EMU_SANITIZE") == "1" else ()
    key = hashlib.sha1(b"".join(open(p, "rb").read() for p in srcs) + " ".join(flags).encode()).hexdigest()[:20]
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"lz77_wide_{key}")
    if os.path.exists(exe):
        return exe
    tmp = f"{exe}.{os.getpid()}.tmp"
    libdir = os.path.dirname(z.library_path())
    cmd = ["g++", "-O1", "-std=c++17", "-w", *flags, "-I", EMU, "-I", dev, "-I", os.path.join(ROOT, "include"), os.path.join(EMU, "lz77_wide_emu_main.cpp"),
           os.path.join(EMU, "wave_emu.cpp"), "-L", libdir, "-lzpaq_amd", f"-Wl,-rpath,{libdir}", "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("wide LZ77 emulator build failed:\n" + r.stdout[-6000:])
    os.replace(tmp, exe)
    return exe


def run(kind: int, min_match: int, lookahead: int, bucket: int, checkbits: int, pieces: Sequence[int], blocks: Sequence[bytes],
        names: Sequence[str] | None = None, sanitize: bool = False):
    """Every block alone through the emulated search and, once per piece size, the piece walk, the stitch and the gather, all in
    one process: per block and piece size (the final token list as bytes, 16 per match; (pieces, adopted whole, re-joined after a
    re-walk, own tokens only or nothing)).  A piece size of 0 is one piece that holds the block.  A guard page hit raises, naming
    the block."""
    exe = build(sanitize)
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for k, data in enumerate(blocks):
            pth = os.path.join(td, f"in{k}")
            with open(pth, "wb") as fh:
                fh.write(bytes(data))
            paths.append(pth)
        prefix = os.path.join(td, "out")
        r = subprocess.run([exe, str(kind), str(min_match), str(lookahead), str(bucket), str(checkbits), ",".join(str(int(p)) for p in pieces), prefix, *paths],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
        lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("block ")]
        if r.returncode != 0:
            at = len(lines) // len(pieces)
            raise RuntimeError(f"wide LZ77 emulator failed ({r.returncode}) in block {at}" + (f" ({names[at]})" if names and at < len(names) else "") +
                               ":\n" + r.stdout[-1000:])
        assert len(lines) == len(blocks) * len(pieces), r.stdout[-1000:]
        res = []
        for k in range(len(blocks)):
            per = []
            for j in range(len(pieces)):
                w = lines[k * len(pieces) + j]
                assert int(w[1]) == k and int(w[3]) == len(blocks[k]) and int(w[5]) == j, w
                toks = open(f"{prefix}.{k}.{j}", "rb").read()
                assert len(toks) == 16 * int(w[7]), w
                per.append((toks, (int(w[9]), int(w[11]), int(w[13]), int(w[15]))))
            res.append(per)
        return res
