"""TEST INFRASTRUCTURE: build and run the emulator executable of the device's generic post-processor for one PCOMP program
(zpq_pcomp_source's text -- device/pcomp_kernel.h with pcomp_body and the program as host/codegen.cpp translates it -- in front of
tests/emu/pcomp_emu_main.cpp).  Used by tests/test_emu_pcomp.py and tests/fuzz_pcomp.py."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
import tempfile
from typing import Optional, Sequence

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EMU = os.path.join(ROOT, "tests", "emu")
BUILD = os.path.join(ROOT, "build", "emu")
DEV = os.path.join(ROOT, "zpaq_amd", "csrc", "device")


def source(code: bytes, ph: int, pm: int) -> str:
    """zpq_pcomp_source: the translation unit the engine hands to hipRTC for this program."""
    import zpaq_amd as z
    L = z.lib()
    L.zpq_pcomp_source.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p]
    buf = C.create_string_buffer(4 << 20)
    ln = C.c_size_t(0)
    key = C.create_string_buffer(41)
    if L.zpq_pcomp_source(bytes(code), len(code), ph, pm, buf, len(buf), C.byref(ln), key) != 0:
        raise RuntimeError(L.zpq_last_error().decode())
    return buf.value.decode()


def build(code: bytes, ph: int, pm: int) -> str:
    """Compile the emulator executable for this program (cached under build/emu); returns its path."""
    src = source(code, ph, pm)
    dev = DEV
    deps = b"".join(open(p, "rb").read() for p in (
        os.path.join(EMU, "wave_emu.h"), os.path.join(EMU, "wave_emu.cpp"), os.path.join(EMU, "pcomp_emu_main.cpp"), os.path.join(EMU, "guard_alloc.h"),
        os.path.join(dev, "pcomp_kernel.h"), os.path.join(dev, "spec_kernel.h"), os.path.join(dev, "layout.h")))
    flags = ("-fsanitize=undefined", "-fno-sanitize=shift,signed-integer-overflow", "-fno-sanitize-recover=undefined", "-g") \
        if os.environ.get("ZPQ_EMU_SANITIZE") == "1" else ()
    key = hashlib.sha1(src.encode() + deps + " ".join(flags).encode()).hexdigest()[:20]
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, f"pcomp_{key}")
    if os.path.exists(exe):
        return exe
    gen = os.path.join(BUILD, f"pgen_{key}.{os.getpid()}.cpp")
    tmp = f"{exe}.{os.getpid()}.tmp"
    with open(gen, "w") as fh:
        fh.write('#include "wave_emu.h"\n' + src)
    cmd = ["g++", "-O1", "-std=c++17", "-w", *flags, "-I", EMU, "-I", dev, "-I", os.path.join(ROOT, "include"), gen,
           os.path.join(EMU, "pcomp_emu_main.cpp"), os.path.join(EMU, "wave_emu.cpp"), "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    os.remove(gen)
    if r.returncode != 0:
        raise RuntimeError("pcomp emulator build failed:\n" + r.stdout[-6000:])
    os.replace(tmp, exe)
    return exe


def launch(exe: str, ph: int, pm: int, streams: Sequence[bytes], caps: Sequence[int], timeout: float = 240):
    """One launch: [(result[0], status, the min(result[0], cap) bytes the lane left in its buffer)] per stream."""
    with tempfile.TemporaryDirectory() as td:
        spec, inp, outp = (os.path.join(td, n) for n in ("spec", "in", "out"))
        with open(spec, "w") as fh:
            fh.write("".join("%d %d\n" % (len(s), c) for s, c in zip(streams, caps)))
        with open(inp, "wb") as fh:
            fh.write(b"".join(bytes(s) for s in streams))
        r = subprocess.run([exe, "run", str(ph), str(pm), spec, inp, outp], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
        if r.returncode != 0:
            raise RuntimeError(f"pcomp emulator failed ({r.returncode}):\n" + r.stdout[-4000:])
        blob = open(outp, "rb").read()
    lines = r.stdout.splitlines()
    res, at = [], 0
    for k, c in enumerate(caps):
        w = lines[k].split()
        assert w[0] == "stream" and int(w[1]) == k, r.stdout[:400]
        n, status = int(w[3]), int(w[5])
        kept = min(n, c)
        res.append((n, status, blob[at:at + kept]))
        at += kept
    assert at == len(blob)
    return res


def engine_cap(hint: int, in_len: int) -> int:
    return (hint if hint else 8 * in_len) + 65536


def run(code: bytes, ph: int, pm: int, streams: Sequence[bytes], hints: Optional[Sequence[int]] = None, exe: Optional[str] = None):
    """The batch as engine_pcomp runs it: capacities from the hints, one launch, and a second one with the reported sizes when an
    output went beyond its capacity.  Returns (None when a lane reported a status or a capacity lies beyond the kernel's range --
    the engine hands the batch back -- else the outputs, the statuses of the last launch, the streams whose first capacity
    was too small)."""
    exe = build(code, ph, pm) if exe is None else exe
    hints = [0] * len(streams) if hints is None else hints
    caps = [engine_cap(h, len(s)) for h, s in zip(hints, streams)]
    if any(c > 0xFFFFFFF0 for c in caps):
        return None, [], []
    first = launch(exe, ph, pm, streams, caps)
    status = [st for _, st, _ in first]
    if any(status):
        return None, status, []
    retried = [k for k, (n, _, _) in enumerate(first) if n > caps[k]]
    for k, (n, _, kept) in enumerate(first):
        assert len(kept) == min(n, caps[k])
    if not retried:
        return [o for _, _, o in first], status, retried
    caps2 = [max(c, n) for c, (n, _, _) in zip(caps, first)]
    second = launch(exe, ph, pm, streams, caps2)
    assert [n for n, _, _ in second] == [n for n, _, _ in first], "the second attempt reports other sizes"
    assert all(n <= c for (n, _, _), c in zip(second, caps2))
    return [o for _, _, o in second], [st for _, st, _ in second], retried
