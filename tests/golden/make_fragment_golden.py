#!/usr/bin/env python3
"""Writes tests/golden/fragment_ref.json: what the reference archiver makes of five of the inputs of tests/fragment_cases.py.

    python tests/golden/make_fragment_golden.py [--check]

Needs the built reference (oracle/_ref/zpaq_ref_cli and libzpaq_ref.so, which __graft_entry__.build() makes where the
reference's sources are present).  Per input the archiver runs twice on a new archive holding the one file:

  add -method 0 -fragment N    the archive's h blocks list (sha1, size) of every new fragment in order: the cuts and the hashes;
  add -method 50 -fragment N   add prints, per block, the method it hands to the compressor, "50,R,T": R = the block's redundancy
                               estimate, T = its text / x86 flags, both sums over the per-fragment analysis.

Both are recorded results.  derive() is what tests/test_fragment_host.py calls to compare a fresh run with the fixture."""
from __future__ import annotations

import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLI = os.path.join(ROOT, "oracle", "_ref", "zpaq_ref_cli")
OUT = os.path.join(HERE, "fragment_ref.json")


def available() -> bool:
    from oracle.oracle_py import have_ref
    return os.path.exists(CLI) and have_ref()


def _add(td, name, data, method, fragment):
    src = os.path.join(td, name)
    with open(src, "wb") as fh:
        fh.write(data)
    arch = os.path.join(td, f"{name}_{method}.zpaq")
    r = subprocess.run([CLI, "add", arch, src, "-method", str(method), "-fragment", str(fragment)], cwd=td,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    return open(arch, "rb").read(), r.stdout


def _h_entries(archive: bytes):
    """(sha1 hex, size) of every fragment the archive's h blocks list, in order."""
    from oracle.oracle_py import TAG, Ref, parse_block
    ref = Ref()
    starts = [m.start() for m in re.finditer(re.escape(TAG), archive)]
    out = []
    for a, b in zip(starts, starts[1:] + [len(archive)]):
        name = parse_block(archive, a)["filename"]
        if not re.fullmatch(rb"jDC\d{14}h\d{10}", name):
            continue
        body = ref.decompress(archive[a:b], 1 << 24)
        assert (len(body) - 4) % 24 == 0
        for k in range(4, len(body), 24):
            out.append([body[k:k + 20].hex(), int.from_bytes(body[k + 20:k + 24], "little")])
    return out


def derive():
    """The fixture's content from a fresh run of the reference."""
    import fragment_cases as fc
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for name, fragment, data in fc.golden_inputs():
            arch, _ = _add(td, name, data, 0, fragment)
            frags = _h_entries(arch)
            assert sum(s for _, s in frags) <= len(data)        # (a fragment seen before is stored and listed once)
            _, said = _add(td, name, data, 50, fragment)
            methods = re.findall(r"\[\d+\.\.\d+\] \d+ -method (\S+)", said)
            assert methods, said
            res[name] = {"fragment": fragment, "bytes": len(data), "fragments": frags, "method50": methods}
    return res


def main():
    if not available():
        sys.exit("the reference binaries are not built (oracle/_ref)")
    got = derive()
    if "--check" in sys.argv:
        want = json.load(open(OUT))
        sys.exit(0 if got == want else "the fixture differs from a fresh run")
    with open(OUT, "w") as fh:
        json.dump(got, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
