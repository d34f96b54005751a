"""The forward E8E9 filter on the device (device/e8e9_forward_kernel.h): the stage on its own (zpq_e8e9_device) against the host's
zpq_e8e9 over the blocks of e8e9_forward_cases, in one arena with guard bytes between them; the step cap's decline; and the route
through zpq_compress_blocks (ZPAQ_AMD_DEVICE_E8) in fresh child processes -- the batched hash parse, the batched suffix sort with
LZ77 and with the BWT behind it, and the wide sort of one block -- against the host's route, the reference, and the counters."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import e8e9_forward_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(HERE)
GUARD, GFILL = 64, 0xC3
UNSUPPORTED = 8
METHODS = ("x0,5,6,0,3,20", "x0,6,5,0,7,21,1", "x0,7")             # the hash parse; LZ77 through the suffix array; the BWT
WIDE_METHODS = ("x0,7", "x0,6,5,0,7,21,1")
KNOBS = ("ZPAQ_AMD_DEVICE_E8", "ZPAQ_AMD_E8_MAX_STEPS", "ZPAQ_AMD_DEVICE_SORT_WIDE", "ZPAQ_AMD_SORT_WIDE_FROM", "ZPAQ_AMD_DEVICE_PARSE",
         "ZPAQ_AMD_DEVICE_PARSE_WIDE", "ZPAQ_AMD_DEVICE_CODES")


# ---- the stage alone ----
def _stage(gpu, blocks, max_steps=0):
    rc, bufs, status = gpu.e8e9_device(blocks, max_steps, guard=GUARD, fill=GFILL)
    assert rc == 0, gpu.lib().zpq_last_error().decode()
    for k, (b, buf) in enumerate(zip(blocks, bufs)):
        assert buf[len(b):] == bytes([GFILL]) * GUARD, (k, len(b), "a store into the guard bytes")
    return [buf[:len(b)] for b, buf in zip(blocks, bufs)], status


def test_the_stage_filters_every_block_as_the_host_does(gpu):
    bl = fc.blocks()
    out, status = _stage(gpu, bl)
    assert status == [0] * len(bl)
    for k, (b, o) in enumerate(zip(bl, out)):
        assert o == gpu.e8e9(b), (k, len(b))


def test_the_stage_one_block_at_a_time(gpu):
    for k, b in enumerate(fc.blocks()):
        if len(b) > 20000:
            continue
        out, status = _stage(gpu, [b])
        assert status == [0] and out[0] == gpu.e8e9(b), (k, len(b))


def test_the_step_cap_declines_and_leaves_the_buffer_alone(gpu):
    bl = [b for b in fc.blocks() if len(b) < (1 << 20)]
    at = bl.index(fc.WORST)
    out, status = _stage(gpu, bl, max_steps=1000)
    assert status == [int(k == at) for k in range(len(bl))]
    assert out[at] == fc.WORST                                      # untouched
    for k, (b, o) in enumerate(zip(bl, out)):
        assert k == at or o == gpu.e8e9(b), (k, len(b))


def test_the_skipping_block_completes_at_the_default_cap(gpu):
    b = fc.skipping_block()
    assert len(b) == 1 << 20 and gpu.e8e9(b) != b
    out, status = _stage(gpu, [b])
    assert status == [0] and out[0] == gpu.e8e9(b)


def test_the_empty_batch_and_the_range(gpu):
    rc, bufs, status = gpu.e8e9_device([])
    assert rc == 0 and bufs == [] and status == []
    rc, bufs, status = gpu.e8e9_device([b""] * 65536)
    assert rc == UNSUPPORTED and b"range" in gpu.lib().zpq_last_error()


# ---- through zpq_compress_blocks, in fresh child processes ----
CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import zpaq_amd as z
spec = json.loads(open(sys.argv[2]).read())
z.init(0)
blocks = [np.fromfile(p, np.uint8) for p in spec["blocks"]]
out = {}
for run in spec["runs"]:
    use = [blocks[i].copy() for i in run["blocks"]]
    after = []
    arch = z.compress_blocks(use, run["method"], inputs_after=after)
    out[run["name"]] = {"e8": z.last_device_e8_blocks(), "wide": z.last_wide_sort_blocks(), "hash": z.last_hash_parse_blocks()}
    for k, (a, b) in enumerate(zip(arch, after)):
        open(os.path.join(spec["dir"], run["name"] + ".arch." + str(k)), "wb").write(bytes(a))
        open(os.path.join(spec["dir"], run["name"] + ".buf." + str(k)), "wb").write(bytes(b))
z.shutdown()
print("RESULT " + json.dumps(out))
"""


def _child(tmp, tag, block_paths, runs, env_extra):
    """One fresh process with its environment: (counters per run, archives per run, the caller's buffers afterwards per run)."""
    d = tmp / tag
    d.mkdir()
    spec = d / "spec.json"
    spec.write_text(json.dumps({"dir": str(d), "blocks": [str(p) for p in block_paths], "runs": runs}))
    env = dict(os.environ)
    for k in KNOBS:
        env.pop(k, None)
    env.update(env_extra)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", CHILD, ROOT, str(spec)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=240)
    assert r.returncode == 0, (tag, r.stdout[-3000:])
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    arch = {run["name"]: [(d / f"{run['name']}.arch.{k}").read_bytes() for k in range(len(run["blocks"]))] for run in runs}
    bufs = {run["name"]: [(d / f"{run['name']}.buf.{k}").read_bytes() for k in range(len(run["blocks"]))] for run in runs}
    return got, arch, bufs


def _write(tmp, blocks):
    paths = []
    for i, b in enumerate(blocks):
        p = tmp / f"block{i}"
        p.write_bytes(b)
        paths.append(p)
    return paths


@pytest.fixture(scope="module")
def batch_blocks():
    """8 blocks of x86-like bytes -- enough for the batched routes' thresholds -- and the worst case."""
    return [fc.x86_like(160 * 1024, seed) for seed in range(8)] + [fc.WORST]


@pytest.fixture(scope="module")
def batch_runs(gpu, batch_blocks, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("e8_batch")
    paths = _write(tmp, batch_blocks)
    runs = [{"name": f"m{k}", "method": m, "blocks": list(range(len(paths)))} for k, m in enumerate(METHODS)]
    return {"on": _child(tmp, "on", paths, runs, {"ZPAQ_AMD_DEVICE_E8": "1"}),
            "off": _child(tmp, "off", paths, runs, {"ZPAQ_AMD_DEVICE_E8": "0"}),
            "unset": _child(tmp, "unset", paths, runs, {}),
            "capped": _child(tmp, "capped", paths, runs, {"ZPAQ_AMD_DEVICE_E8": "1", "ZPAQ_AMD_E8_MAX_STEPS": "1000"})}


@pytest.mark.parametrize("k", range(len(METHODS)))
def test_the_batched_routes_filter_there(gpu, batch_blocks, batch_runs, k):
    name, nb = f"m{k}", len(batch_blocks)
    want = [gpu.e8e9(b) for b in batch_blocks]
    assert want[-1] != batch_blocks[-1] and want[0] != batch_blocks[0]
    for env, (got, arch, bufs) in batch_runs.items():
        assert bufs[name] == want, (METHODS[k], env, "the caller's buffers are not what zpq_e8e9 leaves")
        assert arch[name] == batch_runs["off"][1][name], (METHODS[k], env, "the archives differ from the host route's")
        if k == 0:
            assert got[name]["hash"] == nb, (METHODS[k], env, "the batch did not take the device's hash parse")
    assert batch_runs["on"][0][name]["e8"] == nb, METHODS[k]
    assert batch_runs["off"][0][name]["e8"] == 0, METHODS[k]
    assert batch_runs["capped"][0][name]["e8"] == nb - 1, (METHODS[k], "the worst case's walk does not fit 1 000 steps: the host filters it")
    assert batch_runs["unset"][0][name]["e8"] in (0, nb), (METHODS[k], "unset: e8_forward_pays decides for the whole batch")


@pytest.mark.parametrize("k", range(len(METHODS)))
def test_the_batched_routes_against_the_reference(ref, batch_blocks, batch_runs, k):
    want = [ref.compress_block(b, METHODS[k]) for b in batch_blocks]
    for env, (_, arch, _) in batch_runs.items():
        assert arch[f"m{k}"] == want, (METHODS[k], env)


@pytest.fixture(scope="module")
def wide_blocks():
    """200 KiB of x86-like bytes; the worst case padded to 200 KiB with them."""
    n = 200 * 1024
    return [fc.x86_like(n, 21), fc.WORST + fc.x86_like(n - len(fc.WORST), 22)]


@pytest.fixture(scope="module")
def wide_runs(gpu, wide_blocks, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("e8_wide")
    paths = _write(tmp, wide_blocks)
    env = {"ZPAQ_AMD_DEVICE_SORT_WIDE": "1", "ZPAQ_AMD_SORT_WIDE_FROM": "65536", "ZPAQ_AMD_DEVICE_PARSE_WIDE": "1"}
    runs = [{"name": f"w{k}b{i}", "method": m, "blocks": [i]} for k, m in enumerate(WIDE_METHODS) for i in range(2)]
    return {"on": _child(tmp, "on", paths, runs, dict(env, ZPAQ_AMD_DEVICE_E8="1")),
            "off": _child(tmp, "off", paths, runs, dict(env, ZPAQ_AMD_DEVICE_E8="0")),
            "capped": _child(tmp, "capped", paths, runs, dict(env, ZPAQ_AMD_DEVICE_E8="1", ZPAQ_AMD_E8_MAX_STEPS="1000"))}


@pytest.mark.parametrize("k", range(len(WIDE_METHODS)))
def test_the_wide_route_filters_there(gpu, wide_blocks, wide_runs, k):
    for i, b in enumerate(wide_blocks):
        name = f"w{k}b{i}"
        for env, (got, arch, bufs) in wide_runs.items():
            assert got[name]["wide"] == 1, (WIDE_METHODS[k], i, env, "the block did not take the wide route")
            assert bufs[name] == [gpu.e8e9(b)], (WIDE_METHODS[k], i, env)
            assert arch[name] == wide_runs["off"][1][name], (WIDE_METHODS[k], i, env)
        assert wide_runs["on"][0][name]["e8"] == 1 and wide_runs["off"][0][name]["e8"] == 0, (WIDE_METHODS[k], i)
    assert wide_runs["capped"][0][f"w{k}b0"]["e8"] == 1
    assert wide_runs["capped"][0][f"w{k}b1"]["e8"] == 0, (WIDE_METHODS[k], "the worst case's walk does not fit 1 000 steps")


@pytest.mark.parametrize("k", range(len(WIDE_METHODS)))
def test_the_wide_route_against_the_reference(ref, wide_blocks, wide_runs, k):
    for i, b in enumerate(wide_blocks):
        want = [ref.compress_block(b, WIDE_METHODS[k])]
        for env, (_, arch, _) in wide_runs.items():
            assert arch[f"w{k}b{i}"] == want, (WIDE_METHODS[k], i, env)


def test_methods_without_e8e9_are_left_alone(gpu, batch_blocks, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("e8_none")
    paths = _write(tmp, batch_blocks)
    runs = [{"name": f"n{k}", "method": m, "blocks": list(range(len(paths)))} for k, m in enumerate(("x0,1,4,0,3,20", "x0,3"))]
    got, _, bufs = _child(tmp, "on", paths, runs, {"ZPAQ_AMD_DEVICE_E8": "1"})
    for run in runs:
        assert got[run["name"]]["e8"] == 0, run["method"]
        assert bufs[run["name"]] == batch_blocks, (run["method"], "the inputs were touched")
