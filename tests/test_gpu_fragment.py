"""Files cut into fragments on the device (device/fragment_kernel.h, the stitch of device/fragment_stitch.hpp and one SHA-1 job
per fragment): every zpq_fragment_device result against zpq_fragment_host, field by field -- sizes, hits, SHA-1s and the order-1
tables --, with the piece size lowered so that small files have many pieces, the overflow convention, and the number of fix-up
rounds for data that re-joins and data that never does."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fragment_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host0(zlib_):
    """zpq_fragment_host of the ragged batch, once."""
    rc, got, total = zlib_.fragment_host([d for _, d in fc.files0()], 0, fc.BLOCKSIZE)
    assert rc == 0
    return got, total


def _same(got, want, names):
    assert len(got) == len(want)
    for name, g, w in zip(names, got, want):
        assert [x[0] for x in g] == [x[0] for x in w], (name, "sizes")
        assert [x[1] for x in g] == [x[1] for x in w], (name, "hits")
        assert [x[2] for x in g] == [x[2] for x in w], (name, "sha1")
        assert [x[3] for x in g] == [x[3] for x in w], (name, "o1")


@pytest.mark.parametrize("piece", ["16384", ""])
def test_the_ragged_batch_is_cut_as_the_host_cuts_it(gpu, monkeypatch, host0, piece):
    if piece:
        monkeypatch.setenv("ZPAQ_AMD_FRAG_PIECE", piece)
    else:
        monkeypatch.delenv("ZPAQ_AMD_FRAG_PIECE", raising=False)
    want, total = host0
    names = [k for k, _ in fc.files0()]
    rc, got, said = gpu.fragment_device([d for _, d in fc.files0()], 0, fc.BLOCKSIZE, cap=total)
    assert rc == 0, gpu.lib().zpq_last_error().decode()
    assert said == total
    _same(got, want, names)
    assert gpu.last_fragment_rounds() == (1 if piece else 0)          # 16 KiB: zeros has two pieces, the others re-join at once


def test_a_file_of_three_mebibytes_at_fragment_6(gpu, monkeypatch):
    monkeypatch.setenv("ZPAQ_AMD_FRAG_PIECE", str(1 << 20))
    data = fc.file6()
    rc, want, total = gpu.fragment_host([data], 6, fc.BLOCKSIZE)
    assert rc == 0 and total > 30
    rc, got, said = gpu.fragment_device([data], 6, fc.BLOCKSIZE, cap=total)
    assert rc == 0, gpu.lib().zpq_last_error().decode()
    _same(got, want, ["text6"])
    assert gpu.last_fragment_rounds() == 1


def test_three_hundred_small_files(gpu, monkeypatch):
    monkeypatch.delenv("ZPAQ_AMD_FRAG_PIECE", raising=False)
    rng = np.random.default_rng(3)
    kinds = ("text", "lcg", "zeros", "records", "pattern")
    files = [fc._kind(kinds[k % 5], int(rng.integers(0, 3001)), 100 + k) for k in range(300)]
    files[7] = b""
    rc, want, total = gpu.fragment_host(files, 0, fc.BLOCKSIZE)
    assert rc == 0 and total > 600
    rc, got, said = gpu.fragment_device(files, 0, fc.BLOCKSIZE, cap=total)
    assert rc == 0, gpu.lib().zpq_last_error().decode()
    _same(got, want, list(range(300)))
    assert len(got[7]) == 1 and got[7][0][0] == 0


def test_a_capacity_too_small_reports_the_count_and_writes_nothing(gpu, monkeypatch, host0):
    monkeypatch.setenv("ZPAQ_AMD_FRAG_PIECE", "16384")
    _, total = host0
    files = [d for _, d in fc.files0()]
    for cap in (0, total - 1):
        rc, untouched, said = gpu.fragment_device(files, 0, fc.BLOCKSIZE, cap=cap)
        assert rc == 3 and untouched is True and said == total, (cap, rc, said)


def test_zeros_never_rejoin_and_text_does_at_once(gpu, monkeypatch):
    """Zeros cut every 107 bytes and 4 096 is no multiple of it: a round per piece behind the first.  Text re-joins in the first."""
    monkeypatch.setenv("ZPAQ_AMD_FRAG_PIECE", "4096")
    f = dict(fc.files0())
    for name, rounds in (("zeros", 4), ("text", 1)):
        rc, want, total = gpu.fragment_host([f[name]], 0, fc.BLOCKSIZE)
        rc, got, _ = gpu.fragment_device([f[name]], 0, fc.BLOCKSIZE, cap=total)
        assert rc == 0, gpu.lib().zpq_last_error().decode()
        _same(got, want, [name])
        assert gpu.last_fragment_rounds() == rounds, name
        assert gpu.last_fragment_rounds() > (1 if name == "zeros" else 0)
