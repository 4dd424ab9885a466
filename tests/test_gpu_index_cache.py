"""GPU: PINTRON_INDEX_CACHE through the est-fact binary on test-AMBN (tests/golden/ambn): a cold run writes the index
file, a warm run loads it and leaves it alone, a damaged file is noticed, rebuilt and replaced, and two processes that
miss the cache together leave one whole file.  The outputs are the committed expected files every time.

The three damaged files hold zeros or the valid tables of another sequence of the same length: even a loader that
accepted them would hand the kernels nothing out of range, so a case can fail and cannot do more than fail.
Every child runs under a time limit and a non-zero exit ends the test before anything else is started."""
import filecmp
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import index_file_lib as IF

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "ambn")
EXE = os.path.join(ROOT, "pintron_amd", "bin", "est-fact")
FILES = ["raw-multifasta-out.txt", "processed-ests.txt", "megs.txt", "processed-megs.txt", "meg-edges.txt"]


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(EXE)
    return EXE


def _run(exe, work, cache):
    """one est-fact run on test-AMBN in the fresh directory `work`; the outputs must be the golden ones"""
    os.makedirs(work)
    for f in ("genomic.txt", "ests.txt"):
        shutil.copy(os.path.join(GOLD, f), work)
    subprocess.run([exe], cwd=work, env=dict(os.environ, PINTRON_INDEX_CACHE=str(cache)), check=True, timeout=120)
    for f in FILES:
        assert filecmp.cmp(os.path.join(work, f), os.path.join(GOLD, "expected-" + f), shallow=False), f


@pytest.fixture(scope="module")
def prepared():
    """the genomic sequence as the index sees it (shared, not to be modified)"""
    import meg_lib as M
    _, genomic = M.first_attempt_megs(open(os.path.join(GOLD, "genomic.txt")).read(),
                                      open(os.path.join(GOLD, "ests.txt")).read())
    assert len(genomic) > 1000
    return genomic


@pytest.fixture(scope="module")
def cold(exe, tmp_path_factory):
    """the cold run, once: (cache directory, file name, the file's bytes)"""
    top = tmp_path_factory.mktemp("index_cache_cold")
    cache = top / "cache"
    cache.mkdir()
    _run(exe, top / "run", cache)
    names = os.listdir(cache)
    assert len(names) == 1, names
    return cache, names[0], (cache / names[0]).read_bytes()


def test_cold_run_writes_the_index_of_the_prepared_sequence(cold, prepared):
    cache, name, _ = cold
    m = re.fullmatch(r"pintron-index-([0-9a-f]{16})-(\d+)\.bin", name)
    assert m, name
    header, arrays = IF.parse(str(cache / name))
    assert int(m.group(1), 16) == header["hash"] == IF.fnv1a64(prepared)
    assert int(m.group(2)) == header["len"] == len(prepared)
    assert (header["version"], header["ktab"]) == (IF.VERSION, IF.KTAB)
    assert header["payload_hash"] == IF.payload_hash(arrays)
    sa, lcp = IF.expected_sa_lcp(prepared)
    assert np.array_equal(arrays["sa"], sa) and np.array_equal(arrays["lcp"], lcp)
    IF.check_kmer_table(arrays["klo"], arrays["khi"], IF.expected_kmer_table(prepared, sa), "test-AMBN")
    assert not [f for f in os.listdir(cache) if ".tmp." in f]


def _seeded_cache(tmp_path, name, data):
    cache = tmp_path / "cache"
    cache.mkdir()
    (cache / name).write_bytes(data)
    return cache, cache / name


def test_warm_run_loads_the_file_and_leaves_it_alone(exe, cold, tmp_path):
    _, name, pristine = cold
    cache, path = _seeded_cache(tmp_path, name, pristine)
    before = os.stat(path)
    _run(exe, tmp_path / "run", cache)
    after = os.stat(path)
    assert (after.st_ino, after.st_mtime_ns) == (before.st_ino, before.st_mtime_ns)
    assert path.read_bytes() == pristine and os.listdir(cache) == [name]


def _index_of_another_sequence(prepared, pristine):
    """the good file of a sequence of the same length that differs in one base (CPU oracle: every entry below n)"""
    other = bytearray(prepared)
    at = len(other) // 2
    other[at] = ord("A") if other[at] != ord("A") else ord("C")
    header, arrays = IF.expected_file(bytes(other))
    data = IF.to_bytes(header, arrays)
    assert len(data) == len(pristine) and data != pristine and max(int(arrays[t].max()) for t in IF.TABLES) <= len(other)
    return data


@pytest.mark.parametrize("damage", ["emptied", "header-and-half-the-payload", "another-sequence"])
def test_damaged_cache_file_is_rebuilt_and_replaced(exe, cold, prepared, tmp_path, damage):
    _, name, pristine = cold
    data = {"emptied": lambda: b"", "header-and-half-the-payload": lambda: pristine[:40 + (len(pristine) - 40) // 2],
            "another-sequence": lambda: _index_of_another_sequence(prepared, pristine)}[damage]()
    cache, path = _seeded_cache(tmp_path, name, data)
    before = os.stat(path)
    _run(exe, tmp_path / "run", cache)
    after = os.stat(path)
    assert (after.st_ino, after.st_mtime_ns) != (before.st_ino, before.st_mtime_ns)
    assert path.read_bytes() == pristine and os.listdir(cache) == [name]


def test_two_processes_on_a_cold_cache(exe, cold, tmp_path):
    _, name, pristine = cold
    cache = tmp_path / "cache"
    cache.mkdir()
    with ThreadPoolExecutor(2) as pool:
        runs = [pool.submit(_run, exe, tmp_path / ("run%d" % k), cache) for k in range(2)]
        for r in runs:
            r.result()                         # a failed child or wrong outputs: raised here
    assert os.listdir(cache) == [name]
    assert (cache / name).read_bytes() == pristine
