"""-m gpu: small k (k <= 13) from the table of counters to a database on libkmc_hip.so — the cases of tests/test_smallk_db_emulated.py (tests/smallk_db_cases.py), and
what the emulation is too slow for: k = 11 and k = 13 at every legal prefix length, the recorded runs of `kmc` at k = 12 and k = 13."""
import numpy as np
import pytest

import smallk_db_cases as K
from kmc_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    capi.require_gpu_backend()
    c = K.SkContext(capi.lib_path())
    yield c
    c.close()


@pytest.mark.parametrize("k", [1, 2, 4, 5, 6, 8])
@pytest.mark.parametrize("ipt", [1, None])
def test_planted_tables_against_the_restatement(lib, k, ipt, monkeypatch):
    K.with_ipt(monkeypatch, ipt)
    for fill in K.FILLS:
        cs = 1 + (K.FILLS.index(fill) + k) % 4
        K.check_planted(lib, k, fill, cs, data_sizes=range(cs, 5) if fill in ("drawn", "half") else None)


@pytest.mark.parametrize("cs", [1, 2, 3, 4])
def test_every_counter_size_on_the_drawn_counters(lib, cs, monkeypatch):
    K.with_ipt(monkeypatch, 1)
    K.check_planted(lib, 6, "drawn", cs, data_sizes=range(cs, 5))


@pytest.mark.parametrize("fill,cs", [("drawn", 4), ("seam_end", 2), ("sparse64", 1), ("all_kept", 3)])
def test_k9_at_every_prefix_length(lib, fill, cs, monkeypatch):
    K.with_ipt(monkeypatch, None)
    K.check_planted(lib, 9, fill, cs)


@pytest.mark.parametrize("wgs", [1, 3])
def test_a_tally_workgroup_walks_many_tiles(lib, wgs, monkeypatch):
    """16 tiles of 256 entries under 1 and 3 workgroups: an even and an odd number of tiles per workgroup, and workgroups with different numbers of them"""
    K.with_ipt(monkeypatch, 1)
    monkeypatch.setenv("KMC_HIP_SMALLK_TALLY_WGS", str(wgs))
    K.check_planted(lib, 6, "drawn", 3)
    K.check_planted(lib, 6, "seam_end", 1)


def test_k9_one_entry_per_thread(lib, monkeypatch):
    K.with_ipt(monkeypatch, 1)
    K.check_planted(lib, 9, "half", 3, prefixes=[5], data_sizes=[3])


@pytest.mark.parametrize("ipt,offset", [(1, 0), (3, 0), (None, 0), (None, 8), (2, 8), (5, 0), (99, 0)])
def test_the_bytes_do_not_depend_on_the_tile(lib, ipt, offset, monkeypatch):
    K.with_ipt(monkeypatch, ipt)
    K.check_planted(lib, 6, "drawn", 2, offset=offset)
    K.check_planted(lib, 6, "seam_start", 1, offset=offset)


def test_k11_at_every_prefix_length(lib, monkeypatch):
    """p = 3, 7, 11: spans of 65 536 entries, 256 entries and 1"""
    K.with_ipt(monkeypatch, None)
    assert K.legal_prefixes(11) == [3, 7, 11]
    K.check_planted(lib, 11, "drawn", 4)
    K.check_planted(lib, 11, "half", 2, data_sizes=[2, 4])


def test_k13_sparse_at_every_prefix_length(lib, monkeypatch):
    """the one table of the workload's own size (512 MB, planted on the device): 1 entry in 16 non-zero, p = 1, 5, 9, 13 — spans of 16 M entries down to 1"""
    K.with_ipt(monkeypatch, None)
    k, (ci, cx, cm) = 13, K.PARAMS[2]
    assert K.legal_prefixes(k) == [1, 5, 9, 13]
    rng = np.random.default_rng(13)
    table = np.zeros(1 << 26, dtype=np.uint64)
    at = rng.integers(0, 1 << 26, size=1 << 22)
    table[at] = K.drawn_values(ci, cx, cm)[rng.integers(0, 9, size=at.size)]
    table[(1 << 26) - 1] = ci  # the last entry is kept
    dev = K.Planted(lib, table)
    try:
        for p in K.legal_prefixes(k):
            K.check_view(lib, dev.d, table, k, ci, cx, cm, p)
        K.check_view(lib, dev.d, table, k, ci, cx, cm, framing=1, data_size=3)
    finally:
        dev.free()


@pytest.mark.parametrize("name", K.OPEN_IDS)
def test_the_open_table(lib, name, monkeypatch):
    K.with_ipt(monkeypatch, None)
    K.check_open_table(lib, name)


@pytest.mark.parametrize("name", K.CASE_IDS)
def test_count_small_writes_what_kmc_wrote(lib, name, tmp_path, monkeypatch):
    K.with_ipt(monkeypatch, None)
    K.check_golden(lib, name, tmp_path)


def test_going_on_on_the_device(lib, tmp_path, monkeypatch):
    K.with_ipt(monkeypatch, None)
    K.check_going_on(lib, tmp_path)


def test_refusals(lib, monkeypatch):
    K.with_ipt(monkeypatch, None)
    K.check_refusals(lib)
