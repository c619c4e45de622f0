"""-m gpu: small k (k <= 13) counted on the device. The per-part cases of tests/test_stage1_smallk_emulated.py on libkmc_hip.so (k_s1_smallk_count on
gfx950; parts of 4-5 tiles, where every seam, halo and table placement exists), one 8 MB part of the large-part kind of the -hc / estimate tests at k = 13
and k = 6, then kmc_hip_s1 against the reference's kmc: database bytes, statistics lines, the worker's report line."""
import os
import subprocess
import threading

import numpy as np
import pytest

from kmc_amd import build as B
from kmc_amd import capi, synth
from smallk_cases import (E2E_IDS, E2E_SETS, EINVAL, UNCOVERED, SmallKLib, check_e2e, check_part, format_cases, run_kmc, seam_text, smallk_nonzero, smallk_table)
from test_stage1_emulated import _records_text
from test_stage1_hc_emulated import _rnd, getseq_returns
from test_stage1_multiline_emulated import _wrap

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    L = SmallKLib(os.environ.get("KMC_HIP_LIB") or B.LIB_HIP)
    yield L
    L.close()


def test_the_library_says_it_counts_small_k_and_keeps_its_contract(lib):
    L = lib.L
    assert L.kmc_hip_abi_version() == 4
    assert L.kmc_hip_split_covers(capi.SPLIT_COVERS_SMALLK) == 1 and [L.kmc_hip_split_covers(t) for t in (0x101, 0x104)] == [0, 0]
    lib.close_table()
    text = b">t\nACGTACGTTGCATGCATTGACCAGTAGGATCCAGT\n"
    assert lib.part(text, 5, True, 0, 1 << 17)[0] == EINVAL  # none open
    assert lib.open(0, True) == EINVAL and lib.open(14, True) == EINVAL
    assert lib.open(5, True) == 0 and lib.open(5, True) == 0 and lib.open(5, False) == EINVAL and lib.open(6, True) == EINVAL
    for bad in (dict(flags=4), dict(file_type=3), dict(k=14), dict(k=6)):
        kw = dict(dict(k=5, both=True, file_type=0, line_cap=1 << 17, flags=0), **bad)
        assert lib.part(text, kw["k"], kw["both"], kw["file_type"], kw["line_cap"], 0, kw["flags"])[0] == EINVAL, bad
    assert lib.part(b">a\nACGTACG\n\n>b\nACGTACGT\n", 5, True, 0, 1 << 17)[0] == UNCOVERED
    assert not lib.read_all(5).any()
    lib.close_table()


@pytest.mark.parametrize("k", list(range(1, 14)))
def test_windows_across_every_seam_for_every_k(lib, k):
    for both in (True, False):
        for fmt, eol in (("fq", b"\n"), ("fq", b"\r\n"), ("fa", b"\n"), ("fa", b"\r\n")):
            returns = check_part(lib, seam_text(k, fmt, eol), 1 if fmt == "fq" else 0, k, both, 1 << 17)
            lens = [q.size for q in returns]
            assert k - 1 in lens and k in lens and 9000 in lens


@pytest.mark.parametrize("k", [5, 11])
def test_formats_part_kinds_and_homopolymer_compression(lib, k):
    for name, text, ft, line_cap, long_read, returns, n_reads in format_cases(k):
        for hc, both in ((False, True), (True, True), (True, False), (False, False)):
            check_part(lib, text, ft, k, both, line_cap, long_read, hc, returns, n_reads)


@pytest.mark.parametrize("k", [3, 6, 7, 8, 13])
def test_same_address_adds_on_both_sides_of_the_table_placement(lib, k, monkeypatch):
    """a 9 000-symbol homopolymer; with two workgroups only, every workgroup walks several tiles before it flushes its LDS table (k <= 7)"""
    text = b">poly\n" + b"C" * 9000 + b"\n>other\n" + _rnd(np.random.default_rng(4), 9000) + b"\n>again\n" + b"ACAC" * 1200 + b"\n"
    check_part(lib, text, 0, k, True, 1 << 17)
    monkeypatch.setenv("KMC_HIP_S1_SMALLK_WGS", "2")
    check_part(lib, text, 0, k, False, 1 << 17)
    monkeypatch.setenv("KMC_HIP_S1_SMALLK_LDS_K", "0")  # the global path at a k that has the LDS path
    check_part(lib, text, 0, k, True, 1 << 17)


def test_accumulation_over_calls_slots_and_threads(lib):
    k, both = 9, True
    rng = np.random.default_rng(11)
    texts = [_records_text("fq", b"\n", [_rnd(rng, int(n)) for n in rng.integers(20, 300, size=40)] + [b"A" * 400]) for _ in range(4)]
    each = [smallk_table(getseq_returns(t, 1, k, 1 << 17)[0], k, both)[0] for t in texts]
    lib.reopen(k, both)
    for t in texts[:2]:
        assert lib.part(t, k, both, 1, 1 << 17)[0] == 0
    rcs = {}

    def work(slot, t):
        rcs[slot] = lib.part(t, k, both, 1, 1 << 17, slot=slot)[0]

    th = [threading.Thread(target=work, args=(1 + i, texts[2 + i])) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert rcs == {1: 0, 2: 0}
    want = each[0] + each[1] + each[2] + each[3]
    assert np.array_equal(lib.read_all(k), want) and np.array_equal(lib.read_all(k), want)
    assert np.array_equal(np.concatenate([lib.read(f, min(5000, want.size - f)) for f in range(0, want.size, 5000)]), want)
    lib.close_table()


@pytest.mark.parametrize("k", [13, 6])
def test_large_part_on_the_device(lib, k):
    """one 8 MB part (~2 000 tiles, more than the 1 024 persistent workgroups): homopolymer-rich records, one of 2.5 Mbp beyond a 1 MB line cap, a run of 20 000"""
    rng = np.random.default_rng(17)
    recs = []
    for i in range(45):
        n = 2_500_000 if i == 7 else int(rng.integers(1000, 250_000))
        recs.append(synth.homopolymer_rich_sequence(rng, n, 2.0, 0.2, 30, 40).tobytes())
        if i == 20:
            recs.append(b"G" * 20_000)
    text = b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(recs))
    assert 7_000_000 < len(text) < 10_000_000
    lib.reopen(k, True)
    rc, n_reads, n_kmers = lib.part(text, k, True, 0, 1 << 20)
    assert rc == 0
    ent, cnt = lib.read_nonzero(k)
    lib.close_table()
    returns, w_reads = getseq_returns(text, 0, k, 1 << 20)
    w_ent, w_cnt, total = smallk_nonzero(returns, k, True)
    assert (n_reads, n_kmers) == (w_reads, total) and np.array_equal(ent, w_ent) and np.array_equal(cnt, w_cnt)


# ---- kmc_hip_s1 against kmc
def _exe(name):
    return os.path.join(ROOT, "kmc_amd", "bin", name) if name.startswith("kmc_hip") else os.path.join(ROOT, "oracle", "_ref", name)


def _require_binaries():
    missing = [n for n in ("kmc", "kmc_hip_s1") if not os.path.exists(_exe(n))]
    if missing:
        pytest.skip("needs the reference pipeline binaries (%s not built: the reference source tree was absent at build time)" % ", ".join(missing))


_state = {"broken": False}  # one failed or hung run is enough: the other parameter sets do not spend GPU time on the same problem
_IN = {}


def _reads(tmp_path_factory, fmt):
    """~5 Mbp, as the estimate test's generator makes them: the 3.4 Mbp record arrives as long-read parts under -m2"""
    if fmt not in _IN:
        p = str(tmp_path_factory.mktemp("smallk") / ("reads." + fmt))
        if fmt == "ml":
            rng = np.random.default_rng(5)
            with open(p, "wb") as f:
                for i, n in enumerate([900_000, 0, 3_400_000, 20_000, 600_000]):
                    f.write(b">ctg%d\n" % i + _wrap(synth.homopolymer_rich_sequence(rng, n, 2.0, 0.2, 30, 40).tobytes(), 60, b"\n"))
        else:
            synth.make_long_reads(p, 4, [200, 600_000, 150, 3_400_000, 90, 530_000, 40_000], fmt=fmt, mean_run=2.0, lower_frac=0.2, n_run_per_mbp=30, n_run_len=40)
        _IN[fmt] = p
    return _IN[fmt]


def _guarded(fn):
    if _state["broken"]:
        pytest.fail("an earlier run of kmc_hip_s1 with small k failed or hung")
    try:
        return fn()
    except (AssertionError, subprocess.TimeoutExpired):
        _state["broken"] = True
        raise


@pytest.mark.parametrize("flags,fmt", E2E_SETS, ids=E2E_IDS)
def test_kmc_hip_s1_small_k_writes_the_reference_database(flags, fmt, tmp_path, tmp_path_factory):
    _require_binaries()
    env = {"KMC_HIP_LIB": os.environ.get("KMC_HIP_LIB") or B.LIB_HIP}
    _guarded(lambda: check_e2e(_exe("kmc"), _exe("kmc_hip_s1"), flags, _reads(tmp_path_factory, fmt), tmp_path, env, timeout=300))


def test_kmc_hip_s1_counts_a_k10_database_at_k9(tmp_path, tmp_path_factory):
    """the reference's CI pair: a -k10 database fed to -k9 -fkmc"""
    _require_binaries()
    env = {"KMC_HIP_LIB": os.environ.get("KMC_HIP_LIB") or B.LIB_HIP}

    def both():
        rc, _, log = run_kmc(_exe("kmc"), ["-k10", "-ci1", "-m2", "-sf1", "-sp2", "-sr2"], _reads(tmp_path_factory, "fq"), tmp_path, "k10", timeout=300)
        assert rc == 0, log[-1500:]
        check_e2e(_exe("kmc"), _exe("kmc_hip_s1"), ["-k9", "-fkmc"], str(tmp_path / "db_k10"), tmp_path, env, timeout=300)

    _guarded(both)
