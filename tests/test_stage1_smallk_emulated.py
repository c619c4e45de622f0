"""CPU: small k (k <= 13) counted on the device — kmc_hip_smallk_open / _part / _read / _close (k_s1_smallk_count behind the front half of
kmc_amd/csrc/stage1_chain.h) in the PRODUCT'S host library compiled over the emulated HIP runtime (tests/emu.py build_hostlib), and kmc_hip_s1 over it.

The oracle is the numpy restatement of CSplitter::ProcessReadsSmallK in tests/smallk_cases.py, over the buffers the Python GetSeq restatements of the -hc
and -fm tests return. It is held to tables recorded from the reference itself (tests/golden/smallk_counts.json, written by tests/make_smallk_golden.py:
kmc_dump of `kmc -k5` and `kmc -k9 -b` databases of tests/golden/smallk_input.fa), so it is pinned to the reference and not to the code under test.
Tables are compared exactly: whole at k <= 9, the non-zero entries beyond. The -m gpu file runs the same cases on the device."""
import ctypes
import json
import os
import re
import threading

import numpy as np
import pytest

import emu
from kmc_amd import capi, synth
from smallk_cases import (E2E_IDS, E2E_SETS, EINVAL, REPORT, UNCOVERED, SmallKLib, check_e2e, check_part, codes_of, format_cases, run_kmc, seam_text,
                          smallk_kmers, smallk_nonzero, smallk_table)
from test_stage1_emulated import _parse_bin, _records_text, _sig_map
from test_stage1_hc_emulated import _rnd, getseq_returns, seam_reads
from test_stage1_multiline_emulated import _exe, _require, _wrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def hostlib():
    lib = SmallKLib(emu.build_hostlib("small"))
    yield lib
    lib.close()


# ---- 1: the restatement is the reference
def _kmer_int(s):
    v = 0
    for ch in s:
        v = v * 4 + "ACGT".index(ch)
    return v


@pytest.mark.parametrize("name,k,both", [("k5", 5, True), ("k9b", 9, False)])
def test_the_restatement_counts_what_the_reference_counts(name, k, both):
    with open(os.path.join(GOLDEN, "smallk_counts.json")) as f:
        gold = json.load(f)[name]
    with open(os.path.join(GOLDEN, "smallk_input.fa"), "rb") as f:
        text = f.read()
    returns, n_reads = getseq_returns(text, 0, k, 524296)
    assert n_reads == 69 and len(returns) == 69
    ent, cnt, total = smallk_nonzero(returns, k, both)
    assert len(gold) >= 500 and [_kmer_int(a) for a, _ in gold] == [int(x) for x in ent] and [c for _, c in gold] == [int(x) for x in cnt]
    assert total == sum(c for _, c in gold) and max(c for _, c in gold) >= 30  # the homopolymer


def test_the_restatement_follows_its_definition():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 4, size=300).astype(np.int8)
    for k in (1, 2, 5, 13):
        fwd = smallk_kmers(q, k, False)
        assert fwd.size == 300 - k + 1 and int(fwd[17]) == int("".join(str(int(x)) for x in q[17:17 + k]), 4)
        rc = (3 - q[::-1]).astype(np.int8)
        assert np.array_equal(smallk_kmers(rc, k, True)[::-1], smallk_kmers(q, k, True))  # canonical
        assert np.array_equal(smallk_kmers(q, k, True), np.minimum(fwd, smallk_kmers(rc, k, False)[::-1]))
    q2 = q.copy()
    q2[100] = -1
    assert smallk_kmers(q2, 13, True).size == 300 - 13 + 1 - 13 and smallk_kmers(q[:12], 13, True).size == 0


# ---- 2: contract
def test_the_library_says_it_counts_small_k_and_keeps_its_contract(hostlib):
    L, lib = hostlib.L, hostlib
    assert L.kmc_hip_abi_version() == 4
    assert L.kmc_hip_split_covers(capi.SPLIT_COVERS_SMALLK) == 1 and capi.SPLIT_COVERS_SMALLK == 0x103
    assert [L.kmc_hip_split_covers(t) for t in (0x100, 0x101, 0x102, 0x104, 0x200)] == [1, 0, 1, 0, 0]
    for sym in capi.SYMBOLS:
        assert hasattr(L, sym), sym
    assert {"kmc_hip_smallk_open", "kmc_hip_smallk_part", "kmc_hip_smallk_read", "kmc_hip_smallk_close"} <= set(capi.SYMBOLS)
    lib.close_table()
    lib.close_table()  # closing twice is fine
    for bad in (0, 14, 27):
        assert lib.open(bad, True) == EINVAL
    assert lib.open(5, True) == 0 and lib.open(5, True) == 0
    assert lib.open(5, False) == EINVAL and lib.open(6, True) == EINVAL
    assert L.kmc_hip_smallk_read(lib.h, 0, 1, 1 << 10, None) == EINVAL and lib.read(1 << 10, 0).size == 0
    lib.close_table()


def test_calls_that_add_nothing_leave_the_table_as_it_was(hostlib):
    lib, k = hostlib, 5
    rng = np.random.default_rng(12)
    text = _records_text("fa", b"\n", [_rnd(rng, 300) for _ in range(10)])
    lib.close_table()
    rc, _, _ = lib.part(text, k, True, 0, 1 << 17)
    assert rc == EINVAL and b"smallk_open" in lib.L.kmc_hip_last_error(lib.h)  # no table open
    lib.reopen(k, True)
    assert lib.part(text, k, True, 0, 1 << 17)[0] == 0
    want, _ = smallk_table(getseq_returns(text, 0, k, 1 << 17)[0], k, True)
    assert np.array_equal(lib.read_all(k), want)
    blank = b">a\n" + _rnd(rng, 200) + b"\n\n>b\n" + _rnd(rng, 200) + b"\n"
    assert lib.part(blank, k, True, 0, 1 << 17)[0] == UNCOVERED
    assert np.array_equal(lib.read_all(k), want)
    for bad in (dict(flags=4), dict(flags=2), dict(file_type=3), dict(k=14), dict(k=6), dict(both=False), dict(part_kind=2), dict(line_cap=100)):
        kw = dict(dict(k=k, both=True, file_type=0, line_cap=1 << 17, part_kind=0, flags=0), **bad)
        assert lib.part(text, kw["k"], kw["both"], kw["file_type"], kw["line_cap"], kw["part_kind"], kw["flags"])[0] == EINVAL, bad
        assert np.array_equal(lib.read_all(k), want), bad
    # signature_len, n_bins and max_x are ignored: values the bin path refuses
    assert lib.part(text, k, True, 0, 1 << 17, signature_len=9, n_bins=5000, max_x=7)[0] == 0
    assert np.array_equal(lib.read_all(k), 2 * want)
    lib.close_table()


def test_the_bin_path_is_the_same_before_and_after_a_small_k_session(hostlib):
    lib = hostlib
    lib.close_table()
    smap = _sig_map(9, 37, 5)
    big = _records_text("fq", b"\n", seam_reads(27))
    rc, before = lib.split(big, 27, 9, 37, smap, 1 << 17, 1, flags=0)
    assert rc == 0
    assert lib.open(7, True) == 0 and lib.part(big, 7, True, 1, 1 << 17)[0] == 0 and lib.read_all(7).any()
    rc, during = lib.split(big, 27, 9, 37, smap, 1 << 17, 1, flags=0)
    lib.close_table()
    rc2, after = lib.split(big, 27, 9, 37, smap, 1 << 17, 1, flags=0)
    assert rc == 0 and rc2 == 0
    for other in (during, after):
        assert all(a.size == b.size and _parse_bin(a, 27) == _parse_bin(b, 27) for a, b in zip(before["bins"], other["bins"]))
        assert all(np.array_equal(before[key], other[key]) for key in ("kmers", "supers", "plus_x")) and before["n_reads"] == other["n_reads"]


# ---- 3: seams, every k
@pytest.mark.parametrize("both", [True, False], ids=["both", "fwd"])
@pytest.mark.parametrize("k", list(range(1, 14)))
def test_windows_across_every_seam_for_every_k(hostlib, k, both):
    returns = check_part(hostlib, seam_text(k, "fq", b"\n"), 1, k, both, 1 << 17)
    lens = [q.size for q in returns]
    assert k - 1 in lens and k in lens and 9000 in lens and sum(x + 1 for x in lens) > 4 * 4096
    stream = np.concatenate([np.concatenate([q, np.array([-1], dtype=np.int8)]) for q in returns])
    assert stream[4 * 4096 + 3] < 0 and np.all(stream[4 * 4096 + 3 - 256:4 * 4096 + 3] >= 0)  # the invalid code inside the fourth tile's halo


@pytest.mark.parametrize("fmt,eol", [("fq", b"\r\n"), ("fa", b"\n"), ("fa", b"\r\n")], ids=["fq-crlf", "fa-lf", "fa-crlf"])
@pytest.mark.parametrize("k", [2, 7, 12])
def test_seams_in_the_other_formats(hostlib, k, fmt, eol):
    text = seam_text(k, fmt, eol)
    assert fmt != "fa" or text[-1:] not in (b"\n", b"\r")  # a window ends on the last code of the stream
    check_part(hostlib, text, 1 if fmt == "fq" else 0, k, k != 7, 1 << 17)


# ---- 4: formats and part kinds, with and without -hc
@pytest.mark.parametrize("hc", [False, True], ids=["plain", "hc"])
@pytest.mark.parametrize("k", [5, 11])
def test_formats_part_kinds_and_homopolymer_compression(hostlib, k, hc):
    names = []
    for name, text, ft, line_cap, long_read, returns, n_reads in format_cases(k):
        got = check_part(hostlib, text, ft, k, True, line_cap, long_read, hc, returns, n_reads)
        names.append(name)
        if name == "pieces":
            assert len(got) >= 6 + 4  # the lines beyond line_cap came in pieces
        if name == "bam":
            check_part(hostlib, text, ft, k, False, line_cap, long_read, hc, returns, n_reads)  # flag 0x10 reversed and complemented
    assert {"pieces", "long-titled", "long-untitled", "multiline-0", "multiline-1", "bam"} <= set(names)


# ---- 5: same-address adds and both sides of the table placement
@pytest.mark.parametrize("k", [3, 6, 7, 8, 13])
def test_same_address_adds_on_both_sides_of_the_table_placement(hostlib, k, monkeypatch):
    """a 9 000-symbol homopolymer at every k that takes another path: the 4^6-entry LDS table (k <= 6), the 4^7-entry one (k = 7), adds straight into the
    table in memory (k >= 8). With two workgroups only, each walks several tiles before it flushes; with the LDS table switched off the small k take the global path"""
    text = b">poly\n" + b"C" * 9000 + b"\n>other\n" + _rnd(np.random.default_rng(4), 3000) + b"\n>again\n" + b"ACAC" * 1200 + b"\n"
    returns = check_part(hostlib, text, 0, k, True, 1 << 17)
    assert smallk_nonzero(returns, k, True)[1].max() >= 9000 - k + 1
    monkeypatch.setenv("KMC_HIP_S1_SMALLK_WGS", "2")
    check_part(hostlib, text, 0, k, False, 1 << 17)
    if k <= 7:
        monkeypatch.setenv("KMC_HIP_S1_SMALLK_LDS_K", "0")
        check_part(hostlib, text, 0, k, True, 1 << 17)


def test_a_kmer_with_more_than_65535_copies_in_one_workgroup(hostlib, monkeypatch):
    """the workgroup-private counters are 32 bits wide: 70 000 copies of one k-mer through ONE workgroup's LDS table"""
    monkeypatch.setenv("KMC_HIP_S1_SMALLK_WGS", "1")
    text = b">poly\n" + b"G" * 70_004 + b"\n"
    returns = check_part(hostlib, text, 0, 5, True, 1 << 17)
    assert smallk_nonzero(returns, 5, True)[1].max() == 70_000


# ---- 6: accumulation
def test_parts_accumulate_over_calls_slots_and_threads(hostlib):
    k, both, lib = 9, True, hostlib
    rng = np.random.default_rng(11)
    texts = [_records_text("fq", b"\n", [_rnd(rng, int(n)) for n in rng.integers(20, 300, size=40)] + [b"A" * 400]) for _ in range(4)]
    each = [smallk_table(getseq_returns(t, 1, k, 1 << 17)[0], k, both)[0] for t in texts]
    lib.reopen(k, both)
    for t in texts[:2]:  # one after the other on one slot
        assert lib.part(t, k, both, 1, 1 << 17)[0] == 0
    want = each[0] + each[1]
    assert np.array_equal(lib.read_all(k), want)
    rcs = {}

    def work(slot, t):
        rcs[slot] = lib.part(t, k, both, 1, 1 << 17, slot=slot)[0]

    th = [threading.Thread(target=work, args=(1 + i, texts[2 + i])) for i in range(2)]  # two slots from two host threads at once
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert rcs == {1: 0, 2: 0}
    want = want + each[2] + each[3]
    assert np.array_equal(lib.read_all(k), want) and np.array_equal(lib.read_all(k), want)  # reading does not clear
    assert np.array_equal(np.concatenate([lib.read(f, min(5000, want.size - f)) for f in range(0, want.size, 5000)]), want)  # reads at chunk offsets
    lib.close_table()


# ---- 7: the product binary over the emulated library, and over a library without the capability
def _write_input(path, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == "ml":
        with open(path, "wb") as f:
            for i in range(300):
                f.write(b">ctg%d\n" % i + _wrap(synth.homopolymer_rich_sequence(rng, int(rng.integers(30, 2000)), 1.8, 0.2).tobytes(), 60, b"\n"))
    else:
        synth.make_long_reads(path, seed, [int(x) for x in rng.integers(30, 2000, size=300)], fmt=fmt, mean_run=1.8, lower_frac=0.2, n_run_per_mbp=3000, n_run_len=4)


_state = {"broken": False}


def _guarded(fn):
    if _state["broken"]:
        pytest.fail("an earlier run of kmc_hip_s1 with small k over the emulated library failed")
    try:
        return fn()
    except BaseException:
        _state["broken"] = True
        raise


@pytest.mark.parametrize("flags,fmt", E2E_SETS, ids=E2E_IDS)
def test_kmc_hip_s1_small_k_over_the_emulated_library_writes_the_reference_database(flags, fmt, tmp_path):
    _require("kmc", "kmc_hip_s1")
    inp = str(tmp_path / ("in." + fmt))
    _write_input(inp, fmt, 12)
    assert 200_000 < os.path.getsize(inp) < 900_000  # a few hundred kB
    _guarded(lambda: check_e2e(_exe("kmc"), _exe("kmc_hip_s1"), flags, inp, tmp_path, {"KMC_HIP_LIB": emu.build_hostlib("small")}))


def test_kmc_hip_s1_counts_a_k10_database_at_k9_over_the_emulated_library(tmp_path):
    """the reference's CI pair: a -k10 database fed to -k9 -fkmc"""
    _require("kmc", "kmc_hip_s1")
    inp = str(tmp_path / "in.fq")
    _write_input(inp, "fq", 13)

    def both():
        rc, _, log = run_kmc(_exe("kmc"), ["-k10", "-ci1", "-m2", "-sf1", "-sp2", "-sr2"], inp, tmp_path, "k10")
        assert rc == 0, log[-1500:]
        check_e2e(_exe("kmc"), _exe("kmc_hip_s1"), ["-k9", "-fkmc"], str(tmp_path / "db_k10"), tmp_path, {"KMC_HIP_LIB": emu.build_hostlib("small")})

    _guarded(both)


def test_kmc_hip_s1_small_k_over_a_library_without_the_capability_runs_the_reference_worker(tmp_path):
    """the mock library has neither kmc_hip_smallk_* nor the capability: the reference's CWSmallKSplitter counts, as before; no report line"""
    _require("kmc", "kmc_hip_s1")
    inp = str(tmp_path / "in.fq")
    _write_input(inp, "fq", 14)
    mock = emu.build_mock()
    assert not hasattr(ctypes.CDLL(mock), "kmc_hip_smallk_open")
    check_e2e(_exe("kmc"), _exe("kmc_hip_s1"), ["-k5", "-ci1"], inp, tmp_path, {"KMC_HIP_LIB": mock}, on_device=False)
