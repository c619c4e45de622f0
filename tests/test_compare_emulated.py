"""CPU: `kmc_tools compare`, `check` and `info` — kmc_hip_db_compare_device in the PRODUCT'S host library compiled over the emulated HIP runtime (tests/emu.py
build_hostlib, small geometry; $KMC_HIP_COMPARE_STEPS = 1: compare tiles of 256 words, so that databases of a few hundred records cross wave and tile seams),
kmc_amd/dbio.py and `python -m kmc_amd.tools compare | check | info` over it.

The oracle of the compare is the restatement in tests/compare_cases.py (k-mers as Python ints). It is held to what `kmc_tools compare` itself printed for the recorded
lines (tests/golden/toolsline_*, made by tests/make_compare_golden.py), so the planted cases rest on the reference and not on the code under test. The command lines
must reproduce the recorded stdout, stderr and exit status byte for byte. The -m gpu file runs the same cases on the device."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import compare_cases as CC
import emu
import setops_cases as S
from kmc_amd import capi, dbio, tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECORRUPT = -1, -4
U32 = 0xFFFFFFFF
STEPS = 1
ENV = dict(KMC_HIP_COMPARE_STEPS=str(STEPS), KMC_HIP_QUERY_IPT="1")


@pytest.fixture(scope="module")
def lib():
    os.environ.update(ENV)
    c = CC.CompareContext(emu.build_hostlib("small"))
    yield c
    c.close()
    for key in ENV:
        del os.environ[key]


@pytest.fixture
def reversed_tiles(monkeypatch):
    monkeypatch.setenv("KMC_HIP_COMPARE_REVERSED", "1")


# ---- 1: the restatement is the reference
@pytest.mark.parametrize("line", [ln for ln in CC.LINES if ln[1][0] == "compare"], ids=lambda ln: ln[0])
def test_the_restatement_prints_what_kmc_tools_prints(line):
    (a, a_cut), (b, b_cut) = CC.compare_inputs(line)
    want = CC.read_golden(line)
    assert CC.report(CC.restate(a, b, a_cut, b_cut)) == (want["stdout"], want["status"]) and want["stderr"] == ""


def test_the_recorded_lines_are_what_they_are_for():
    by = {ln[0]: CC.read_golden(ln) for ln in CC.LINES}
    assert {by[n]["stdout"] for n in by if n.startswith("cmp_")} == {"DB Equals\n", "DB Differs\n", "one of input is not finished\nDB Differs\n"}
    assert by["chk_k27_at_cx"]["stdout"] == "0\n" and by["chk_k27_below_cx"]["stdout"] == "5\n"  # the cutoff_max rule of check
    assert by["chk_k27_kff_absent"] == dict(stdout="", stderr="", status=0)
    assert by["chk_k27_too_short"]["stderr"] == "Error: invalid k-mer length\n" and by["chk_k27_with_n"]["stderr"] == "Error: invalid k-mer format\n"
    assert by["info_k27_kff_multi"]["stdout"].count("\tnb_blocks") == 58 and by["info_k27_kff_multi"]["stderr"].startswith("footer values:\n")
    a, b = CC.compare_inputs(("x", ["compare", "{g}/setops_k27_a", "{g}/setops_k27_b"]))
    res = CC.restate(a[0], b[0], a[1], b[1])
    assert (res["kind"], res["ordinal"], res["counter_a"], res["counter_b"]) == (1, 0, 3, 12)  # the first records: 3 against 12 occurrences


# ---- 2: the device call
@pytest.mark.parametrize("k,p", CC.WIDTHS, ids=CC.WIDTH_IDS)
def test_planted_pairs(lib, k, p):
    """three tiles and a third of 256 words; every case asserts all eight result words"""
    for name, a, b, kw in CC.planted_cases(k, p, STEPS, reduced=k not in (27, 65)):
        try:
            CC.check_case(lib, k, a, b, **kw)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")


@pytest.mark.parametrize("k,p", [(27, 3), (33, 5), (65, 5), (127, 3), (224, 4)], ids=["27-p3", "33-p5", "65-p5", "127-p3", "224-p4"])
def test_the_smaller_of_two_differences_wins_with_the_tiles_reversed(lib, reversed_tiles, k, p):
    """the tiles taken last to first: the later difference is published first; the tile in front of the published record's — and that record's own, where it lies
    across the seam — must still be walked"""
    ran = 0
    for name, a, b, kw in CC.planted_cases(k, p, STEPS, reduced=True):
        if name.startswith(("two_", "both_", "a_short_and", "counter_at_seam", "kmer_at_seam", "cut_and_a", "uncut_differs")):
            try:
                CC.check_case(lib, k, a, b, **kw)
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}")
            ran += 1
    assert ran > 10


def test_records_are_located_across_compaction_tiles(lib, monkeypatch):
    """product tiles (2048 words) and 3 400 records: the record numbers of the first difference lie in the third and later compaction tiles of 256 records"""
    monkeypatch.setenv("KMC_HIP_COMPARE_STEPS", "8")
    ran = [CC.check_case(lib, 27, a, b, **kw) for name, a, b, kw in CC.planted_cases(27, 3, 8, reduced=True)
           if name.startswith(("cut_and_a", "cut_makes_equal_every", "uncut_differs_tile", "cut_in_a_last", "two_", "cut_makes_different"))]
    assert len(ran) >= 6 and max(r["record_b"] for r in ran) > 3 * 256


def test_the_golden_bodies(lib):
    """a against b at k = 27 and 55 (they differ in the first record), a against itself under cutoffs on one side and on both"""
    for k in (27, 55):
        a, b = (dbio.read_database(S.golden_path(k, n)) for n in "ab")
        bodies = [(d.lut_prefix_len, d.counter_size, d.lut, d.recs) for d in (a, b)]
        lists = [S.decode_body(k, *body) for body in bodies]
        for a_cut, b_cut in (((1, 255), (1, 255)), ((2, 255), (1, 255)), ((2, 9), (2, 9)), ((200, 255), (1, 255)), ((200, 255), (200, 255))):
            assert CC.run_device(lib, k, bodies[0], bodies[1], a_cut, b_cut) == CC.restate(lists[0], lists[1], a_cut, b_cut)
            assert CC.run_device(lib, k, bodies[0], bodies[0], a_cut, b_cut) == CC.restate(lists[0], lists[0], a_cut, b_cut)


# ---- 3: errors and legal edges
def test_errors_and_edges(lib):
    k = 27
    a = dbio.read_database(S.golden_path(27, "a"))
    good = (a.lut_prefix_len, a.counter_size, a.lut, a.recs)
    bad_lut = a.lut.copy()
    bad_lut[-1] = a.total_kmers + 1

    def code(x, y, kk=k):
        with pytest.raises(capi.KmcHipError) as e:
            CC.run_device(lib, kk, x, y)
        assert "kmc_hip_db_compare_device" in str(e.value)
        return e.value.code

    for bad, want in (((3, 0, a.lut, a.recs), EINVAL), ((3, 5, a.lut, a.recs[:0]), EINVAL), ((4, 1, np.zeros(256, dtype=np.uint64), a.recs[:0]), EINVAL),  # (27 - 4) % 4 != 0
                      ((16, 1, np.zeros(4, dtype=np.uint64), a.recs[:0]), EINVAL), ((3, 1, bad_lut, a.recs), ECORRUPT)):
        assert code(bad, good) == want and code(good, bad) == want
    L, C = lib.L, lib.C
    d = lib.malloc(4096)
    try:
        v = capi.DbView(d, 0, d, 3, 1, 1, 255)
        res = (C.c_uint64 * 8)()
        args = [lib.h, 0, k, C.byref(v), C.byref(v), res]
        for i in (3, 4, 5):
            assert L.kmc_hip_db_compare_device(*[None if j == i else x for j, x in enumerate(args)]) == EINVAL and b"NULL" in L.kmc_hip_last_error(lib.h)
        for broken in (capi.DbView(d, 0, 0, 3, 1, 1, 255), capi.DbView(0, 5, d, 3, 1, 1, 255)):  # no LUT; records announced and none given
            assert L.kmc_hip_db_compare_device(lib.h, 0, k, C.byref(broken), C.byref(v), res) == EINVAL
            assert L.kmc_hip_db_compare_device(lib.h, 0, k, C.byref(v), C.byref(broken), res) == EINVAL
        w = capi.DbView(d, 0, d, 1, 1, 1, 255)
        assert L.kmc_hip_db_compare_device(lib.h, 0, 225, C.byref(w), C.byref(w), res) == EINVAL  # kmer_len > 224
        assert L.kmc_hip_db_compare_device(lib.h, 1, k, C.byref(v), C.byref(v), res) == EINVAL  # no such device
    finally:
        lib.free(d)
    # legal: both empty with NULL records; empty against the golden body; everything cut on both sides
    empty = (3, 1, np.zeros(64, dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    n = a.total_kmers
    assert CC.run_device(lib, k, empty, empty) == dict.fromkeys(CC.RESULT, 0)
    first = int(a.recs[a.rec_bytes - 1])
    assert CC.run_device(lib, k, empty, good) == dict(kind=3, ordinal=0, n_a=0, n_b=n, counter_a=0, counter_b=first, record_a=0, record_b=0)
    assert CC.run_device(lib, k, good, empty) == dict(kind=4, ordinal=0, n_a=n, n_b=0, counter_a=first, counter_b=0, record_a=0, record_b=0)
    assert CC.run_device(lib, k, good, good, (100, 200), (201, 255)) == dict.fromkeys(CC.RESULT, 0)


def test_the_binding_knows_the_entry_point():
    assert "kmc_hip_db_compare_device" in capi.SYMBOLS and hasattr(capi.Context, "db_compare_device")
    assert capi.DBC_RESULT == CC.RESULT and capi.DBC_KINDS == CC.KINDS
    with open(os.path.join(ROOT, "include", "kmc_hip.h")) as f:
        header = f.read()
    assert "int kmc_hip_db_compare_device(" in header and "#define KMC_HIP_ABI_VERSION 4 " in header
    for i, name in enumerate(("EQUAL", "COUNTER", "KMER", "A_ENDED", "B_ENDED")):
        assert f"KMC_HIP_DBC_{name} = {i}" in header
    for i, name in enumerate(CC.RESULT):
        assert f"KMC_HIP_DBC_RES_{name.upper()} = {i}" in header


# ---- 4: the command lines
def _in_process(line, ctx):
    """-> (stdout, stderr, exit status) of tools.main's three new modes with the library handed in"""
    argv = CC.argv_of(line)
    out, err = io.StringIO(), io.StringIO()
    status = 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            if argv[0] == "compare":
                res = tools.compare(argv[1:], ctx=ctx)
                out.write(tools.compare_report(res))
                status = 0 if res["kind"] == "equal" else 1
            elif argv[0] == "check":
                out.write(tools.check(argv[1:], ctx=ctx))
            else:
                o, e = tools.info(argv[1:])
                out.write(o)
                err.write(e)
        except SystemExit as e:  # what the interpreter does with it: the message and a line end to stderr, status 1
            err.write(f"{e.code}\n")
            status = 1
    return dict(stdout=out.getvalue(), stderr=err.getvalue(), status=status)


@pytest.mark.parametrize("line", CC.LINES, ids=CC.LINE_IDS)
def test_the_command_line_prints_the_recorded_lines(lib, line):
    assert _in_process(line, lib) == CC.read_golden(line)


def test_compare_returns_the_result_and_the_two_kmers(lib):
    res = tools.compare([S.golden_path(27, "a"), S.golden_path(27, "b")], ctx=lib)
    assert res == dict(kind="counter", ordinal=0, n_a=3448, n_b=res["n_b"], counter_a=3, counter_b=12, record_a=0, record_b=0, kmer_a="AAAAAACCTGACTCGCGTTTCTCTGCG",
                       kmer_b="AAAAAACGGAAGAAAAAGGTACTCGAG")
    a = S.golden_path(27, "a")
    res = tools.compare([a, a, "-ci2"], ctx=lib)  # A's third record is the first one counted once; B's third present record is its fifth
    (la, _), _ = CC.compare_inputs(("x", ["compare", a, a]))
    want = CC.restate(la, la, (1, U32), (2, U32))
    assert {key: res[key] for key in CC.RESULT[1:]} == {key: want[key] for key in CC.RESULT[1:]} and res["kind"] == CC.KINDS[want["kind"]] == "counter"
    assert (res["ordinal"], res["record_a"], res["record_b"], res["counter_a"]) == (2, 2, 4, 1) and res["kmer_a"] == "AAAAAAGGTTTCTGAAGGTGGTGGATC" and res["kmer_b"] != res["kmer_a"]
    res = tools.compare([a, "-ci200", a], ctx=lib)
    assert (res["kind"], res["kmer_a"], res["kmer_b"], res["record_a"]) == ("a_ended", None, "AAAAAACCTGACTCGCGTTTCTCTGCG", 3448)
    assert tools.compare([a, CC.K.kff_file("kff_k27_a")], ctx=lib) == dict(kind="equal", ordinal=0, n_a=3448, n_b=3448, counter_a=0, counter_b=0, record_a=0, record_b=0)


def test_check_kmers(lib, monkeypatch):
    """a batch through the reads query in parts of four k-mers: present, absent, the first and the last of the database, a k-mer whose reverse complement alone is present,
    lower case, and a counter equal to -cx"""
    monkeypatch.setenv("KMC_HIP_CHECK_PART_MB", str(4 * 28 / (1 << 20)))
    a = S.golden_path(27, "a")
    kmers, counts = S.decode_body(27, *(lambda d: (d.lut_prefix_len, d.counter_size, d.lut, d.recs))(dbio.read_database(a)))
    text = lambda x: "".join("ACGT"[(x >> (2 * (26 - i))) & 3] for i in range(27))  # noqa: E731
    batch = ["AAAAAAGGGATCCTCGCAGGTCGCAAA", "AAAAAAGGGATCCTCGCAGGTCGCAAC", text(kmers[0]), text(kmers[-1]), CC.RC_ONLY_27, "aaaaaaGGGATCCTCGCAGGTcgcaaa"] + [text(x) for x in kmers[100:110]]
    want = [4, 0, counts[0], counts[-1], 0, 4] + counts[100:110]
    got = tools.check_kmers(a, batch, ctx=lib)
    assert got.dtype == np.uint32 and got.tolist() == want
    five = text(kmers[counts.index(5)])
    assert tools.check_kmers(a, [five, batch[0], five], cx=5, ctx=lib).tolist() == [0, 4, 0]  # equal to cutoff_max: absent in this mode alone
    assert tools.check_kmers(a, [five, batch[0]], ci=5, cx=6, ctx=lib).tolist() == [5, 0]
    assert tools.check_kmers(a, [], ctx=lib).size == 0
    assert tools.check_kmers(CC.K.kff_file("kff_k27_multi"), ["CACGTTCTTGTGTGTCGGTTGTGACTA", "CACGTTCTTGTGTGTCGGTTGTGACTC"], ctx=lib).tolist() == [4, 0]
    assert tools.check_kmers(S.golden_path(33, "raw_a"), ["TTTATAACTATTAGGAGACGTTGACACCGAAAA", "CACCGCGCCTAGTGCTCCGCACCACCGTAGGTG"], ctx=lib).tolist() == [16, 2]
    for bad, why in ((["ACGT"], "length"), ([batch[0], batch[0][:-1] + "N"], "format")):
        with pytest.raises(tools.UsageError) as e:
            tools.check_kmers(a, bad, ctx=lib)
        assert why in str(e.value)


def test_info_opens_no_device(monkeypatch):
    monkeypatch.setenv("KMC_HIP_LIB", "/nonexistent/libkmc_hip.so")
    monkeypatch.setattr(capi, "Context", None)
    for name in ("info_k27_kmc1", "info_k33_kmc2", "info_k27_kff_multi"):
        line = next(ln for ln in CC.LINES if ln[0] == name)
        want = CC.read_golden(line)
        assert tools.info(CC.argv_of(line)[1:]) == (want["stdout"], want["stderr"])


def test_read_kff_keeps_what_its_callers_read():
    """the fields `info` needs are added; the flattened sections stay"""
    f = dbio.read_kff(CC.K.kff_file("kff_k27_multi"))
    assert len(f.scopes) == 1 and f.sections == f.scopes[0][1] and len(f.sections) == 58 and f.scopes[0][0]["k"] == 27
    assert f.encoding == dbio.KFF_ENCODING and f.all_unique == 1 and f.footer["min_count"] == f.min_count


@pytest.mark.parametrize("line", CC.LINES, ids=CC.LINE_IDS)
def test_python_m_kmc_amd_tools(line):
    """the process as a user starts it, on every recorded line"""
    r = subprocess.run([sys.executable, "-m", "kmc_amd.tools", *CC.argv_of(line)], cwd=ROOT, capture_output=True, text=True, timeout=1200,
                       env=dict(os.environ, KMC_HIP_LIB=emu.build_hostlib("small"), **ENV))
    assert dict(stdout=r.stdout, stderr=r.stderr, status=r.returncode) == CC.read_golden(line)


def test_usage():
    for argv in ([], ["frobnicate"]):
        with pytest.raises(tools.UsageError) as e:
            tools.main(argv)
        for mode in ("simple", "filter", "transform", "complex", "compare", "check", "info", "count"):
            assert f"kmc_amd.tools {mode} " in str(e.value), mode
    a = S.golden_path(27, "a")

    def refused(fn, argv, *words):
        with pytest.raises(tools.UsageError) as e:
            fn(argv)
        assert all(w in str(e.value) for w in words), str(e.value)

    refused(tools.compare, [], "usage")
    refused(tools.compare, [a], "Input database source missed")
    refused(tools.compare, [a, "-ci2", "-cx3", "-ci4", a], "Input database source required, but -ci4found")
    refused(tools.compare, [a, "-cs3", a], "Unknow parameter: -cs3")
    refused(tools.compare, [a, a, a], "Unknow parameter")
    refused(tools.compare, [a, S.golden_path(55, "a")], "contains 27-mers", "contains 55-mers")
    refused(tools.check, [a], "check operation require k-mer to check")
    refused(tools.check, [a, "-okmc", "ACGT"], "Unknow parameter: -okmc")
    refused(tools.check, ["-ci2", a], "Input database source required")
    refused(tools.info, [], "usage")
    refused(tools.info, [os.path.join(ROOT, "tests", "golden", "no_such_database")], "no_such_database")
