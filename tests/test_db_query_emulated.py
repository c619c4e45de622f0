"""CPU: the reads of a file against an ordered k-mer database (`kmc_tools filter`) — kmc_hip_db_query_reads_device in the PRODUCT'S host library compiled over the
emulated HIP runtime (tests/emu.py build_hostlib, small geometry; $KMC_HIP_QUERY_IPT = 1: lookup tiles of 256 window starts), kmc_amd/readsio.py and
`python -m kmc_amd.tools filter` over it.

The oracle is the restatement of the semantics in tests/query_cases.py. It is held to the files `kmc_tools -t1 filter` itself wrote (tests/golden/filter_out_*, made by
tests/make_filter_golden.py), byte for byte, so it is pinned to the reference and not to the code under test. The -m gpu file runs the same cases on the device."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import emu
import query_cases as Q
import setops_cases as S
from kmc_amd import capi, readsio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECORRUPT = -1, -4
TILE = 256
PLANTED = [(27, 3), (32, 4), (33, 5), (33, 1), (64, 4), (65, 5)]  # tiles of 256: read 0 of the layout (3 k + 8 symbols at least) ends on the first seam up to k = 82


@pytest.fixture(scope="module")
def lib():
    os.environ["KMC_HIP_QUERY_IPT"] = "1"
    c = Q.LibContext(emu.build_hostlib("small"))
    yield c
    c.close()
    del os.environ["KMC_HIP_QUERY_IPT"]


@pytest.fixture()
def runner(lib):
    r = Q.Runner(lib)
    yield r
    r.close()


# ---- 1: the restatement is the reference
@pytest.mark.parametrize("line", Q.LINES, ids=Q.LINE_IDS)
def test_the_restatement_writes_what_kmc_tools_writes(line):
    want = Q.golden_out(line[0])
    assert len(want) > 1000 and Q.restate_filter(line) == want


def test_the_goldens_cover_what_they_are_for():
    fq = readsio.parse(gzip.open(os.path.join(Q.GOLDEN, Q.FQ), "rb").read(), True)
    fa = readsio.parse(gzip.open(os.path.join(Q.GOLDEN, Q.FA), "rb").read(), False)
    lens = fq.seq[1] - fq.seq[0]
    assert len(fq) == len(fa) == 200 and np.array_equal(lens, fa.seq[1] - fa.seq[0])
    assert lens.min() < 27 and (lens == 27).any() and (lens == 33).any() and lens.max() > 300
    text = fq.text.tobytes()
    assert b"N" in text and b"\r\n" in text and np.isin(readsio.sequence_buffer(fq)[0], np.frombuffer(b"acgt", dtype=np.uint8)).any()
    assert np.any(fq.plus[1] - fq.plus[0] > 1) and np.any(fq.plus[1] - fq.plus[0] == 1)
    long_fq = readsio.parse(gzip.open(os.path.join(Q.GOLDEN, Q.FQ_LONG), "rb").read(), True)
    assert (long_fq.seq[1] - long_fq.seq[0]).min() >= 33
    modes = {(tuple(ln[3]), "-fa" in ln[6], "-fa" in ln[6] or "-fa" in ln[7]) for ln in Q.LINES if ln[1] == 27}
    assert len(modes) == 9  # normal, -t, -hm x fq->fq, fq->fa, fa->fa


# ---- 2: the device call is the restatement
@pytest.mark.parametrize("k,p", PLANTED, ids=[f"{k}-p{p}" for k, p in PLANTED])
def test_device_call_on_planted_cases(runner, k, p):
    seen = dict.fromkeys(Q.STATS, 0)
    cases = Q.planted_cases(k, p, TILE)
    assert len(cases) == (9 if k % 2 == 0 else 8)
    for case in cases:
        st = Q.check_case(runner, case)
        for key in seen:
            seen[key] += st[key]
    assert all(v > 0 for v in seen.values()), seen  # every tally was exercised


@pytest.mark.parametrize("k,p", Q.PLANTED, ids=Q.PLANTED_IDS)
def test_the_planted_lists_exercise_every_rule(k, p):
    """the restatement alone, at the tile of this file (where the layout fits) and at the device's: what the planted list is for is in it"""
    for tile in (TILE, Q.product_tile(k)):
        if tile - 1 < 3 * k + 8:
            continue
        seen = dict.fromkeys(Q.STATS, 0)
        for case in Q.planted_cases(k, p, tile):
            counters, n_valid, trim, masked, st = Q.restate(case)
            for key in seen:
                seen[key] += st[key]
            if case["name"].startswith("main_") and case["name"] != "main_cb2_thr1_cut":
                lens = np.diff(case["read_off"].astype(np.int64)) - 1
                assert lens[0] == tile - 1 and lens[1] > 3 * tile and {0, k - 1, k} <= set(lens.tolist())
                m0 = masked[:tile - 1] == ord("N")
                assert m0[0] and m0[-1] and not m0[k] and m0[k + 2:3 * k + 4].all()  # runs that reach both ends, touch and overlap
                assert trim[0] == 0 and trim[5] == k - 1 + 7 and trim[6] == lens[6] and n_valid[4] == 1 and n_valid[3] == 0
                assert 0 < np.count_nonzero(masked[tile:tile + lens[1]] == ord("N")) < lens[1]
                assert (counters[:tile - k] > 0).all() and np.count_nonzero(counters[tile - k:tile]) == 0  # found up to the seam, nothing behind a read's last window
            if case["name"] == "bounds":
                assert (counters[case["read_off"][:-1].astype(np.int64)] > 0).tolist() == [True, True, False, False, False, False, True, True, False, False, True, False, False, False, False]
            if case["name"] == "reverse_complement_alone_forward_db":
                assert n_valid.tolist() == [0, 0, 1, 1]
            if case["name"] in ("reverse_complement_canonical_db", "own_reverse_complement"):
                assert (n_valid > 0).all()
        assert all(v > 0 for v in seen.values()), (tile, seen)


def test_an_invalid_symbol_at_every_offset_around_a_seam(runner):
    """k = 27: the 'N' moves from k symbols in front of the first seam to k behind it; only the 2 k windows over it are lost"""
    k, p = 27, 3
    case, shifted = Q.shifted_invalid(k, p, TILE)
    runner.set_db(k, p, case["cb"], case["db"], case["cut"])
    base, st0 = Q.restate_counters(case["seq"], k, True, case["db"], *case["cut"])
    assert st0["n_invalid_windows"] == k + 1 and np.count_nonzero(base) == base.size - 2 * k  # the k windows over the 'N', the one over the terminator
    for d in range(2 * k + 1):
        seq, off = shifted(d)
        got, n_valid, _, _, st = runner.run(k, True, seq, off, 1, want=("counters", "n_valid"))
        want = np.concatenate([np.zeros(d, dtype=np.uint32), base])
        assert np.array_equal(got, want), (d, np.flatnonzero(got != want)[:8])
        assert st == dict(st0, n_invalid_windows=st0["n_invalid_windows"] + d) and n_valid[-1] == np.count_nonzero(base)
        if d in (1, 2 * k):  # the shifted expectation is the restatement's
            assert np.array_equal(Q.restate_counters(seq, k, True, case["db"], *case["cut"])[0], want)


def test_legal_edges(runner):
    k, p = 27, 3
    case = Q.planted_cases(k, p, TILE)[0]
    runner.set_db(k, p, case["cb"], case["db"], case["cut"])
    seq, off = Q.layout([b"ACGTACGTAC", b"", b"ACG"])
    counters, n_valid, trim, masked, st = runner.run(k, True, seq, off, 2)  # n_bytes < kmer_len
    assert not counters.any() and not n_valid.any() and not trim.any() and np.array_equal(masked, seq) and st == dict.fromkeys(Q.STATS, 0)
    counters, _, _, masked, st = runner.run(k, True, case["seq"], np.zeros(1, dtype=np.uint64), 2, want=("counters", "masked"))  # no reads: a copy
    want = Q.restate_counters(case["seq"], k, True, case["db"], *case["cut"])
    assert np.array_equal(counters, want[0]) and st == want[1] and np.array_equal(masked, case["seq"])
    # no read table at all
    d_seq, d_cnt = runner._buf("seq", seq.size), runner._buf("cnt", 4 * seq.size)
    assert lib_call(runner, k, d_seq, seq.size, 0, 0, d_cnt) == 0
    assert lib_call(runner, k, 0, 0, 0, 0, 0) == 0  # nothing at all


def lib_call(runner, k, d_seq, n, d_off, n_reads, d_cnt, d_nv=0, d_tl=0, d_mk=0, view=None, stats=True):
    L, C = runner.ctx.L, runner.ctx.C
    st = (C.c_uint64 * 4)()
    return L.kmc_hip_db_query_reads_device(runner.ctx.h, 0, C.byref(view or runner.view), k, 1, d_seq or None, n, d_off or None, n_reads, 2, d_cnt or None, d_nv or None, d_tl or None,
                                           d_mk or None, st if stats else None)


# ---- 3: errors
def test_errors(lib, runner):
    k, p = 27, 3
    case = Q.planted_cases(k, p, TILE)[0]
    runner.set_db(k, p, case["cb"], case["db"], case["cut"])
    seq, off = Q.layout([b"ACGT" * 10, b"TTGCA" * 8, b""])
    good = runner.run(k, True, seq, off, 2)
    d = {n: runner.bufs[n][0] for n in ("seq", "off", "cnt", "nv", "tl", "mk")}
    n, n_reads = seq.size, 3
    v = runner.view

    def code(**kw):
        args = dict(d_seq=d["seq"], n=n, d_off=d["off"], n_reads=n_reads, d_cnt=d["cnt"], d_nv=d["nv"], d_tl=d["tl"], d_mk=d["mk"])
        args.update(kw)
        rc = lib_call(runner, args.pop("k", k), **args)
        assert rc == 0 or b"kmc_hip_db_query_reads_device" in lib.L.kmc_hip_last_error(lib.h)
        return rc

    assert code() == 0
    # NULL arguments
    for kw in (dict(d_seq=0), dict(d_cnt=0), dict(d_off=0), dict(stats=False), dict(d_off=0, n_reads=0), dict(d_off=0, n_reads=0, d_nv=0, d_tl=0)):
        assert code(**kw) == EINVAL and b"NULL" in lib.L.kmc_hip_last_error(lib.h), kw
    assert code(d_off=0, n_reads=0, d_nv=0, d_tl=0, d_mk=0) == 0
    assert code(view=capi.DbView(v.d_recs, v.n_recs, 0, p, 1, 1, 255)) == EINVAL  # a database without a LUT
    assert code(view=capi.DbView(0, v.n_recs, v.d_lut, p, 1, 1, 255)) == EINVAL  # records claimed, none given
    for cs in (0, 5):
        assert code(view=capi.DbView(v.d_recs, v.n_recs, v.d_lut, p, cs, 1, 255)) == EINVAL
    for bad_p in (0, 4, 16, 27, 31):
        assert code(view=capi.DbView(v.d_recs, v.n_recs, v.d_lut, bad_p, 1, 1, 255)) == EINVAL, bad_p
    assert code(k=225, view=capi.DbView(v.d_recs, v.n_recs, v.d_lut, 1, 1, 1, 255)) == EINVAL
    # a LUT that ends behind the records
    assert code(view=capi.DbView(v.d_recs, 3, v.d_lut, p, 1, 1, 255)) == ECORRUPT
    # bad offsets: not ascending, behind n_bytes, a read whose terminator is a valid symbol
    for bad_off in ([0, 50, 41, n], [0, 41, 82, n + 1], [0, 40, 82, n], [0, 41, 41, n], [5, 41, 82, 2 ** 40]):
        lib.h2d(d["off"], np.array(bad_off, dtype=np.uint64))
        assert code() == ECORRUPT, bad_off
    lib.h2d(d["off"], off)
    assert code() == 0  # the sticky error was cleared
    again = runner.run(k, True, seq, off, 2)
    assert all(np.array_equal(a, b) for a, b in zip(good[:4], again[:4])) and good[4] == again[4]


def test_the_binding_knows_the_entry_point():
    assert "kmc_hip_db_query_reads_device" in capi.SYMBOLS and hasattr(capi.Context, "db_query_reads_device")
    assert capi.DBQ_STATS == Q.STATS
    hdr = open(os.path.join(ROOT, "include", "kmc_hip.h")).read()
    assert "#define KMC_HIP_ABI_VERSION 4" in hdr and "int kmc_hip_db_query_reads_device(" in hdr


# ---- 4: reads files
FQ_OK = b"@r1 x\nACGT\n+r1\nIIII\n@r2\r\nAC\r\n+\r\nII\r\n"


def test_readsio_cuts_records():
    r = readsio.parse(FQ_OK, True)
    t = FQ_OK
    cut = lambda sp, i: t[sp[0][i]:sp[1][i]]  # noqa: E731
    assert len(r) == 2 and [cut(r.header, i) for i in (0, 1)] == [b"@r1 x", b"@r2"] and [cut(r.seq, i) for i in (0, 1)] == [b"ACGT", b"AC"]
    assert [cut(r.plus, i) for i in (0, 1)] == [b"+r1", b"+"] and [cut(r.qual, i) for i in (0, 1)] == [b"IIII", b"II"] and r.rec_end.tolist() == [20, len(t)]
    buf, off = readsio.sequence_buffer(r)
    assert buf.tobytes() == b"ACGT\nAC\n" and off.tolist() == [0, 5, 8]
    a = readsio.parse(b">a\nACGT\n>b\r\nGG\r\n", False)
    assert len(a) == 2 and a.plus is None and readsio.sequence_buffer(a)[0].tobytes() == b"ACGT\nGG\n"
    assert len(readsio.parse(b"", True)) == 0
    assert readsio.whole_records(np.frombuffer(FQ_OK[:30], dtype=np.uint8), True) == 20 and readsio.whole_records(np.frombuffer(FQ_OK[:19], dtype=np.uint8), True) == 0


@pytest.mark.parametrize("text,fastq", [
    (b">r1\nACGT\n+\nIIII\n", True), (b"@r1\nACGT\n-\nIIII\n", True), (b"@r1\nACGT\n+\nIII\n", True), (b"@r1\nACGT\n+\nIIIII\n", True), (b"@r1\nACGT\n+\nIIII", True),
    (b"@r1\nACGT\n+\n", True), (b"@r1\n\n+\n\n", True), (b"@r1\nAC\tGT\n+\nIIIII\n", True), (b"@r1\nAC\rGT\n+\nIIIII\n", True), (b"@r1\nACGT\n+\nII\xc3I\n", True),
    (b"@r1\nACGT\n+\nIIII\n\n", True), (b"@r1\nACGT\n>r2\nAC\n", False), (b">r1\nACGT\n>r2\n", False), (b">r1\nACGT", False), (b">r1\nAC\nGT\n>r2\nAA\n", False)])
def test_readsio_fails_closed(text, fastq):
    with pytest.raises(readsio.FormatError):
        readsio.parse(text, fastq)


def test_readsio_parts_are_whole_records(tmp_path):
    gz = os.path.join(Q.GOLDEN, Q.FQ)
    whole = gzip.open(gz, "rb").read()
    plain = str(tmp_path / "r.fq")
    with open(plain, "wb") as f:
        f.write(whole)
    for path in (plain, gz):
        got = list(readsio.parts(path, True, 3000))
        assert len(got) > 10 and b"".join(p.tobytes() for p in got) == whole
        assert sum(len(readsio.parse(p, True)) for p in got) == 200


# ---- 5: the front end
def _tools(args, **env):
    return subprocess.run([sys.executable, "-m", "kmc_amd.tools", *args], cwd=ROOT, capture_output=True, text=True, timeout=1200,
                          env=dict(os.environ, KMC_HIP_LIB=emu.build_hostlib("small"), KMC_HIP_QUERY_IPT="1", **env))


@pytest.mark.parametrize("line", Q.LINES, ids=Q.LINE_IDS)
def test_the_command_line_writes_the_golden_files(line, tmp_path):
    out = str(tmp_path / "out")
    r = _tools(Q.command_line(line, out), KMC_HIP_FILTER_PART_MB="0.02")  # parts of about 20 KB: every file in several
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    assert open(out, "rb").read() == Q.golden_out(line[0])
    assert "n_reads 200" in r.stdout


def test_the_command_line_takes_a_list_of_files(tmp_path):
    lst = str(tmp_path / "list.txt")
    with open(lst, "w") as f:
        f.write(os.path.join(Q.GOLDEN, Q.FQ) + "\n\n" + os.path.join(Q.GOLDEN, Q.FQ) + "\n")
    line = Q.LINES[0]
    out = str(tmp_path / "out")
    args = Q.command_line(line, out)
    args[args.index(os.path.join(Q.GOLDEN, Q.FQ))] = "@" + lst
    r = _tools(args)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    assert open(out, "rb").read() == 2 * Q.golden_out(line[0])


def test_the_command_line_names_what_it_refuses(tmp_path):
    a27, fq, fa, out = S.golden_path(27, "a"), os.path.join(Q.GOLDEN, Q.FQ), os.path.join(Q.GOLDEN, Q.FA), str(tmp_path / "o")
    for args, msg in ((["filter", "-t", a27, fq, "-ci0.5", out], "not compatibile with float"), (["filter", "-hm", a27, fq, "-cx0.5", out], "not compatibile with float"),
                      (["filter", a27, fq, "-ci0.5", "-cx10", out], "real number [0;1] or as integer"), (["filter", a27, fq, "-ci2", "-cx0.9", out], "real number [0;1] or as integer"),
                      (["filter", a27, fq, "-ci1.5", out], "wrong value"), (["filter", a27, fa, "-fa", out, "-fq"], "cannot set -fq for output"),
                      (["filter", a27, fq], "Output fastq source missed"), (["filter", a27], "Input fastq files(s) missed"), (["filter", a27, fq, out, "-okff"], "KFF"),
                      (["filter", a27, "@" + str(tmp_path / "none"), out], "No "), (["filter", a27, fa, out], "does not start with '@'"), (["filter", a27, fq, "-fa", out], "does not start with '>'")):
        r = _tools(args)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr[-500:])
    kff = str(tmp_path / "x.kff")
    with open(kff, "wb") as f:
        f.write(b"KFF\x01\x00" + bytes(32))
    r = _tools(["filter", kff, fq, out])
    assert r.returncode != 0 and "KFF" in r.stderr
    r = _tools(["filter"])
    assert r.returncode != 0 and "shorter than k" in r.stderr  # the usage text says what happens to them
