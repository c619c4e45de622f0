"""CPU: one k-mer database transformed (`kmc_tools transform`) — kmc_hip_db_reduce_device, kmc_hip_db_histogram_device and kmc_hip_db_dump_device in the PRODUCT'S
host library compiled over the emulated HIP runtime (tests/emu.py build_hostlib, small geometry; $KMC_HIP_DUMP_TILE = 200: dump tiles of 200 records, reduce tiles are 256),
kmc_amd/dbio.py and `python -m kmc_amd.tools transform` over it.

The oracle is the restatement of the semantics in tests/transform_cases.py (k-mers as Python ints). It is held to what `kmc_tools transform` itself wrote
(tests/golden/transform_*, made by tests/make_transform_golden.py), byte for byte, so it is pinned to the reference and not to the code under test. The -m gpu file runs the
same cases on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emu
import setops_cases as S
import transform_cases as T
from kmc_amd import capi, dbio, tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECORRUPT, ECAPACITY = -1, -4, -5
DUMP_TILE = 200
TILE = 256  # the planted databases are 3 1/3 of the larger tile long


@pytest.fixture(scope="module")
def lib():
    os.environ["KMC_HIP_DUMP_TILE"] = str(DUMP_TILE)
    c = T.TransformContext(emu.build_hostlib("small"))
    yield c
    c.close()
    del os.environ["KMC_HIP_DUMP_TILE"]


@pytest.fixture(scope="module")
def inputs():
    """the golden inputs, read once: fixture -> (database, its (kmers, counts) in file order)"""
    out = {}
    for fixture in sorted({ln[1] for ln in T.LINES}):
        db = dbio.read_database(T.fixture_path(fixture))
        out[fixture] = (db, T.file_order(db))
    return out


@pytest.fixture(scope="module")
def restated(inputs):
    return {ln[0]: T.restate_line(ln, inputs[ln[1]][0]) for ln in T.LINES}


def test_the_fixtures_are_what_the_cases_assume(inputs):
    shape = {f: (db.total_kmers, db.lut_prefix_len, db.counter_size, db.kmc2) for f, (db, _) in inputs.items()}
    assert shape == {"setops_k27_a": (3448, 3, 1, False), "setops_k33_a": (8473, 5, 1, False), "setops_k33_raw_a": (8473, 5, 1, True), "setops_k55_a": (3301, 3, 1, False)}
    counts = inputs["setops_k27_a"][1][1]
    assert (min(counts), max(counts), sum(c >= 10 for c in counts)) == (1, 25, 1278)
    raw = inputs["setops_k33_raw_a"][0]
    assert len(raw.bins) == 64 and raw.raw_lut.size == 64 * 1024 + 1 and int(raw.raw_lut[-1]) == raw.total_kmers and raw.raw_recs.size == raw.total_kmers * raw.rec_bytes


# ---- 1: the restatement is the reference
@pytest.mark.parametrize("line", T.LINES, ids=T.LINE_IDS)
def test_the_restatement_writes_what_kmc_tools_writes(inputs, restated, line, tmp_path):
    db = inputs[line[1]][0]
    got = restated[line[0]]
    assert [g[0] for g in got] == [i for i, (op, _) in enumerate(line[3]) if not (op[0] == "sort" and not db.kmc2)] and got
    for idx, kind, want, _ in got:
        if kind == "text":
            assert want == T.read_golden_text(line, idx) and len(want) > 0, (line[0], idx)
        else:
            assert T.database_files(db.kmer_len, want, db.both_strands, db.mode, str(tmp_path / "db")) == T.golden_database_files(line, idx), (line[0], idx)
    for i in range(len(line[3])):  # a sort of an ordered input writes nothing
        if i not in [g[0] for g in got]:
            assert not os.path.exists(T.golden_out(line, i) + ".kmc_pre")


def test_the_raw_dump_is_in_bin_order(restated):
    raw, ordered = restated["k33raw_dump"][0][2], restated["k33raw_dump_s"][0][2]
    assert raw != ordered and sorted(raw.split(b"\n")) == sorted(ordered.split(b"\n"))
    assert restated["k33raw_reduce_dump"][1][2] == ordered  # a database output on the line: the plain dump is ordered too


# ---- 2: the device calls on the golden inputs
def _body_of(lib, db):
    if db.kmc2:
        return T.DeviceBody(lib, db.kmer_len, db.lut_prefix_len, db.counter_size, db.raw_lut, db.raw_recs, n_seg=len(db.bins))
    return T.DeviceBody(lib, db.kmer_len, db.lut_prefix_len, db.counter_size, db.lut, db.recs)


@pytest.mark.parametrize("line", T.LINES, ids=T.LINE_IDS)
def test_device_calls_on_the_golden_inputs(lib, inputs, restated, line):
    """the body as it lies in the file where the line needs no order (a KMC2 body under its segmented LUT); where it does, the ordered twin among the fixtures"""
    db = inputs[line[1]][0]
    k = db.kmer_len
    in_cut, need_order, res = T.resolve_line(line, dict(S.header_of(db), kmc2=db.kmc2))
    src = inputs["setops_k33_a"][0] if (db.kmc2 and need_order) else db
    with _body_of(lib, src) as body:
        for r, (idx, kind, want, wst) in zip(res, restated[line[0]]):
            if r["op"] == "histogram":
                hist, st = T.run_histogram(lib, body, in_cut, r["ci"], r["cx"])
                assert T.histogram_text([int(x) for x in hist], r["ci"]) == T.read_golden_text(line, idx)
            elif r["op"] == "dump":
                text, st = T.run_dump(lib, body, in_cut, r["ci"], r["cx"], r["cs"])
                assert text == T.read_golden_text(line, idx)
            else:
                p_out = S.best_p(k, db.total_kmers)
                lut, recs, st = T.run_reduce(lib, body, in_cut, r["ci"], r["cx"], r["cs"], r["value"], p_out)
                g = dbio.read_database(T.golden_out(line, idx))
                assert (g.lut_prefix_len, g.total_kmers, g.min_count, g.max_count) == (p_out, st["n_written"], r["ci"], r["cx"])
                assert np.array_equal(recs, g.recs) and np.array_equal(lut, g.lut)
            assert st == wst, (line[0], idx, st, wst)


# ---- 3: planted databases
@pytest.mark.parametrize("k,p,p_out", T.KS, ids=T.K_IDS)
def test_planted_databases(lib, k, p, p_out):
    """every record width of the reduce template (SIZE 1 .. 7) and the prefix inside and across a 64-bit word; reduce, dump and histogram on every case"""
    cases = T.planted_cases(k, p, TILE)
    assert len(cases) > 20
    seen = dict.fromkeys(T.TALLIES, 0)
    seen_h = dict(n_cut_in=0, n_outside=0, n_counted=0)
    for name, c in cases:
        lut, recs = S.encode_body(k, p, c["cb"], c["kmers"], c["counts"])
        try:
            with T.DeviceBody(lib, k, p, c["cb"], lut, recs) as body:
                st = T.check_reduce(lib, body, c["kmers"], c["counts"], c["in_cut"], c["ci"], c["cx"], c["cs"], c["value"], p_out)
                if not c["value"]:
                    assert T.check_dump(lib, body, c["kmers"], c["counts"], c["in_cut"], c["ci"], c["cx"], c["cs"]) == st
                sth = T.check_histogram(lib, body, c["counts"], c["in_cut"], *T.histogram_window(c))
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")
        for key in seen:
            seen[key] += st[key]
        for key in seen_h:
            seen_h[key] += sth[key]
    assert all(v > 0 for v in seen.values()) and all(v > 0 for v in seen_h.values()), (seen, seen_h)  # every tally was exercised


@pytest.mark.parametrize("k,p", [(27, 3), (33, 5), (65, 9)])
def test_dump_and_histogram_of_a_segmented_body(lib, k, p):
    """a KMC2-shaped LUT: empty segments at the front, in the middle and at the end, prefixes that recur; dumped in file order, whole and in ranges that start and end
    inside tiles and concatenate to the whole"""
    segments, kmers, counts = T.segmented_case(k, p, TILE)
    lut, recs = T.encode_segmented(k, p, 1, segments)
    assert T.decode_segmented(k, p, 1, lut, recs) == (kmers, counts) and kmers != sorted(kmers)
    with T.DeviceBody(lib, k, p, 1, lut, recs, n_seg=len(segments)) as body:
        T.check_dump(lib, body, kmers, counts, (1, S.U32), 1, S.U32, S.U32)
        T.check_dump(lib, body, kmers, counts, (5, 150), 20, 120, 99)
        T.check_histogram(lib, body, counts, (5, 150), 20, 120)
        whole, _ = T.restate_dump(k, kmers, counts, (5, 150), 20, 120, 99)
        cuts = [0, 1, DUMP_TILE - 1, DUMP_TILE + 77, 2 * DUMP_TILE + 77, 2 * DUMP_TILE + 78, len(kmers) - 3, len(kmers)]
        parts, tallies = [], dict.fromkeys(T.TALLIES, 0)
        for a, b in zip(cuts, cuts[1:]):
            want, wst = T.restate_dump(k, kmers[a:b], counts[a:b], (5, 150), 20, 120, 99)
            text, st = T.run_dump(lib, body, (5, 150), 20, 120, 99, first=a, count=b - a, base_offset=len(parts) % 16)
            assert (text, st) == (want, wst), (a, b)
            parts.append(text)
        assert b"".join(parts) == whole


def test_the_text_starts_at_every_byte_offset(lib):
    """d_text at each of the 16 residues of an address: the copy's head, aligned body and tail; a capacity of exactly count x (k + 12); the guard behind *n_bytes intact"""
    k, p = 27, 3
    rng = np.random.default_rng(1)
    n = 2 * DUMP_TILE + 31
    kmers = S.random_kmers(rng, k, n)
    counts = [T.DIGIT_EDGES[i % 12] for i in range(n)]
    lut, recs = S.encode_body(k, p, 3, kmers, counts)
    with T.DeviceBody(lib, k, p, 3, lut, recs) as body:
        for off in range(16):
            T.check_dump(lib, body, kmers, counts, (1, S.U32), 1, S.U32, S.U32, base_offset=off, capacity=n * (k + 12))
        for count in (1, 2, 3):  # texts shorter than the 15 bytes of a head … a little longer
            T.check_dump(lib, body, kmers[:count], counts[:count], (1, S.U32), 1, S.U32, S.U32, base_offset=7, count=count)


def test_histogram_in_lds_and_in_hbm_agree(lib):
    k, p = 27, 3
    rng = np.random.default_rng(2)
    n = 3 * TILE + 85
    kmers = S.random_kmers(rng, k, n)
    counts = [1 if x < 0.7 else int(2 + rng.geometric(0.05)) for x in rng.random(n)]
    lut, recs = S.encode_body(k, p, 2, kmers, counts)
    with T.DeviceBody(lib, k, p, 2, lut, recs) as body:
        a, _ = T.run_histogram(lib, body, (1, S.U32), 1, T.HIST_LDS_BINS)  # the widest range in LDS
        b, _ = T.run_histogram(lib, body, (1, S.U32), 1, T.HIST_LDS_BINS + 1)  # one more: 64-bit atomics in HBM
        assert np.array_equal(a, b[:-1]) and b[-1] == 0 and np.array_equal(a[:400], np.bincount(counts, minlength=401)[1:401])
        T.check_histogram(lib, body, counts, (2, 60), 3, 40)  # bin 0 is not counter 0
        T.check_histogram(lib, body, counts, (1, S.U32), 1, 1)  # one bin


def test_histogram_of_counters_near_the_top(lib):
    k, p = 27, 3
    rng = np.random.default_rng(3)
    n = TILE + 9
    kmers = S.random_kmers(rng, k, n)
    counts = [S.U32 - int(x) for x in rng.integers(0, 6, size=n)]
    lut, recs = S.encode_body(k, p, 4, kmers, counts)
    with T.DeviceBody(lib, k, p, 4, lut, recs) as body:
        T.check_histogram(lib, body, counts, (1, S.U32), S.U32 - 3, S.U32)
        T.check_histogram(lib, body, counts, (1, S.U32 - 1), S.U32 - 4, S.U32 - 2)


# ---- 4: errors and legal edges
def test_errors_and_edges(lib):
    k = 27
    a = dbio.read_database(T.fixture_path("setops_k27_a"))
    n = a.total_kmers
    good = (a.lut_prefix_len, a.counter_size, a.lut, a.recs)

    def code(fn, who, body=good, n_seg=1, **kw):
        with T.DeviceBody(lib, k, *body, n_seg=n_seg) as b, pytest.raises(capi.KmcHipError) as e:
            fn(lib, b, **kw)
        assert who in str(e.value)
        return e.value.code

    red = dict(in_cut=(1, 255), ci=1, cx=255, cs=255, value=0, p_out=3)
    dmp = dict(in_cut=(1, 255), ci=1, cx=255, cs=255)
    hst = dict(in_cut=(1, 255), ci=1, cx=255)
    bad = a.lut.copy()
    bad[-1] = n + 1
    for fn, who, kw in ((T.run_reduce, "kmc_hip_db_reduce_device", red), (T.run_dump, "kmc_hip_db_dump_device", dmp), (T.run_histogram, "kmc_hip_db_histogram_device", hst)):
        assert code(fn, who, body=(3, 0, a.lut, a.recs), **kw) == EINVAL  # counter size 0
        assert code(fn, who, body=(3, 5, a.lut, a.recs[:0]), **kw) == EINVAL
        assert code(fn, who, body=(4, 1, np.zeros(256, dtype=np.uint64), a.recs[:0]), **kw) == EINVAL  # (27 - 4) % 4 != 0
        assert code(fn, who, **dict(kw, ci=0)) == EINVAL
        assert code(fn, who, body=(3, 1, bad, a.recs), **kw) == ECORRUPT
    assert code(T.run_reduce, "kmc_hip_db_reduce_device", **dict(red, p_out=4)) == EINVAL
    assert code(T.run_reduce, "kmc_hip_db_reduce_device", **dict(red, cs=0)) == EINVAL
    assert code(T.run_reduce, "kmc_hip_db_reduce_device", capacity=n * a.rec_bytes - 1, **red) == ECAPACITY
    assert code(T.run_dump, "kmc_hip_db_dump_device", capacity=n * (k + 12) - 1, **dmp) == ECAPACITY
    assert code(T.run_dump, "kmc_hip_db_dump_device", first=n - 1, count=2, **dmp) == EINVAL
    assert code(T.run_dump, "kmc_hip_db_dump_device", n_seg=0, **dmp) == EINVAL
    assert code(T.run_histogram, "kmc_hip_db_histogram_device", **dict(hst, ci=9, cx=8)) == EINVAL
    # a segmented LUT is checked at its closing entry
    seg_lut = np.concatenate([a.lut, a.lut[-1:], np.full(63, n, dtype=np.uint64), [n + 1]]).astype(np.uint64)
    assert code(T.run_dump, "kmc_hip_db_dump_device", body=(3, 1, seg_lut, a.recs), n_seg=2, **dmp) == ECORRUPT
    # legal: an empty database, an empty range, everything cut (an empty output under a LUT of zeros)
    empty = (3, 1, np.zeros(64, dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    with T.DeviceBody(lib, k, *empty) as b:
        lut, recs, st = T.run_reduce(lib, b, **red)
        assert recs.size == 0 and not lut.any() and st == dict.fromkeys(T.TALLIES, 0)
        assert T.run_dump(lib, b, **dmp) == (b"", dict.fromkeys(T.TALLIES, 0))
        hist, st = T.run_histogram(lib, b, **hst)
        assert not hist.any() and sum(st.values()) == 0
    with T.DeviceBody(lib, k, *good) as b:
        assert T.run_dump(lib, b, first=100, count=0, **dmp) == (b"", dict.fromkeys(T.TALLIES, 0))
        assert T.run_dump(lib, b, first=n, count=0, **dmp)[0] == b""
        lut, recs, st = T.run_reduce(lib, b, **dict(red, ci=200))
        assert recs.size == 0 and not lut.any() and st == dict(n_cut_in=0, n_below_min=n, n_above_max=0, n_written=0)
        assert T.run_dump(lib, b, **dict(dmp, in_cut=(100, 200))) == (b"", dict(n_cut_in=n, n_below_min=0, n_above_max=0, n_written=0))
    # NULL arguments
    L, C = lib.L, lib.C
    d = lib.malloc(4096)
    try:
        v = capi.DbView(d, 0, d, 3, 1, 1, 255)
        n_out, st = C.c_uint64(), (C.c_uint64 * 4)()
        args = [lib.h, 0, k, C.byref(v), 1, 255, 255, 0, 3, d, 1024, d, C.byref(n_out), st]
        for i in (3, 9, 11, 12, 13):
            assert L.kmc_hip_db_reduce_device(*[None if j == i else x for j, x in enumerate(args)]) == EINVAL and b"NULL" in L.kmc_hip_last_error(lib.h)
        args = [lib.h, 0, k, C.byref(v), 1, 1, 255, d, st]
        for i in (3, 7, 8):
            assert L.kmc_hip_db_histogram_device(*[None if j == i else x for j, x in enumerate(args)]) == EINVAL and b"NULL" in L.kmc_hip_last_error(lib.h)
        args = [lib.h, 0, k, C.byref(v), 1, 0, 0, 1, 255, 255, d, 1024, C.byref(n_out), st]
        for i in (3, 12, 13):
            assert L.kmc_hip_db_dump_device(*[None if j == i else x for j, x in enumerate(args)]) == EINVAL and b"NULL" in L.kmc_hip_last_error(lib.h)
        no_lut = capi.DbView(d, 0, 0, 3, 1, 1, 255)
        assert L.kmc_hip_db_dump_device(lib.h, 0, k, C.byref(no_lut), 1, 0, 0, 1, 255, 255, d, 1024, C.byref(n_out), st) == EINVAL
        assert L.kmc_hip_db_reduce_device(lib.h, 0, 225, C.byref(capi.DbView(d, 0, d, 1, 1, 1, 255)), 1, 255, 255, 0, 1, d, 1024, d, C.byref(n_out), st) == EINVAL  # kmer_len > 224
    finally:
        lib.free(d)


# ---- 5: the binding
def test_the_binding_knows_the_entry_points():
    for name in ("reduce", "histogram", "dump"):
        assert f"kmc_hip_db_{name}_device" in capi.SYMBOLS and hasattr(capi.Context, f"db_{name}_device")
    assert capi.DBT_STATS == T.TALLIES and capi.DBH_STATS == ("n_cut_in", "n_outside", "n_counted")
    with open(os.path.join(ROOT, "include", "kmc_hip.h")) as f:
        header = f.read()
    for name in ("reduce", "histogram", "dump"):
        assert f"int kmc_hip_db_{name}_device(" in header


# ---- 6: the command line
def _check_outputs(line, paths):
    for i, (op, _) in enumerate(line[3]):
        if T.is_text(op):
            assert open(paths[i], "rb").read() == T.read_golden_text(line, i), (line[0], i)
        elif os.path.exists(T.golden_out(line, i) + ".kmc_pre"):
            assert tuple(open(paths[i] + e, "rb").read() for e in (".kmc_pre", ".kmc_suf")) == T.golden_database_files(line, i), (line[0], i)
        else:
            assert not os.path.exists(paths[i] + ".kmc_pre"), "a sort of an ordered input was written"


@pytest.mark.parametrize("line", T.LINES, ids=T.LINE_IDS)
def test_the_command_line_writes_the_golden_files(lib, restated, line, tmp_path, monkeypatch):
    monkeypatch.setenv("KMC_HIP_DUMP_PART_MB", "0.008")  # 8 KiB of text a part: 186 records at k = 33, 45 parts
    paths = [str(tmp_path / T.out_name(line, i)) for i in range(len(line[3]))]
    sts = tools.transform(T.command_line(line, T.fixture_path(line[1]), paths)[1:], ctx=lib)
    _check_outputs(line, paths)
    assert len(sts) == len(restated[line[0]])
    for st, (_, _, _, wst) in zip(sts, restated[line[0]]):
        assert {key: st[key] for key in wst} == wst


def test_a_sort_of_an_ordered_input_alone_writes_nothing(lib, tmp_path, capsys):
    assert tools.transform([T.fixture_path("setops_k33_a"), "sort", str(tmp_path / "o")], ctx=lib) == []
    assert os.listdir(tmp_path) == [] and "already sorted" in capsys.readouterr().err


def test_python_m_kmc_amd_tools_transform(tmp_path):
    """the process as a user starts it: the KMC2 input, a sorted dump, a histogram and a reduce on one command line"""
    line = ("cli", "setops_k33_raw_a", [], [(["dump", "-s"], []), (["histogram"], []), (["reduce"], ["-ci2"])])
    paths = [str(tmp_path / n) for n in ("out.txt", "h.txt", "r")]
    r = subprocess.run([sys.executable, "-m", "kmc_amd.tools", *T.command_line(line, T.fixture_path(line[1]), paths)], cwd=ROOT, capture_output=True, text=True, timeout=1200,
                       env=dict(os.environ, KMC_HIP_LIB=emu.build_hostlib("small"), KMC_HIP_DUMP_TILE=str(DUMP_TILE), KMC_HIP_DUMP_PART_MB="0.05"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    by = {ln[0]: ln for ln in T.LINES}
    assert open(paths[0], "rb").read() == T.read_golden_text(by["k33raw_dump_s"], 0)
    assert open(paths[1], "rb").read() == T.read_golden_text(by["k33raw_hist"], 0)
    assert tuple(open(paths[2] + e, "rb").read() for e in (".kmc_pre", ".kmc_suf")) == T.golden_database_files(by["k33raw_reduce_dump"], 0)
    assert r.stdout.count("->") == 3 and "n_written 7850" in r.stdout


# ---- 7: what the command line refuses
def test_the_command_line_names_what_it_refuses(tmp_path):
    a, out = T.fixture_path("setops_k27_a"), str(tmp_path / "o")
    kff = tmp_path / "x.kff"
    kff.write_bytes(b"KFF\x01\x00")

    def refused(argv, *words):
        with pytest.raises(tools.UsageError) as e:
            tools.transform(argv)
        assert all(w in str(e.value) for w in words), str(e.value)

    refused([str(kff), "dump", out], "KFF")
    refused([a, "reduce", out, "-okff"], "KFF")
    refused([a, "reduce", "-s", out], "-s", "dump")
    refused([a, "histogram", "-s", out], "-s", "dump")
    refused([a, "dump", out, "-okmc"], "-o", "compact, reduce, set_counts and sort")
    refused([a, "histogram", out, "-okmc"], "-o")
    refused([a, "reduce"], "Output path missed")
    refused([a, "dump", "-s"], "Output path missed")
    refused([a], "at least one")
    refused([a, "set_counts"], "count value")
    refused([a, "set_counts", "x7", out], "Count value expected")
    refused([a, "set_counts", "-3", out], "Count value expected")
    refused([a, "set_counts", "4294967296", out], "4294967295")
    refused([a, "frobnicate", out], "unknown operation")
    refused([a, "histogram", out, "-cx300000000"], "2^28", "268435456")
    refused([a, "-ci2", "-q", "dump", out], "unknown input option")
    assert os.listdir(tmp_path) == ["x.kff"]
    (o,) = tools.parse_transform([a, "-ci2", "histogram", out, "-ci0", "-cx0"])[1]  # 0 is taken as 1 (parameters_parser.cpp:16-25)
    assert (o["ci"], o["cx"]) == (1, 1)
