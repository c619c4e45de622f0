"""CPU: set operations between two ordered k-mer databases (`kmc_tools simple`) — kmc_hip_db_set_op_device in the PRODUCT'S host library compiled over the
emulated HIP runtime (tests/emu.py build_hostlib, small geometry; $KMC_HIP_SETOP_IPT = 1: merge tiles of 256 records), kmc_amd/dbio.py and
`python -m kmc_amd.tools simple` over it.

The oracle is the restatement of the semantics in tests/setops_cases.py (k-mers as Python ints, dicts). It is held to the databases `kmc_tools simple` itself
wrote (tests/golden/setops_*, made by tests/make_setops_golden.py), byte for byte, so it is pinned to the reference and not to the code under test. The -m gpu
file runs the same cases on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emu
import setops_cases as S
from kmc_amd import capi, dbio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECORRUPT, ECAPACITY = -1, -4, -5
TILE = 256


@pytest.fixture(scope="module")
def lib():
    os.environ["KMC_HIP_SETOP_IPT"] = "1"
    c = S.LibContext(emu.build_hostlib("small"))
    yield c
    c.close()
    del os.environ["KMC_HIP_SETOP_IPT"]


@pytest.fixture(scope="module")
def goldens():
    """per k: the two inputs (header, decoded body) — read once, shared"""
    out = {}
    for k in S.PAIRS:
        dbs = [S.golden_db(k, n) for n in "ab"]
        out[k] = (dbs, [S.decode_body(k, d.lut_prefix_len, d.counter_size, d.lut, d.recs) for d in dbs])
    return out


# ---- 1: the restatement is the reference
@pytest.mark.parametrize("k,line", S.GOLDEN_CASES, ids=S.GOLDEN_IDS)
def test_the_restatement_writes_what_kmc_tools_writes(goldens, k, line):
    (a, b), (da, db_) = goldens[k]
    r = S.resolve_line(line, S.header_of(a), S.header_of(b))
    kmers, counts, st = S.restate(da, db_, r["a_cut"], r["b_cut"], r["op"], r["oc"], r["ci"], r["cx"], r["cs"])
    lut, recs = S.encode_body(k, r["p_out"], r["cs_bytes"], kmers, counts)
    want = S.golden_db(k, line[0])
    assert (want.lut_prefix_len, want.counter_size, want.min_count, want.max_count, want.total_kmers) == (r["p_out"], r["cs_bytes"], r["ci"], r["cx"], st["n_written"])
    assert want.total_kmers > 0 and np.array_equal(lut, want.lut) and np.array_equal(recs, want.recs)


def test_the_output_counter_size_is_the_writers(lib):
    """kmc1_db_writer.h:154 MIN(BYTE_LOG(counter_max), BYTE_LOG(cutoff_max)) == kmc_hip_counter_size, except at counter_max == 1 (no counter when counting, one byte here)"""
    for cx in (1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, S.U32, 10**12):
        for cs in (2, 255, 256, 65535, 65536, 1 << 24, S.U32):
            assert lib.L.kmc_hip_counter_size(cx, cs) == min(S.byte_log(cs), S.byte_log(cx))
    assert lib.L.kmc_hip_counter_size(1000, 1) == 0


# ---- 2: the device call is the restatement
@pytest.mark.parametrize("k,line", S.GOLDEN_CASES, ids=S.GOLDEN_IDS)
def test_device_call_on_the_golden_inputs(lib, goldens, k, line):
    (a, b), _ = goldens[k]
    r = S.resolve_line(line, S.header_of(a), S.header_of(b))
    lut, recs, st = S.run_device(lib, k, (a.lut_prefix_len, a.counter_size, a.lut, a.recs), (b.lut_prefix_len, b.counter_size, b.lut, b.recs), r["a_cut"], r["b_cut"],
                                 r["op"], r["oc"], r["ci"], r["cx"], r["cs"], r["p_out"])
    want = S.golden_db(k, line[0])
    assert st["n_written"] == want.total_kmers
    assert np.array_equal(recs, want.recs) and np.array_equal(lut, want.lut)
    _, _, wst = S.restate(*goldens[k][1], r["a_cut"], r["b_cut"], r["op"], r["oc"], r["ci"], r["cx"], r["cs"])
    assert st == wst


@pytest.mark.parametrize("k,prefix_lens,reduced", S.PLANTED, ids=S.PLANTED_IDS)
def test_device_call_on_planted_databases(lib, k, prefix_lens, reduced):
    """every record width, SIZE 1 (k = 27, 32, 33) .. 7 (193, 224), and at k = 33, 35, 65, 129, 161, 193 the LUT prefix of A, of B and of the output across a 64-bit
    word boundary; databases of 3-4 merge tiles. The k this test was first written for run every case, the others the reduced list (setops_cases.REDUCED)"""
    cases = S.planted_cases(k, TILE, prefix_lens=prefix_lens, reduced=reduced)
    assert len(cases) == 16 if reduced else len(cases) > 40
    seen = dict(n_pairs=0, n_only_a=0, n_only_b=0, n_below_min=0, n_above_max=0, n_written=0)
    for name, a, b, kw in cases:
        try:
            st = S.check_case(lib, k, a, b, **kw)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")
        for key in seen:
            seen[key] += st[key]
    assert all(v > 0 for v in seen.values()), seen  # every tally was exercised


@pytest.mark.parametrize("k,prefix_lens,reduced", S.PLANTED, ids=S.PLANTED_IDS)
def test_the_planted_lists_exercise_every_tally(k, prefix_lens, reduced):
    """the restatement alone, for the merge tile of this file and for the device's (test_gpu_db_setops.py asserts nothing about the tallies' sum)"""
    for tile in (TILE, 256 * max(1, 8 // ((k + 31) // 32 + 1))):
        seen = dict(n_pairs=0, n_only_a=0, n_only_b=0, n_below_min=0, n_above_max=0, n_written=0)
        for _, a, b, kw in S.planted_cases(k, tile, prefix_lens=prefix_lens, reduced=reduced):
            cb_a, cb_b = kw["a_fmt"][1], kw["b_fmt"][1]
            st = S.restate((a[0], [c & ((1 << (8 * cb_a)) - 1) for c in a[1]]), (b[0], [c & ((1 << (8 * cb_b)) - 1) for c in b[1]]), kw.get("a_cut", (1, S.U32)), kw.get("b_cut", (1, S.U32)),
                           kw["op"], kw["oc"], kw.get("ci", 1), kw.get("cx", S.U32), kw.get("cs", S.U32))[2]
            for key in seen:
                seen[key] += st[key]
        assert all(v > 0 for v in seen.values()), (tile, seen)


@pytest.mark.parametrize("k,prefix_lens", S.SEAMS, ids=S.SEAM_IDS)
def test_cut_records_on_every_tile_seam(lib, k, prefix_lens):
    """equal key sets in both parities, one side or the other cut by its INPUT'S cutoffs at every position: so_step's pair-or-single decision from the halo record"""
    cases = S.seam_cut_cases(k, TILE, prefix_lens)
    assert len(cases) == 32
    cut = 0
    for name, a, b, kw in cases:
        try:
            st = S.check_case(lib, k, a, b, **kw)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")
        assert st["n_pairs"] + st["n_only_a"] + st["n_only_b"] > 0
        cut += len(a[0]) + len(b[0]) - 2 * st["n_pairs"] - st["n_only_a"] - st["n_only_b"]
    assert cut >= 32 * (len(cases[0][1][0]) - 1)  # in every case about half of all records are cut


# ---- 3: errors
def test_errors(lib):
    k = 27
    a = S.golden_db(k, "a")
    body = (a.lut_prefix_len, a.counter_size, a.lut, a.recs)
    common = dict(a_cut=(1, 255), b_cut=(1, 255), op="union", oc="sum", ci=1, cx=255, cs=255)

    def code(a_body=body, b_body=body, p_out=3, capacity=None, **kw):
        with pytest.raises(capi.KmcHipError) as e:
            S.run_device(lib, k, a_body, b_body, p_out=p_out, capacity=capacity, **dict(common, **kw))
        assert "kmc_hip_db_set_op_device" in str(e.value)
        return e.value.code

    assert code(p_out=4) == EINVAL  # (27 - 4) % 4 != 0
    assert code(a_body=(4, a.counter_size, np.zeros(256, dtype=np.uint64), a.recs[:0])) == EINVAL
    assert code(b_body=(2, a.counter_size, np.zeros(16, dtype=np.uint64), a.recs[:0])) == EINVAL
    assert code(a_body=(3, 0, a.lut, a.recs)) == EINVAL  # counter size 0
    assert code(b_body=(3, 5, a.lut, a.recs[:0])) == EINVAL
    n = a.total_kmers
    rb = a.rec_bytes
    assert code(capacity=2 * n * rb - 1) == ECAPACITY  # union: n_a + n_b records
    assert code(op="intersect", capacity=n * rb - 1) == ECAPACITY
    assert code(op="kmers_subtract", capacity=n * rb - 1) == ECAPACITY
    assert code(op="reverse_counters_subtract", capacity=n * rb - 1) == ECAPACITY
    bad = a.lut.copy()
    bad[-1] = n + 1
    assert code(a_body=(3, a.counter_size, bad, a.recs)) == ECORRUPT
    assert code(b_body=(3, a.counter_size, bad, a.recs)) == ECORRUPT
    # NULL arguments
    L, C = lib.L, lib.C
    v = capi.DbView(0, 0, 0, 3, 1, 1, 255)
    op = capi.DbOp(0, 0, 1, 255, 255, 3)
    n_out, st = C.c_uint64(), (C.c_uint64 * 6)()
    d = lib.malloc(1024)
    try:
        good = capi.DbView(d, 0, d, 3, 1, 1, 255)
        args = [lib.h, 0, k, C.byref(good), C.byref(good), C.byref(op), d, 1024, d, C.byref(n_out), st]
        for i in (3, 4, 5, 6, 8, 9, 10):
            bad_args = list(args)
            bad_args[i] = None
            assert L.kmc_hip_db_set_op_device(*bad_args) == EINVAL and b"NULL" in L.kmc_hip_last_error(lib.h)
        assert L.kmc_hip_db_set_op_device(lib.h, 0, k, C.byref(v), C.byref(good), C.byref(op), d, 1024, d, C.byref(n_out), st) == EINVAL  # an input without a LUT
        for bad_op in (capi.DbOp(6, 0, 1, 255, 255, 3), capi.DbOp(0, 6, 1, 255, 255, 3), capi.DbOp(0, 0, 0, 255, 255, 3), capi.DbOp(0, 0, 1, 0, 255, 3)):
            assert L.kmc_hip_db_set_op_device(lib.h, 0, k, C.byref(good), C.byref(good), C.byref(bad_op), d, 1024, d, C.byref(n_out), st) == EINVAL
        assert L.kmc_hip_db_set_op_device(lib.h, 0, 225, C.byref(good), C.byref(good), C.byref(capi.DbOp(0, 0, 1, 255, 255, 1)), d, 1024, d, C.byref(n_out), st) == EINVAL
    finally:
        lib.free(d)


def test_the_binding_knows_the_entry_point():
    assert "kmc_hip_db_set_op_device" in capi.SYMBOLS and hasattr(capi.Context, "db_set_op_device")
    assert list(capi.DB_OPS) == list(S.OPS) and set(capi.DB_COUNTER_OPS) == {"min", "max", "sum", "diff", "left", "right"}


# ---- 4: the front end
@pytest.mark.parametrize("k", S.PAIRS)
def test_dbio_round_trips_a_golden_database(k, tmp_path):
    for name in ("a", "union", "intersect_ocsum_cs65535" if k != 33 else "counters_subtract"):
        d = dbio.read_database(S.golden_path(k, name))
        assert not d.kmc2 and d.kmer_len == k and d.total_kmers * d.rec_bytes == d.recs.size and int(d.lut[-1]) <= d.total_kmers
        out = str(tmp_path / name)
        dbio.write_kmc1(out, d.kmer_len, d.counter_size, d.lut_prefix_len, d.min_count, d.max_count, d.both_strands, d.lut, d.recs, mode=d.mode)
        for ext in (".kmc_pre", ".kmc_suf"):
            assert open(out + ext, "rb").read() == open(S.golden_path(k, name) + ext, "rb").read(), (name, ext)


def _tools(args, **env):
    return subprocess.run([sys.executable, "-m", "kmc_amd.tools", *args], cwd=ROOT, capture_output=True, text=True, timeout=1200,
                          env=dict(os.environ, KMC_HIP_LIB=emu.build_hostlib("small"), KMC_HIP_SETOP_IPT="1", **env))


def _same_files(a, b):
    for ext in (".kmc_pre", ".kmc_suf"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), (a, ext)


@pytest.mark.parametrize("k", S.PAIRS)
def test_the_command_line_writes_the_golden_databases(k, tmp_path):
    """every golden line; the lines that share their input options go into one command, as kmc_tools takes them"""
    a, b = S.golden_path(k, "a"), S.golden_path(k, "b")
    plain = [ln for ln in S.LINES_OF[k] if not ln[1] and not ln[2]]
    args = ["simple", a, b]
    for ln in plain:
        args += [ln[3], str(tmp_path / ln[0]), *ln[4]]
    r = _tools(args)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    for ln in S.LINES_OF[k]:
        if ln not in plain:
            r = _tools(S.command_line(ln, a, b, str(tmp_path / ln[0])))
            assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
        _same_files(str(tmp_path / ln[0]), S.golden_path(k, ln[0]))


def test_the_command_line_names_what_it_refuses(tmp_path):
    a27, a55 = S.golden_path(27, "a"), S.golden_path(55, "a")
    r = _tools(["simple", a27, a55, "union", str(tmp_path / "o")])
    assert r.returncode != 0 and "different k-mer lengths" in r.stderr
    kff = str(tmp_path / "x.kff")
    with open(kff, "wb") as f:
        f.write(b"KFF\x01\x00" + bytes(32))
    r = _tools(["simple", kff, a27, "union", str(tmp_path / "o")])
    assert r.returncode != 0 and "KFF" in r.stderr
    r = _tools(["simple", a27, a27, "union", str(tmp_path / "o"), "-okff"])
    assert r.returncode != 0 and "KFF" in r.stderr
    d = dbio.read_database(a27)
    sb = (27 - d.lut_prefix_len) // 4
    dbio.write_kmc1(str(tmp_path / "set"), 27, 0, d.lut_prefix_len, 1, 255, True, d.lut, d.recs.reshape(-1, sb + 1)[:, :sb].copy())
    r = _tools(["simple", str(tmp_path / "set"), a27, "union", str(tmp_path / "o")])
    assert r.returncode != 0 and "counter size 0" in r.stderr
    assert not os.path.exists(str(tmp_path / "o") + ".kmc_pre")


@pytest.mark.parametrize("k", sorted(S.RAW_A))
def test_the_command_line_orders_a_kmc2_fixture_first(k, tmp_path):
    """the database as `kmc` wrote it (KMC2, tests/golden/setops_k<k>_raw_a) as first input: ordered on the device, then united with b == the `union` golden"""
    raw = S.golden_path(k, S.RAW_A[k])
    assert dbio.read_database(raw).kmc2
    r = _tools(["simple", raw, S.golden_path(k, "b"), "union", str(tmp_path / "u")])
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    _same_files(str(tmp_path / "u"), S.golden_path(k, "union"))


def test_the_command_line_orders_a_kmc2_input_first(ref_bins, tmp_path):
    if ref_bins is None:
        pytest.skip("oracle/_ref not shipped")
    from kmc_amd import synth

    dbs = []
    for i, seed in enumerate((3, 4)):
        fq = str(tmp_path / f"r{i}.fq")
        synth.write_fastq(fq, np.concatenate([synth.make_reads(50, 3000, 40, 150, 0.004), synth.make_reads(60 + seed, 3000, 20, 150, 0.004)]))
        (tmp_path / f"t{i}").mkdir()
        subprocess.run([ref_bins["kmc"], "-k27", "-ci1", "-t2", fq, str(tmp_path / f"db{i}"), str(tmp_path / f"t{i}")], check=True, capture_output=True)
        dbs.append(str(tmp_path / f"db{i}"))
    assert dbio.read_database(dbs[0]).kmc2
    tail = lambda d: ["union", str(tmp_path / d / "u"), "-ocmax", "counters_subtract", str(tmp_path / d / "c"), "-ci2"]  # noqa: E731
    (tmp_path / "ref").mkdir()
    (tmp_path / "got").mkdir()
    subprocess.run([ref_bins["kmc_tools"], "simple", dbs[0], dbs[1], "-ci2", *tail("ref")], check=True, capture_output=True)
    r = _tools(["simple", dbs[0], dbs[1], "-ci2", *tail("got")])
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    for o in "uc":
        _same_files(str(tmp_path / "got" / o), str(tmp_path / "ref" / o))
        assert dbio.read_database(str(tmp_path / "got" / o)).total_kmers > 100
