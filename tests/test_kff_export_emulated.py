"""CPU: KFF output — kmc_hip_db_kff_export_device (k_kff_frame) in the PRODUCT'S host library compiled over the emulated HIP runtime (tests/emu.py build_hostlib, small
geometry; $KMC_HIP_KFF_IPT = 1: tiles of 256 records), kmc_amd/dbio.write_kff, `python -m kmc_amd.tools export` and `count` with output_format="kff" over it.

The oracle is the restatement of container and record in tests/kff_cases.py, which tests/test_kff_emulated.py holds to the reference's own files; the expected files are
reference outputs recorded under tests/golden (kff_*.kff with the import, kffout_*.kff by tests/make_kffout_golden.py). The -m gpu file runs the same cases on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emu
import kff_cases as K
import kffout_cases as X
import setops_cases as S
from kmc_amd import capi, dbio, tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = X.tile_records(27, 3, 1, ipt=1)
ENV = {"KMC_HIP_KFF_IPT": "1", "KMC_HIP_KFF_PART_MB": "0.01"}  # tiles of 256 records; parts of about 1300 records, so that the recorded files go through in several


@pytest.fixture(scope="module")
def lib():
    os.environ.update(ENV)
    c = X.ExportContext(emu.build_hostlib("small"))
    yield c
    c.close()
    for key in ENV:
        del os.environ[key]


def golden(name):
    with open(X.kff_file(name), "rb") as f:
        return f.read()


# ---- 1: the recorded files (these fail without the feature: the verb and the symbol do not exist)
@pytest.mark.parametrize("name", list(X.OLD_FILES))
def test_export_writes_the_files_recorded_with_the_import(lib, name, tmp_path):
    out = str(tmp_path / "o")
    st = tools.export(X.export_argv(name, out), ctx=lib)
    assert open(out + ".kff", "rb").read() == golden(name)
    assert st["n_written"] == K.FILE_SHAPES[name][3] and os.listdir(tmp_path) == ["o.kff"]


def test_the_command_line_writes_a_recorded_file(tmp_path):
    """the verb through main, in a process of its own"""
    out = str(tmp_path / "o")
    r = subprocess.run([sys.executable, "-m", "kmc_amd.tools", "export", *X.export_argv("kff_k27_a", out)], cwd=ROOT, capture_output=True, text=True, timeout=1200,
                       env=dict(os.environ, KMC_HIP_LIB=emu.build_hostlib("small"), **ENV))
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    assert open(out + ".kff", "rb").read() == golden("kff_k27_a") and r.stdout.startswith(f"export -> {out}.kff: ")


def test_the_entry_returns_the_record_bytes_of_the_recorded_file(lib):
    db = dbio.read_database(S.golden_path(27, "a"))
    h = K.decode_container(golden("kff_k27_a"))
    (off, n), = h["sections"]
    got = X.run_export(lib, 27, db.lut_prefix_len, db.counter_size, db.lut, db.recs)
    assert n == db.total_kmers and got == golden("kff_k27_a")[off:off + n * (7 + 1)]


@pytest.mark.parametrize("name", list(X.FILES))
def test_export_writes_the_new_recorded_files(lib, name, tmp_path):
    out = str(tmp_path / "o")
    tools.export(X.export_argv(name, out), ctx=lib)
    raw = open(out + ".kff", "rb").read()
    assert raw == golden(name)
    h = K.decode_container(raw)
    k, ds, n, ci, cx = X.FILE_SHAPES[name]
    got = (h["k"], h["cs"], sum(m for _, m in h["sections"]), h["min_count"], h["max_count"])
    assert len(h["sections"]) == 1 and all(w is None or w == g for w, g in zip((k, ds, n, ci, cx), got)), got  # what the FILE says: data_size 3 for -cs70000


# ---- 2: the entry on planted bodies
@pytest.mark.parametrize("k,p", X.WIDTHS, ids=X.WIDTH_IDS)
def test_planted_bodies_and_round_trips(lib, k, p):
    """every case as one ascending body and as a segmented body in file order; import(export) and export(import) on each"""
    cases = X.planted_cases(k, p, TILE)
    assert len(cases) >= 30
    for name, cs, sections in cases:
        try:
            X.round_trips(lib, k, p, cs, sections)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")


def test_five_records_under_the_widest_lut(lib):
    k, p = X.WIDEST
    rng = np.random.default_rng(9)
    n_pref = 1 << (2 * p)
    for name, prefixes in (("spread", [0, 1, n_pref // 2, n_pref - 2, n_pref - 1]), ("random", None)):
        ks = S.random_kmers(rng, k, 5) if prefixes is None else sorted(S.random_kmers(rng, k, 1, lo_prefix=x, p=p)[0] for x in prefixes)
        lut, recs, kmers, counts = X.ordered_body(k, p, 3, [(ks, [1, 1 << 16, 65535, 65536, (1 << 24) - 1])])
        X.check_export(lib, k, p, 3, lut, recs, kmers, counts)
        X.check_export(lib, k, p, 3, lut, recs, kmers, counts, first=1, count=3)


@pytest.mark.parametrize("cs", [1, 2, 3, 4])
def test_every_data_size(lib, cs):
    """counters of cs bytes at the byte edges, framed with every data_size from cs to 4; 2 tiles and a few records"""
    k, p = 27, 3
    kmers = S.random_kmers(np.random.default_rng(cs), k, 2 * TILE + 9)
    lut, recs, kmers, counts = X.ordered_body(k, p, cs, [(kmers, K.edge_counts(cs, len(kmers)))])
    for ds in range(cs, 5):
        X.check_export(lib, k, p, cs, lut, recs, kmers, counts, ds=ds)
    slut, srecs, skmers, scounts = X.segmented_body(k, p, cs, K.split(kmers, counts, [TILE - 1, TILE + 70]))
    X.check_export(lib, k, p, cs, slut, srecs, skmers, scounts, n_seg=3, ds=4)


@pytest.mark.parametrize("k,p", [(27, 3), (33, 9), (64, 4)])
def test_ranges(lib, k, p):
    """ranges that start and end inside tiles; three ranges side by side are the whole; count 0 anywhere"""
    n = 3 * TILE + TILE // 3 + 5
    kmers = S.random_kmers(np.random.default_rng(k), k, n)
    lut, recs, kmers, counts = X.ordered_body(k, p, 2, [(kmers, K.edge_counts(2, n))])
    whole = X.check_export(lib, k, p, 2, lut, recs, kmers, counts)
    for first, count in ((1, n - 2), (TILE - 1, 2), (TILE, TILE), (TILE + 3, TILE - 3), (TILE // 2, 2 * TILE), (n - 1, 1), (0, 0), (n, 0), (TILE, 0)):
        X.check_export(lib, k, p, 2, lut, recs, kmers, counts, first=first, count=count)
    cuts = [0, TILE + 17, 2 * TILE + 200, n]
    assert b"".join(X.check_export(lib, k, p, 2, lut, recs, kmers, counts, first=a, count=b - a, ds=3) for a, b in zip(cuts, cuts[1:])) == X.run_export(lib, k, p, 2, lut, recs, ds=3)
    slut, srecs, skmers, scounts = X.segmented_body(k, p, 2, K.split(kmers, counts, [5, TILE, TILE, 2 * TILE + 1]))
    assert X.check_export(lib, k, p, 2, slut, srecs, skmers, scounts, n_seg=5) == whole
    for first, count in ((3, 4), (TILE - 1, TILE + 3), (2 * TILE, n - 2 * TILE)):
        X.check_export(lib, k, p, 2, slut, srecs, skmers, scounts, n_seg=5, first=first, count=count)


def test_every_address_residue(lib):
    """d_recs and d_kff at each of the 16 residues of an address: head, aligned pieces and tail of both copies; the tiles start at other residues again (7 bytes in, 8 out)"""
    k, p, cs = 27, 3, 1
    kmers = S.random_kmers(np.random.default_rng(4), k, 2 * TILE + 37)
    lut, recs, kmers, counts = X.ordered_body(k, p, cs, [(kmers, K.edge_counts(cs, len(kmers)))])
    for off in range(16):
        X.check_export(lib, k, p, cs, lut, recs, kmers, counts, in_off=off, out_off=(5 * off + 3) % 16)
        X.check_export(lib, k, p, cs, lut, recs, kmers, counts, in_off=(3 * off + 1) % 16, out_off=off, first=1, ds=2)
    for n in (1, 2, 3):  # fewer bytes than the 15 of a head
        X.check_export(lib, k, p, cs, lut, recs, kmers, counts, in_off=9, out_off=11, first=5, count=n)


@pytest.mark.parametrize("n_seg", [2, 7, 300])
def test_segmented_luts(lib, n_seg):
    """a KMC2 body of n_seg bins, empty ones at the front, in the middle and at the end, prefixes that recur across the bins"""
    k, p, cs = 28, 4, 2
    rng = np.random.default_rng(n_seg)
    sizes = [int(x) for x in rng.integers(0, max(3, 4 * TILE // n_seg), size=n_seg)]
    sizes[0] = sizes[n_seg // 2] = sizes[-1] = 0
    if n_seg == 2:
        sizes = [0, TILE + 50]
    kmers = S.random_kmers(rng, k, sum(sizes))
    sections = K.deal(rng, kmers, K.edge_counts(cs, len(kmers)), sizes)
    slut, srecs, skmers, scounts = X.segmented_body(k, p, cs, sections)
    assert slut.size == (n_seg << (2 * p)) + 1
    X.check_export(lib, k, p, cs, slut, srecs, skmers, scounts, n_seg=n_seg)
    X.check_export(lib, k, p, cs, slut, srecs, skmers, scounts, n_seg=n_seg, first=len(skmers) // 3, count=len(skmers) // 2, ds=3)


# ---- 3: errors and legal edges
def test_errors_and_edges(lib):
    k, p, cs = 27, 3, 1
    lut, recs, kmers, counts = X.ordered_body(k, p, cs, [([1, 2, 1 << 50], [1, 2, 3])])

    def code(**kw):
        a = dict(k=k, p=p, cs=cs, lut=lut, recs=recs)
        a.update(kw)
        with pytest.raises(capi.KmcHipError) as e:
            X.run_export(lib, a.pop("k"), a.pop("p"), a.pop("cs"), a.pop("lut"), a.pop("recs"), **a)
        assert "kmc_hip_db_kff_export_device" in str(e.value)
        return e.value.code

    assert code(ds=0) == X.EINVAL and code(ds=5) == X.EINVAL
    assert code(cs=2, ds=1, recs=np.zeros(3 * 8, dtype=np.uint8)) == X.EINVAL  # data_size below counter_size
    assert code(first=2, count=2) == X.EINVAL and code(first=4, count=0) == X.EINVAL  # first + count > n_recs
    assert code(n_seg=0) == X.EINVAL
    assert code(capacity=3 * 8 - 1) == X.ECAPACITY and code(capacity=0) == X.ECAPACITY
    bad_lut = lut.copy()
    bad_lut[-1] = 4
    assert code(lut=bad_lut) == X.ECORRUPT  # the LUT ends behind the records
    L, C = lib.L, lib.C
    d = lib.malloc(8192)
    try:
        lib.h2d(d, np.zeros(8192, dtype=np.uint8))
        v = capi.DbView(d, 3, d + 4096, p, cs, 1, 10)
        args = [lib.h, 0, k, C.byref(v), 1, 0, 3, 1, d + 1024, 1024]
        assert L.kmc_hip_db_kff_export_device(*args) == 0
        for i in (0, 3, 8):  # ctx, the view, d_kff with records to frame
            assert L.kmc_hip_db_kff_export_device(*[None if j == i else x for j, x in enumerate(args)]) == X.EINVAL, i
        assert b"NULL" in L.kmc_hip_last_error(lib.h)
        assert L.kmc_hip_db_kff_export_device(*[0 if j == 6 else None if j == 8 else x for j, x in enumerate(args)]) == 0  # nothing to frame: d_kff may be NULL
        for field, value in (("d_lut", None), ("d_recs", None), ("counter_size", 0), ("counter_size", 5), ("lut_prefix_len", 0), ("lut_prefix_len", 4), ("lut_prefix_len", 16)):
            w = capi.DbView(d, 3, d + 4096, p, cs, 1, 10)
            setattr(w, field, value)
            assert L.kmc_hip_db_kff_export_device(*[C.byref(w) if j == 3 else x for j, x in enumerate(args)]) == X.EINVAL, (field, value)
        empty = capi.DbView(None, 0, d + 4096, p, cs, 1, 10)  # an empty body: d_recs and d_kff may be NULL
        assert L.kmc_hip_db_kff_export_device(lib.h, 0, k, C.byref(empty), 1, 0, 0, 1, None, 0) == 0
        assert L.kmc_hip_db_kff_export_device(*[0 if j == 2 else x for j, x in enumerate(args)]) == X.EINVAL  # kmer_len 0
        w = capi.DbView(d, 3, d + 4096, 1, cs, 1, 10)
        assert L.kmc_hip_db_kff_export_device(*[225 if j == 2 else C.byref(w) if j == 3 else x for j, x in enumerate(args)]) == X.EINVAL  # kmer_len > 224
        assert L.kmc_hip_db_kff_export_device(*[1 if j == 1 else x for j, x in enumerate(args)]) == X.EINVAL  # no such device
        # a LUT of 2^31 entries and more: k = 31, p = 15 is 2^30 entries a segment — refused on the host before anything is read
        w = capi.DbView(d, 3, d + 4096, 15, cs, 1, 10)
        assert L.kmc_hip_db_kff_export_device(*[31 if j == 2 else C.byref(w) if j == 3 else 2 if j == 4 else x for j, x in enumerate(args)]) == X.EINVAL
        assert b"2^31" in L.kmc_hip_last_error(lib.h)
    finally:
        lib.free(d)
    # the library is usable after every refusal; k = 224 at its widest counter
    X.check_export(lib, k, p, cs, lut, recs, kmers, counts)
    lut2, recs2, km2, cc2 = X.ordered_body(224, 4, 4, [([1 << 447, (1 << 448) - 1], [K.U32, 1 << 24])])
    X.check_export(lib, 224, 4, 4, lut2, recs2, km2, cc2)


def test_the_binding_knows_the_entry_point():
    assert "kmc_hip_db_kff_export_device" in capi.SYMBOLS and hasattr(capi.Context, "db_kff_export_device")
    with open(os.path.join(ROOT, "include", "kmc_hip.h")) as f:
        header = f.read()
    assert "int kmc_hip_db_kff_export_device(" in header and "#define KMC_HIP_ABI_VERSION 4 " in header
    with open(os.path.join(ROOT, "kmc_amd", "csrc", "kmc_hip.hip")) as f:
        assert f.read().count('#include "host_kff_export.hip.h"') == 1


# ---- 4: dbio.write_kff
@pytest.mark.parametrize("name", list(K.FILES))
def test_write_kff_rewrites_the_recorded_files(name, tmp_path):
    """from the parsed header and sections, byte for byte — the 58 sections of kff_k27_multi.kff included; and read_kff reads back what it wrote"""
    f = dbio.read_kff(K.kff_file(name))
    rb = f.rec_bytes
    assert len(f.sections) == K.FILE_SHAPES[name][2]
    out = str(tmp_path / "w.kff")
    dbio.write_kff(out, f.kmer_len, f.counter_size, f.both_strands, f.min_count, f.max_count, [f.raw[o:o + n * rb] for o, n in f.sections])
    assert open(out, "rb").read() == open(K.kff_file(name), "rb").read()
    g = dbio.read_kff(out)
    assert (g.kmer_len, g.counter_size, g.min_count, g.max_count, g.both_strands, g.sections) == (f.kmer_len, f.counter_size, f.min_count, f.max_count, f.both_strands, f.sections)
    assert g.records().tobytes() == f.records().tobytes()
    # a section handed over in pieces is the same section
    dbio.write_kff(out, f.kmer_len, f.counter_size, f.both_strands, f.min_count, f.max_count, [iter([bytes(f.raw[o:o + rb]), f.raw[o + rb:o + n * rb]]) for o, n in f.sections])
    assert open(out, "rb").read() == open(K.kff_file(name), "rb").read()


def test_write_kff_without_records(tmp_path):
    out = str(tmp_path / "w.kff")
    for sections in ([], [b""], [b"", b""]):
        for canonical in (False, True):
            dbio.write_kff(out, 33, 2, canonical, 3, 70000, sections)
            assert open(out, "rb").read() == K.encode_container(33, 2, int(canonical), 3, 70000, sections)
    dbio.write_kff(out, 27, 1, True, 250, 10**9, [b""])
    assert open(out, "rb").read() == golden("kffout_k27_empty")  # what the reference writes for an output without records: one section of 0 records
    assert dbio.read_kff(out).sections == [(dbio.read_kff(out).sections[0][0], 0)] and dbio.read_kff(out).n_recs == 0
    with pytest.raises(ValueError):
        dbio.write_kff(out, 27, 1, True, 1, 10, [b"\0" * 9])  # no whole number of records


# ---- 5: export --sections
def test_export_sections_of_a_kmc2_database(lib, tmp_path):
    src = os.path.join(X.GOLDEN, "setops_k33_raw_a")
    db = dbio.read_database(src)
    assert db.kmc2
    out = str(tmp_path / "s")
    st = tools.export([src, out, "--sections"], ctx=lib)
    f = dbio.read_kff(out + ".kff")
    bins = [(recs, lut) for recs, lut in db.bins if recs.size]
    assert st == dict(n_written=db.total_kmers, n_sections=len(bins)) and len(bins) > 1
    assert (f.kmer_len, f.counter_size, f.min_count, f.max_count, f.both_strands) == (33, db.counter_size, db.min_count, db.max_count, db.both_strands)
    assert [n for _, n in f.sections] == [recs.size // db.rec_bytes for recs, _ in bins]  # one section per bin that is not empty, in file order
    rb = f.rec_bytes
    for (off, n), (recs, lut) in zip(f.sections, bins):
        kmers, counts = S.decode_body(33, db.lut_prefix_len, db.counter_size, np.concatenate([[0], np.cumsum(lut)[:-1]]), recs)
        assert f.raw[off:off + n * rb].tobytes() == K.encode_records(33, db.counter_size, kmers, counts)
    again = str(tmp_path / "again")
    tools.export([out + ".kff", again], ctx=lib)
    assert open(again + ".kff", "rb").read() == golden("kffout_k33_raw")  # ordered and written as one section: the recorded KMC2 line
    before = sorted(os.listdir(tmp_path))
    for argv in ([os.path.join(X.GOLDEN, "setops_k33_a"), out, "--sections"], [K.kff_file("kff_k27_multi"), out, "--sections"],  # a KMC1 input, a KFF input
                 [src, out, "--sections", "-ci2"], [src, out, "-cx9", "--sections"], [src, "--sections", out, "-cs3"], [src, "-ci2", out, "--sections"]):  # bounds
        with pytest.raises(tools.UsageError):
            tools.export(argv, ctx=lib)
    assert sorted(os.listdir(tmp_path)) == before


def test_export_refuses_what_it_does_not_read(tmp_path):
    a = os.path.join(X.GOLDEN, "setops_k27_a")
    for argv in ([], [a], ["-ci2", a], [a, "-q", "o"], [a, "o", "-okff"], [a, "o", "-okmc"], [a, "o", "p"], [a, "o", "-cix"], [str(tmp_path / "none"), "o"]):
        with pytest.raises(tools.UsageError):
            tools.export([x if x != "o" else str(tmp_path / "o") for x in argv])
    assert os.listdir(tmp_path) == []


# ---- 6: count
def test_count_writes_the_recorded_file_and_what_export_makes_of_its_database(lib, tmp_path):
    fq = os.path.join(X.GOLDEN, "count_k27_fq.fq")
    as_kff, as_kmc, again = str(tmp_path / "kff"), str(tmp_path / "kmc"), str(tmp_path / "again")
    res = tools.count(X.COUNT_ARGV + ["-n8", fq, as_kff], ctx=lib, part_bytes=2048, output_format="kff")
    assert res["n_records"] == 2140 and os.listdir(tmp_path) == ["kff.kff"]  # only the KFF file is written
    assert open(as_kff + ".kff", "rb").read() == golden("kffout_k27_multi")  # `kmc -okff` + `kmc_tools transform reduce -okff`
    tools.count(X.COUNT_ARGV + ["-n8", fq, as_kmc], ctx=lib, part_bytes=2048)
    tools.export([as_kmc, again], ctx=lib)
    assert open(again + ".kff", "rb").read() == open(as_kff + ".kff", "rb").read()
    with pytest.raises(ValueError):
        tools.count(X.COUNT_ARGV + [fq, as_kff], ctx=lib, output_format="kmc1")


# ---- 7: the decision next to the feature
def test_the_four_parsers_still_refuse_okff(tmp_path):
    """-okff in simple, transform, complex and count is left for a follow-up: KFF output arrives through `export` and count's output_format"""
    a, out = S.golden_path(27, "a"), str(tmp_path / "o")
    with pytest.raises(tools.UsageError) as e:
        tools.parse_simple([a, a, "union", out, "-okff"])
    assert "KFF output is not written" in str(e.value)
    with pytest.raises(tools.UsageError) as e:
        tools.parse_transform([a, "reduce", out, "-okff"])
    assert "KFF output is not written" in str(e.value)
    with pytest.raises(tools.UsageError):
        tools.parse_complex(f"INPUT:\na = {a}\nOUTPUT:\n{out} = a\nOUTPUT_PARAMS:\n-okff\n")
    with pytest.raises(tools.UsageError) as e:
        tools.parse_count(["-k27", "-okff", "in.fq", out])
    assert "KFF output" in str(e.value)
    assert os.listdir(tmp_path) == []
