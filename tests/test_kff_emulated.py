"""CPU: KFF files read as database bodies — kmc_hip_kff_import_device in the PRODUCT'S host library compiled over the emulated HIP runtime (tests/emu.py build_hostlib,
small geometry; $KMC_HIP_KFF_IPT = 1: k_kff_repack tiles of 256 records), kmc_amd/dbio.read_kff, and the KFF inputs of `python -m kmc_amd.tools` over it.

The oracle is the restatement of container and record in tests/kff_cases.py (Python ints and bytes). It is held to the files the reference itself wrote
(tests/golden/kff_*.kff, made by tests/make_kff_golden.py), byte for byte, before anything relies on it. The -m gpu file runs the same cases on the device."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import emu
import kff_cases as K
import setops_cases as S
import transform_cases as T
from kmc_amd import capi, dbio, tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = K.tile_records(27, 3, 1, ipt=1)
DUMP_TILE = 200
ENV = {"KMC_HIP_KFF_IPT": "1", "KMC_HIP_DUMP_TILE": str(DUMP_TILE)}


@pytest.fixture(scope="module")
def lib():
    os.environ.update(ENV)
    c = K.KffContext(emu.build_hostlib("small"))
    yield c
    c.close()
    for key in ENV:
        del os.environ[key]


@pytest.fixture(scope="module")
def files():
    """the recorded KFF files, read once: name -> (bytes, header, [(kmers, counts)] per section)"""
    out = {}
    for name in K.FILES:
        raw = open(K.kff_file(name), "rb").read()
        out[name] = (raw, *K.file_sections(raw))
    return out


# ---- 1: the restatement is the reference
@pytest.mark.parametrize("name", list(K.FILES))
def test_the_restatement_writes_the_recorded_files(files, name):
    raw, h, sections = files[name]
    assert (h["k"], h["cs"], len(sections), sum(len(ks) for ks, _ in sections)) == K.FILE_SHAPES[name]
    assert (h["encoding"], h["all_unique"], h["max"], h["ordered"]) == (0b00011011, 1, 1, 1)
    assert K.encode_container(h["k"], h["cs"], h["canonical"], h["min_count"], h["max_count"], [K.encode_records(h["k"], h["cs"], ks, cc) for ks, cc in sections]) == raw
    assert all(ks == sorted(set(ks)) and max(ks) < 1 << (2 * h["k"]) for ks, _ in sections)


def test_the_recorded_files_are_the_twins_of_the_kmc_fixtures(files):
    for k in (27, 33, 55):
        db = dbio.read_database(S.golden_path(k, "a"))
        assert files[f"kff_k{k}_a"][2] == [S.decode_body(k, db.lut_prefix_len, db.counter_size, db.lut, db.recs)]
    assert files["kff_k27_a_cs2"][2] == files["kff_k27_a"][2]
    flat = [x for ks, _ in files["kff_k27_multi"][2] for x in ks]
    assert flat != sorted(flat) and len(set(flat)) == len(flat)


# ---- 2: dbio.read_kff
@pytest.mark.parametrize("name", list(K.FILES))
def test_read_kff_on_the_recorded_files(files, name):
    raw, h, sections = files[name]
    f = dbio.read_kff(K.kff_file(name))
    assert (f.kmer_len, f.counter_size, f.min_count, f.max_count, f.both_strands, f.total_kmers) == (h["k"], h["cs"], h["min_count"], h["max_count"], bool(h["canonical"]), 0)
    assert f.sections == h["sections"] and f.n_recs == K.FILE_SHAPES[name][3]
    assert f.records().tobytes() == b"".join(K.encode_records(h["k"], h["cs"], ks, cc) for ks, cc in sections)
    assert dbio.read_kff(K.kff_file(name)[:-4]).sections == f.sections  # the name + '.kff'
    with pytest.raises(dbio.DbFormatError):  # read_database keeps refusing KFF files
        dbio.read_database(K.kff_file(name))


def test_read_kff_without_a_footer_and_with_the_index_first(files, tmp_path):
    """no footer: the index is the first section; min_count and max_count take their defaults"""
    raw, h, sections = files["kff_k27_multi"]
    first_r, rb = h["sections"][0][0] - 9, 8
    body = [raw[12:first_r]] + [raw[o - 9:o + n * rb] for o, n in h["sections"]]
    idx_end = 12 + 1 + 8 + 9 * len(body) + 8
    index, pos = b"i" + len(body).to_bytes(8, "big"), idx_end
    for i, part in enumerate(body):
        index += (b"r" if i else b"v") + (pos - idx_end).to_bytes(8, "big")
        pos += len(part)
    p = tmp_path / "nofooter.kff"
    p.write_bytes(raw[:12] + index + (0).to_bytes(8, "big") + b"".join(body) + b"KFF")
    f = dbio.read_kff(str(p))
    assert (f.min_count, f.max_count, f.kmer_len, f.n_recs, len(f.sections)) == (1, 0xFFFFFFFF, 27, 2140, 58)
    assert f.records().tobytes() == dbio.read_kff(K.kff_file("kff_k27_multi")).records().tobytes()


def _patched(raw, at, new):
    return raw[:at] + new + raw[at + len(new):]


def test_read_kff_names_what_it_refuses(files, tmp_path):
    raw, h, sections = files["kff_k27_multi"]
    v = raw.index(b"v", 12)
    var = lambda name: raw.index(name.encode() + b"\0", v) + len(name) + 1  # noqa: E731
    first_r = h["sections"][0][0] - 9
    index_at = raw.rindex(b"first_index\0") + 12
    index_pos = int.from_bytes(raw[index_at:index_at + 8], "big")
    two_k = K.encode_container(27, 1, 1, 1, 10**9, [K.encode_records(27, 1, [5], [1])])
    second = K.encode_container(28, 1, 1, 1, 10**9, [K.encode_records(28, 1, [5], [1])])
    cases = {
        "all_unique": (_patched(raw, 6, b"\0"), "all_unique"),
        "encoding": (_patched(raw, 5, b"\x2d"), "encoding"),
        "ordered": (_patched(raw, var("ordered"), (0).to_bytes(8, "big")), "ordered"),
        "data_size_0": (_patched(raw, var("data_size"), (0).to_bytes(8, "big")), "data_size"),
        "data_size_5": (_patched(raw, var("data_size"), (5).to_bytes(8, "big")), "data_size"),
        "max_2": (_patched(raw, var("max"), (2).to_bytes(8, "big")), "max"),
        "k_225": (_patched(raw, var("k"), (225).to_bytes(8, "big")), "k ="),
        "minimizer_section": (_patched(_patched(raw, first_r, b"m"), index_pos + 9 + 9, b"m"), "minimizer"),
        "index_inconsistent": (_patched(raw, first_r, b"x"), "inconsistent"),
        "missing_index": (_patched(raw, index_pos, b"x"), "missing index"),
        "no_index": (_patched(raw, index_at - 12, b"xirst_index"), "no index"),
        "no_end_marker": (raw[:-3] + b"KFX", "marker at the end"),
        "truncated": (raw[:len(raw) // 2], "marker at the end"),
        "truncated_with_marker": (raw[:12] + b"KFF", "no index"),
        "section_behind_the_end": (_patched(raw, first_r + 1, (1 << 40).to_bytes(8, "big")), "truncated"),
        "no_start_marker": (b"KFG" + raw[3:], "marker at the beginning"),
    }
    # several k: a second scope spliced in behind the first file's sections is beyond a byte patch; two files' scopes are joined through the restatement's pieces instead
    index_of = lambda f: int.from_bytes(f[f.rindex(b"first_index\0") + 12:f.rindex(b"first_index\0") + 20], "big")  # noqa: E731

    def join(first, other):
        """the scope of `other` (variables and its raw section) behind the sections of `first`, one index over both, a footer of first_index alone"""
        a_end, b_end, b_v = index_of(first), index_of(other), 12
        a_r, b_r = K.decode_container(first)["sections"][0][0] - 9, K.decode_container(other)["sections"][0][0] - 9
        both = bytearray(first[:a_end] + other[b_v:b_end])
        idx_pos = len(both)
        entries = [(b"v", 12), (b"r", a_r), (b"v", a_end), (b"r", a_end + b_r - b_v)]
        idx_end = idx_pos + 9 + 9 * len(entries) + 8
        both += b"i" + len(entries).to_bytes(8, "big") + b"".join(t + ((pos - idx_end) & ((1 << 64) - 1)).to_bytes(8, "big") for t, pos in entries) + (0).to_bytes(8, "big")
        return both, b"v" + (2).to_bytes(8, "big") + b"first_index\0" + idx_pos.to_bytes(8, "big") + b"footer_size\0" + (1 + 8 + 20 + 20).to_bytes(8, "big")

    joined, foot = join(two_k, second)
    cases["several_k"] = (bytes(joined) + foot + b"KFF", "several k")
    wide, wide_foot = join(two_k, K.encode_container(27, 2, 1, 1, 10**9, [K.encode_records(27, 2, [5], [1])]))  # the same k, scopes of data_size 1 and 2
    cases["scopes_differ_in_data_size"] = (bytes(wide) + wide_foot + b"KFF", "different data_size")
    for name, (data, word) in cases.items():
        p = tmp_path / (name + ".kff")
        p.write_bytes(data)
        with pytest.raises(dbio.DbFormatError) as e:
            dbio.read_kff(str(p))
        assert "KFF" in str(e.value) and word in str(e.value), (name, str(e.value))
    # the joined file is well formed apart from its two k: with one k it is read, two scopes flattened
    same_k = bytes(joined).replace((28).to_bytes(8, "big") + b"max\0", (27).to_bytes(8, "big") + b"max\0") + foot + b"KFF"
    p = tmp_path / "two_scopes.kff"
    p.write_bytes(same_k)
    f = dbio.read_kff(str(p))
    assert (f.kmer_len, [n for _, n in f.sections], f.min_count, f.max_count) == (27, [1, 1], 1, 0xFFFFFFFF)


# ---- 3: the entry on planted sections
@pytest.mark.parametrize("k,p", K.WIDTHS, ids=K.WIDTH_IDS)
def test_planted_sections(lib, k, p):
    """every case with ordered = 0 (k_kff_repack under the segmented LUT) and ordered = 1 (k_kff_repack alone, or unpack, sort, verify and pack)"""
    cases = K.planted_cases(k, p, TILE)
    assert len(cases) >= 20
    for name, cs, sections in cases:
        for ordered in (False, True):
            try:
                K.check_import(lib, k, cs, p, sections, ordered)
            except AssertionError as e:
                raise AssertionError(f"{name}, ordered {ordered}: {e}")


def test_every_address_residue(lib):
    """d_kff and d_out at each of the 16 residues of an address: head, aligned pieces and tail of both copies; tiles start at other residues again (rb_in 8, rb_out 7)"""
    k, p, cs = 27, 3, 1
    rng = np.random.default_rng(4)
    kmers = S.random_kmers(rng, k, 2 * TILE + 37)
    sections = K.split(kmers, K.edge_counts(cs, len(kmers)), [TILE + 3])
    for off in range(16):
        K.check_import(lib, k, cs, p, sections, False, in_off=off, out_off=(5 * off + 3) % 16)
        K.check_import(lib, k, cs, p, sections, True, in_off=(3 * off + 1) % 16, out_off=off)
    for n in (1, 2, 3):  # fewer bytes than the 15 of a head
        K.check_import(lib, k, cs, p, [(kmers[:n], [9] * n)], False, in_off=9, out_off=11)


def test_the_unordered_body_through_dump_and_histogram(lib):
    """ordered = 0 is what `transform` histogram and dump without -s read: the imported body and its segmented LUT through the existing entries, in file order"""
    for k, p in ((27, 3), (33, 5), (65, 9)):
        segments, kmers, counts = T.segmented_case(k, p, TILE)
        data = b"".join(K.encode_records(k, 1, ks, cc) for ks, cc in segments)
        lut, recs, body = K.run_import(lib, k, 1, p, data, [len(ks) for ks, _ in segments], False, keep=True)
        try:
            assert T.decode_segmented(k, p, 1, lut, recs) == (kmers, counts) and kmers != sorted(kmers)
            T.check_dump(lib, body, kmers, counts, (1, S.U32), 1, S.U32, S.U32)
            T.check_dump(lib, body, kmers, counts, (5, 150), 20, 120, 99)
            T.check_histogram(lib, body, counts, (5, 150), 20, 120)
        finally:
            body.free()


# ---- 4: corruption
@pytest.mark.parametrize("k,p", [(27, 3), (33, 5), (64, 4), (129, 5)])
def test_corrupt_sections_are_named(lib, k, p):
    for name, secs, bad0, bad1, where in K.corruption_cases(k, p, TILE):
        rb = (k + 3) // 4 + 1
        sec_n = [len(s) // rb for s in secs]
        for ordered, bad in ((False, bad0), (True, bad1)):
            if not bad:
                K.run_import(lib, k, 1, p, b"".join(secs), sec_n, ordered)
                continue
            with pytest.raises(capi.KmcHipError) as e:
                K.run_import(lib, k, 1, p, b"".join(secs), sec_n, ordered)
            assert e.value.code == K.ECORRUPT and "KFF" in str(e.value), (name, ordered, str(e.value))
            if where is not None:
                sec = 0 if where < sec_n[0] else 1
                assert f"KFF record {where} (record {where - sec * sec_n[0]} of section {sec})" in str(e.value), (name, ordered, str(e.value))
            else:
                assert "two KFF sections" in str(e.value)
    # the library is usable after every refusal
    K.check_import(lib, k, 1, p, [([1, 2, 3], [4, 5, 6])], True)


def test_a_prefix_beyond_the_lut_is_corrupt_not_written(lib):
    """k = 28, p = 4: one prefix byte and no padding, so every byte value is a valid prefix; k = 27, p = 3: the prefix byte's top two bits are the padding"""
    data = K.encode_records(27, 1, [3, 1 << 53], [1, 1])
    K.run_import(lib, 27, 1, 3, data, [2], False)
    with pytest.raises(capi.KmcHipError) as e:
        K.run_import(lib, 27, 1, 3, data[:8] + bytes([0x40]) + data[9:], [2], False)
    assert e.value.code == K.ECORRUPT and "record 1 of section 0" in str(e.value)


# ---- 5: errors and legal edges
def test_errors_and_edges(lib):
    k, p, cs = 27, 3, 1
    data = K.encode_records(k, cs, [1, 2, 3], [1, 2, 3])

    def code(**kw):
        a = dict(k=k, cs=cs, p=p, data=data, sec_n=[3], ordered=False)
        a.update(kw)
        with pytest.raises(capi.KmcHipError) as e:
            K.run_import(lib, a.pop("k"), a.pop("cs"), a.pop("p"), a.pop("data"), a.pop("sec_n"), a.pop("ordered"), **a)
        assert "kmc_hip_kff_import_device" in str(e.value)
        return e.value.code

    assert code(cs=0) == K.EINVAL and code(cs=5) == K.EINVAL
    assert code(k=225, p=1) == K.EINVAL and code(k=228, p=4) == K.EINVAL
    assert code(p=4) == K.EINVAL and code(p=0) == K.EINVAL  # (27 - 4) % 4 != 0
    assert code(capacity=3 * 7 - 1) == K.ECAPACITY and code(capacity=3 * 7 - 1, ordered=True) == K.ECAPACITY
    L, C = lib.L, lib.C
    d = lib.malloc(4096)
    try:
        n_out, sec = C.c_uint64(), (C.c_uint64 * 1)(0)
        args = [lib.h, 0, k, cs, d, sec, 1, 1, p, d, 1024, d, C.byref(n_out)]
        for i in (5, 9, 11, 12):
            assert L.kmc_hip_kff_import_device(*[None if j == i else x for j, x in enumerate(args)]) == K.EINVAL and b"NULL" in L.kmc_hip_last_error(lib.h)
        assert L.kmc_hip_kff_import_device(*[None if j == 4 else x for j, x in enumerate(args)]) == 0  # no record: d_kff may be NULL
        sec[0] = 1
        assert L.kmc_hip_kff_import_device(*[None if j == 4 else x for j, x in enumerate(args)]) == K.EINVAL
        assert L.kmc_hip_kff_import_device(*[2 if j == 7 else x for j, x in enumerate(args)]) == K.EINVAL  # ordered
        assert L.kmc_hip_kff_import_device(*[0 if j == 2 else x for j, x in enumerate(args)]) == K.EINVAL  # kmer_len 0
        # refused on the host before anything is allocated or read: a segmented LUT of 2^31 entries and more (k = 31, p = 15: 2^30 entries per section), and more
        # records than a byte offset reaches (one section, then two whose sum is beyond it)
        many = (C.c_uint64 * 2)(0, 0)
        lut_args = [lib.h, 0, 31, cs, d, many, 2, 0, 15, d, 1024, d, C.byref(n_out)]
        assert L.kmc_hip_kff_import_device(*lut_args) == K.EINVAL and b"2^31" in L.kmc_hip_last_error(lib.h)
        for big in ((1 << 60, 0), ((1 << 52) + 1, (1 << 52) + 1)):  # k = 27, one counter byte: 2^53 records of 8 bytes are the limit
            many[0], many[1] = big
            assert L.kmc_hip_kff_import_device(*[many if j == 5 else 2 if j == 6 else x for j, x in enumerate(args)]) == K.EINVAL and b"byte offset" in L.kmc_hip_last_error(lib.h)
    finally:
        lib.free(d)
    # legal: no section, empty sections only (covered per width by the planted cases); k = 224 at its widest counter
    K.check_import(lib, 224, 4, 4, [([1 << 447, (1 << 448) - 1], [K.U32, 1 << 24])], True)


def test_the_binding_knows_the_entry_point():
    assert "kmc_hip_kff_import_device" in capi.SYMBOLS and hasattr(capi.Context, "kff_import_device")
    with open(os.path.join(ROOT, "include", "kmc_hip.h")) as f:
        assert "int kmc_hip_kff_import_device(" in f.read()
    with open(os.path.join(ROOT, "kmc_amd", "csrc", "kmc_hip.hip")) as f:
        text = f.read()
    assert text.count('#include "host_kff.hip.h"') == 1 and text.count('#include "kff_db.hip.h"') == 1


# ---- 6: the command line, a process of its own per recorded line
@pytest.mark.parametrize("line", K.LINES, ids=K.LINE_IDS)
def test_the_command_line_writes_the_recorded_files(line, tmp_path):
    argv, outs = K.command_line(line, str(tmp_path))
    r = subprocess.run([sys.executable, "-m", "kmc_amd.tools", *argv], cwd=ROOT, capture_output=True, text=True, timeout=1200,
                       env=dict(os.environ, KMC_HIP_LIB=emu.build_hostlib("small"), KMC_HIP_DUMP_PART_MB="0.05", **ENV))
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    for i, (path, kind) in enumerate(zip(outs, line[3])):
        assert K.output_bytes(path, kind) == K.read_golden(line, i, kind), (line[0], i)


def test_the_twin_lines_hold_the_twin_records():
    """the lines over KFF twins of the KMC fixtures equal the KMC runs already recorded, apart from lut_prefix_len and the header"""
    by = {ln[0]: ln for ln in K.LINES}
    for name, twin in K.TWINS.items():
        got, want = dbio.read_database(K.golden_out(by[name], 0)), dbio.read_database(os.path.join(K.GOLDEN, twin))
        assert S.decode_body(got.kmer_len, got.lut_prefix_len, got.counter_size, got.lut, got.recs) == S.decode_body(want.kmer_len, want.lut_prefix_len, want.counter_size, want.lut, want.recs)
    assert dbio.read_database(K.golden_out(by["k33_reduce"], 0)).lut_prefix_len == 1  # total_kmers stays 0: the smallest valid prefix length
    with gzip.open(os.path.join(K.GOLDEN, "filter_out_k27_normal_defaults.gz"), "rb") as f:  # filter over the KFF twin: the reads the KMC database keeps
        assert f.read() == K.read_golden(by["k27_filter"], 0, "fq")[0]
    # no KMC run of the complex line's expression is recorded (the complex_* goldens use other expressions and cutoffs): its records are held to the set-operation
    # restatement instead, which tests/golden/setops_* pin to kmc_tools — `a + b` with a -ci2 and the output's -cx30 is a union with counter mode sum
    a, b, got = dbio.read_database(S.golden_path(27, "a")), dbio.read_database(S.golden_path(27, "b")), dbio.read_database(K.golden_out(by["k27_complex"], 0))
    body = lambda d: S.decode_body(d.kmer_len, d.lut_prefix_len, d.counter_size, d.lut, d.recs)  # noqa: E731
    wk, wc, _ = S.restate(body(a), body(b), (2, a.max_count), (b.min_count, b.max_count), "union", "sum", min(2, b.min_count), 30, 255)
    assert body(got) == (wk, wc) and (got.min_count, got.max_count, got.counter_size) == (min(2, b.min_count), 30, 1) and len(wk) > 1000


def test_kff_output_stays_refused(tmp_path):
    a, out = K.kff_file("kff_k27_a"), str(tmp_path / "o")
    for fn, argv in ((tools.transform, [a, "reduce", out, "-okff"]), (tools.simple, [a, a, "union", out, "-okff"])):
        with pytest.raises(tools.UsageError) as e:
            fn(argv)
        assert "KFF output is not written" in str(e.value)
    assert os.listdir(tmp_path) == []
