"""CPU: BGZF input — kmc_hip_bgzf_scan, kmc_hip_bgzf_inflate / _inflate_device (k_bgzf_inflate), kmc_hip_bam_whole_records in the PRODUCT'S host library compiled over
the emulated HIP runtime (tests/emu.py build_hostlib, small geometry), readsio's device chunk source, and `count`, `count-small` and `filter` over it.

The oracle of the kernel is zlib (tests/bgzf_cases.py); the expected databases are reference outputs recorded under tests/golden (bgzf_* by tests/make_bgzf_golden.py,
count_* and filter_* from before). The -m gpu file runs the same cases on the device. Without the feature every test here fails: the symbols, capi.bgzf_* and
input_format do not exist."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bgzf_cases as B
import count_cases as CC
import emu
import query_cases as Q
from kmc_amd import capi, readsio, synth, tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    c = B.make_context(emu.build_hostlib("small"))
    yield c
    c.close()


# ---- 1: the kernel against zlib
def test_block_types_match_geometry_and_sizes(lib):
    B.check_kernel_cases(lib)


def test_many_members_odd_offsets_and_an_odd_source_address(lib):
    B.check_placements(lib)


def test_every_corruption_is_refused_as_zlib_refuses_it(lib):
    assert B.check_corruptions(lib) == B.CORRUPTION_REASONS


def test_the_same_on_device_pointers_leaves_every_other_byte_alone(lib):
    B.check_kernel_cases(lib, device=True)
    B.check_corruptions(lib, device=True)


def test_the_largest_member_is_what_the_cases_say():
    """level-6 random data of 65536 bytes does not fit a member, compressible data does"""
    assert len(B.deflate(B.noise(1, 65536), 6)) + 26 > 0x10000 and len(B.size_members()["level6_65536"]) < 0x10000
    table = B.py_table(B.size_members()["level6_65536"] + B.size_members()["stored_65280"])
    assert [int(x) for x in table["isize"]] == [65536, 65280]


def test_two_bad_members_name_the_first(lib):
    c = B.corruptions()
    blob = B.GOOD[0] + c["block_type_3"][0][len(B.GOOD[0]) + len(B.GOOD[1]):-len(B.GOOD[2]) - 28] + B.GOOD[1] + B.member(B.text(1, 100), 6)[:-8] + struct.pack("<II", 1, 100) + B.GOOD[2]
    B.check(lib, blob, expect_bad=[1, 3])


# ---- 2: the scan
def test_scan_header_variants_and_the_carry(lib):
    blob = B.header_variants()
    table = B.py_table(blob)
    members, used, out = capi.bgzf_scan(blob, L=lib.L)
    assert members.tobytes() == table.tobytes() and used == len(blob) and out == 650 and len(members) == 4
    B.check(lib, blob, expect_bad=[])
    ends = np.cumsum([int(m["comp_len"]) for m in table])  # not the members' ends: any cut inside the blob
    second = int(table["src_off"][1])
    for cut in (0, 1, 3, 4, 11, 12, 17, 18, second - 1, second, second + 5, len(blob) - 28, len(blob) - 27, len(blob) - 1):
        m, u, o = capi.bgzf_scan(blob[:cut], L=lib.L)
        whole = [i for i in range(4) if (int(table["src_off"][i + 1]) if i < 3 else len(blob)) - (0 if i < 3 else 0) <= cut] if cut < len(blob) else [0, 1, 2, 3]
        n = sum(1 for i in range(4) if int(table["src_off"][i]) + int(table["comp_len"][i]) + 8 <= cut)
        assert len(m) == n and m.tobytes() == table[:n].tobytes() and u == (int(table["src_off"][n - 1]) + int(table["comp_len"][n - 1]) + 8 if n else 0), cut
    # the limits: output bytes and table entries
    m, u, o = capi.bgzf_scan(blob, 600, L=lib.L)
    assert len(m) == 2 and o == 600
    m, u, o = capi.bgzf_scan(blob, cap=3, L=lib.L)
    assert len(m) == 3 and o == 650 and u == len(blob) - 28


def test_scan_refuses_what_is_not_bgzf(lib):
    good = B.GOOD[0]

    def refused(blob, word, at):
        with pytest.raises(capi.KmcHipError) as e:
            capi.bgzf_scan(blob, L=lib.L)
        assert e.value.code == -4 and word in str(e.value) and str(e.value).endswith(f"at byte {at}"), str(e.value)

    import gzip
    refused(good + gzip.compress(b"plain gzip", mtime=0), "no BGZF member", len(good))
    refused(good + b"\x1f\x8b\x08\x04" + good[4:10] + struct.pack("<H", 6) + b"XY\2\0ab" + b"\0" * 20, "BC subfield", len(good))
    big = bytearray(good)
    big[-4:] = struct.pack("<I", 65537)
    refused(good + bytes(big), "ISIZE above 65536", len(good))
    small = bytearray(good)
    small[16:18] = struct.pack("<H", 24)  # BSIZE 25: header 18 + trailer 8 do not fit
    refused(bytes(small) + b"\0" * 40, "BSIZE too small", 0)
    refused(b"@r0\nACGT\n+\nIIII\n", "no BGZF member", 0)
    with pytest.raises(capi.KmcHipError):
        capi.bgzf_scan(good, cap=1, L=lib.L) and lib.L.kmc_hip_bgzf_scan(None, 5, 0, None, 0, None, None, None) and lib._chk(-1)


def test_entry_arguments(lib):
    blob = B.GOOD[0] + B.GOOD[1]
    table = B.py_table(blob)
    total = int(table["isize"].sum())

    def code(**kw):
        a = dict(src=blob, members=table, cap=None)
        a.update(kw)
        with pytest.raises(capi.KmcHipError) as e:
            capi.bgzf_inflate(lib, a["src"], a["members"], a["cap"], slot=a.get("slot", 0))
        return e.value.code

    assert code(cap=total - 1) == -5 and code(slot=99) == -1 and code(slot=-1) == -1
    assert code(src=blob[:-9]) == -1  # the last member ends behind the source bytes
    t = table.copy()
    t["dst_off"][1] -= 1
    assert code(members=t) == -1  # outputs that overlap
    t = table.copy()
    t["isize"][1] = 65537
    assert code(members=t) == -1
    assert capi.bgzf_inflate(lib, b"", np.zeros(0, dtype=capi.BGZF_MEMBER)).size == 0
    assert capi.bgzf_inflate(lib, blob, table, slot=3).tobytes() == b"".join(B.oracle(blob, table))
    assert lib.L.kmc_hip_split_covers(capi.SPLIT_COVERS_BGZF) == 1 and capi.SPLIT_COVERS_BGZF == 0x10B and lib.L.kmc_hip_split_covers(0x10A) == 0 and lib.L.kmc_hip_split_covers(0x10C) == 0
    with open(os.path.join(ROOT, "include", "kmc_hip.h")) as f:
        header = f.read()
    assert all(f"int {s}(" in header for s in capi.SYMBOLS if "bgzf" in s or "bam_whole" in s) and "#define KMC_HIP_ABI_VERSION 4 " in header
    with open(os.path.join(ROOT, "kmc_amd", "csrc", "kmc_hip.hip")) as f:
        text = f.read()
    assert text.count('#include "host_bgzf.hip.h"') == 1 and text.count('#include "bgzf.hip.h"') == 1


def test_bam_whole_records(lib):
    recs = [synth.bam_record("ACGT" * n, name=b"r%d" % n) for n in (1, 5, 0, 30)]
    whole = b"".join(recs)
    for cut in (0, 3, 4, len(recs[0]) - 1, len(recs[0]), len(recs[0]) + 4, len(whole) - 1, len(whole)):
        n_bytes, n = capi.bam_whole_records(whole[:cut], L=lib.L)
        want = max(i for i in range(5) if len(b"".join(recs[:i])) <= cut)
        assert (n_bytes, n) == (len(b"".join(recs[:want])), want), cut
    for bad in (31, 0, -1, -2**31):
        with pytest.raises(capi.KmcHipError) as e:
            capi.bam_whole_records(recs[0] + struct.pack("<i", bad) + b"\0" * 40, L=lib.L)
        assert e.value.code == -4 and "record 1" in str(e.value) and f"at byte {len(recs[0])}" in str(e.value)


# ---- 3: readsio
def test_chunks_carry_a_cut_member_at_a_tiny_piece_size(lib, tmp_path, monkeypatch):
    data = CC.CASES["k27_fq"][2][0][2]
    path = str(tmp_path / "reads.fq.gz")
    with open(path, "wb") as f:
        f.write(B.bgzipped(data, 700))
    assert readsio.is_bgzf(path) and not readsio.is_bgzf(CC.golden_input_paths("k27_gz")[0]) and not readsio.is_bgzf(CC.golden_input_paths("k27_fq")[0])
    for piece in (1, 29, 333, 1 << 20):
        monkeypatch.setenv("KMC_HIP_BGZF_PIECE", str(piece))
        got = list(readsio.bgzf_chunks(path, lib, 2048))
        assert b"".join(c.tobytes() for c in got) == data and (piece > 333 or len(got) > 5), piece
    monkeypatch.delenv("KMC_HIP_BGZF_PIECE")
    parts = list(readsio.parts(path, True, 2048, lib))
    assert len(parts) > 3 and b"".join(p.tobytes() for p in parts) == data and all(p[0] == ord("@") and p[-1] == 10 for p in parts)
    monkeypatch.setenv("KMC_HIP_BGZF", "0")
    assert not readsio.on_device(path, lib) and b"".join(p.tobytes() for p in readsio.parts(path, True, 2048, lib)) == data


# ---- 4: count
@pytest.mark.parametrize("name", ["k27_fq", "k27_fa_b", "k27_fm"])
def test_count_on_a_bgzipped_twin_writes_the_recorded_database(lib, name, tmp_path, monkeypatch):
    fname, _, data = CC.CASES[name][2][0]
    path = str(tmp_path / (fname + ".gz"))
    with open(path, "wb") as f:
        f.write(B.bgzipped(data, 900))
    calls = []
    monkeypatch.setattr(capi, "bgzf_inflate", lambda *a, _f=capi.bgzf_inflate, **kw: calls.append(1) or _f(*a, **kw))
    for env, on_device in ((None, True), ("0", False)):
        if env is not None:
            monkeypatch.setenv("KMC_HIP_BGZF", env)
        out = str(tmp_path / ("out" + str(env)))
        del calls[:]
        tools.count(CC.CASES[name][0] + ["-n8", path, out], ctx=lib, part_bytes=2048)
        assert CC.database_bytes(out) == CC.database_bytes(CC.golden_out(name)) and bool(calls) == on_device


@pytest.mark.parametrize("name", ["k27", "k27_b", "k27_hc"])
def test_count_bam_writes_what_the_reference_wrote(lib, name, tmp_path):
    flags, (k, ci, cx, cs, both, hc), reads = B.BAM_CASES[name]
    with open(B.bam_path(name), "rb") as f:
        blob = f.read()
    table = B.py_table(blob)
    header = 12 + len(B.BAM_TEXT) + sum(9 + len(n) for n, _ in B.BAM_REFS)
    assert int(np.searchsorted(np.cumsum(table["isize"]), header)) == 2 and len(table) > 15  # the header ends in the third member
    out = str(tmp_path / "out")
    res = tools.count(flags + ["-n8", B.bam_path(name), out], ctx=lib, part_bytes=2048, input_format="bam")
    assert B.database_bytes(out) == B.database_bytes(B.bam_out(name))
    assert res["totals"]["n_reads"] == synth.bam_reads_as_getseq(reads, both)[1] and res["n_parts"] > 10
    fa = str(tmp_path / "same.fa")
    with open(fa, "wb") as f:
        f.write(B.bam_as_fasta(name))
    tools.count(flags + ["-fa", "-n8", fa, str(tmp_path / "fa")], ctx=lib, part_bytes=2048)
    assert B.database_bytes(str(tmp_path / "fa")) == B.database_bytes(out)


def test_count_bam_with_a_list_the_stage0_map_and_the_host_inflate(lib, tmp_path, monkeypatch):
    lst = str(tmp_path / "in.lst")
    with open(lst, "w") as f:
        f.write(B.bam_path("k27") + "\n" + B.bam_path("k27_hc") + "\n")
    fa = str(tmp_path / "same.fa")
    with open(fa, "wb") as f:
        f.write(B.bam_as_fasta("k27") + B.bam_as_fasta("k27_hc"))
    tools.count(["-k27", "-fa", "-n8", fa, str(tmp_path / "fa")], ctx=lib, part_bytes=4096)
    res = tools.count(["-k27", "-n%d" % tools.COUNT_MAP_MIN_BINS, "@" + lst, str(tmp_path / "a")], ctx=lib, part_bytes=4096, input_format="bam", signature_map="stats")
    assert res["map"] == "stats" and B.database_bytes(str(tmp_path / "a")) == B.database_bytes(str(tmp_path / "fa"))
    monkeypatch.setenv("KMC_HIP_BGZF", "0")
    tools.count(["-k27", "-n8", "@" + lst, str(tmp_path / "b")], ctx=lib, part_bytes=4096, input_format="bam")
    assert B.database_bytes(str(tmp_path / "b")) == B.database_bytes(str(tmp_path / "fa"))


def test_count_small_bam(lib, tmp_path):
    out = str(tmp_path / "out")
    res = tools.count_small(B.BAM_CASES["k9"][0] + [B.bam_path("k9"), out], ctx=lib, part_bytes=2048, input_format="bam")
    assert B.database_bytes(out) == B.database_bytes(B.bam_out("k9")) and res["n_parts"] > 10


def test_filter_on_a_bgzipped_reads_file(lib, tmp_path, monkeypatch):
    monkeypatch.setenv("KMC_HIP_QUERY_IPT", "1")
    monkeypatch.setenv("KMC_HIP_FILTER_PART_MB", "0.02")
    line = Q.LINES[0]
    packed = os.path.join(Q.GOLDEN, Q.FQ)
    import gzip
    twin = str(tmp_path / Q.FQ)
    with open(twin, "wb") as f:
        f.write(B.bgzipped(gzip.open(packed, "rb").read(), 5000))
    args = Q.command_line(line, str(tmp_path / "out"))
    args[args.index(packed)] = twin
    st = tools.filter_reads(args[1:], ctx=lib)
    assert open(str(tmp_path / "out"), "rb").read() == Q.golden_out(line[0]) and st["n_reads"] == 200
    plain = Q.command_line(line, str(tmp_path / "plain"))
    same = ("n_reads", "n_written", "n_valid_windows", "n_found", "n_cut")  # n_invalid_windows counts the separators between the reads of a part: it follows the cut into parts
    twin_st = tools.filter_reads(plain[1:], ctx=lib)
    assert [twin_st[x] for x in same] == [st[x] for x in same] and open(str(tmp_path / "plain"), "rb").read() == Q.golden_out(line[0])


# ---- 5: what is refused
def test_broken_bgzf_and_bam_are_usage_errors(lib, tmp_path):
    data = CC.CASES["k27_fq"][2][0][2]
    good = B.bgzipped(data, 900)
    table = B.py_table(good)
    second = int(table["src_off"][1]) - 18

    def refused(blob, *words, bam=False, name="x.fq.gz"):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(blob)
        with pytest.raises(tools.UsageError) as e:
            tools.count(["-k27", "-n8", path, str(tmp_path / "o")], ctx=lib, part_bytes=2048, input_format="bam" if bam else None)
        assert all(w in str(e.value) for w in (path,) + words), str(e.value)

    import gzip
    refused(good[:second] + gzip.compress(b"@r\nACGT\n+\nIIII\n", mtime=0), f"at byte {second}", "no BGZF member")
    refused(good[:-40], "ends inside the member at byte")
    damaged = bytearray(good)
    damaged[int(table["src_off"][2]) + 5] ^= 0x40
    refused(bytes(damaged), f"byte {int(table['src_off'][2])}", "corrupt")
    bam = open(B.bam_path("k27"), "rb").read()
    bt = B.py_table(bam)
    refused(bam[:int(bt["src_off"][10]) - 18] + B.EOF, "ends inside a record", bam=True, name="cut.bam")
    refused(bam[:int(bt["src_off"][1]) - 18] + B.EOF, "ends inside the header", bam=True, name="head.bam")
    refused(good, "magic", bam=True, name="notbam.bam")
    for verb, k in ((tools.count, "-k27"), (tools.count_small, "-k9")):
        for opt in ("-fa", "-fq", "-fm"):
            with pytest.raises(tools.UsageError) as e:
                verb([k, opt, B.bam_path("k27"), str(tmp_path / "o")], ctx=lib, input_format="bam")
            assert opt in str(e.value)
        with pytest.raises(ValueError):
            verb([k, B.bam_path("k27"), str(tmp_path / "o")], ctx=lib, input_format="sam")
    with pytest.raises(tools.UsageError) as e:
        args = Q.command_line(Q.LINES[0], str(tmp_path / "f"))
        args[args.index(os.path.join(Q.GOLDEN, Q.FQ))] = str(tmp_path / "x.fq.gz")
        tools.filter_reads(args[1:], ctx=lib)
    assert "x.fq.gz" in str(e.value) and "corrupt" in str(e.value)
    assert not os.path.exists(str(tmp_path / "o.kmc_pre"))


def test_fbam_is_still_refused_and_says_what_to_use():
    for parse, k in ((tools.parse_count, "-k27"), (tools.parse_count_small, "-k9")):
        with pytest.raises(tools.UsageError) as e:
            parse([k, "-fbam", "in.bam", "out"])
        assert "-fbam" in str(e.value).split("\n")[0] and "KMC_HIP_COUNT_IN=bam" in str(e.value).split("\n")[0]
    assert "KMC_HIP_COUNT_IN=bam" in tools.COUNT_USAGE and "bgzip" in tools.COUNT_USAGE


def test_the_command_line_reads_bam(tmp_path):
    """through main, in a process of its own"""
    out = str(tmp_path / "o")
    env = dict(os.environ, KMC_HIP_LIB=emu.build_hostlib("small"), KMC_HIP_COUNT_IN="bam", KMC_HIP_COUNT_PART_MB="0")
    r = subprocess.run([sys.executable, "-m", "kmc_amd.tools", "count", "-k27", "-n8", B.bam_path("k27"), out], cwd=ROOT, capture_output=True, text=True, timeout=1200, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    assert B.database_bytes(out) == B.database_bytes(B.bam_out("k27")) and "Total no. of reads" in r.stdout
    r = subprocess.run([sys.executable, "-m", "kmc_amd.tools", "count-small", "-k9", B.bam_path("k9"), out + "9"], cwd=ROOT, capture_output=True, text=True, timeout=1200, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    assert B.database_bytes(out + "9") == B.database_bytes(B.bam_out("k9"))
