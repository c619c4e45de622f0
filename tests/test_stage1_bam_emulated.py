"""CPU: stage 1 on the device for BAM input (-fbam) and KMC databases (-fkmc) — kmc_hip_split_part with file_type 4 (k_s1_bam_chain + k_s1_bam_decode in
front of k_s1_cut, kmc_amd/csrc/stage1_chain.h) in the PRODUCT'S host library compiled over the emulated HIP runtime (tests/emu.py build_hostlib).

The stage-1 oracle has no BAM branch. The expectation comes from an equivalence that needs none: a part of BAM records and a part of single-line FASTA that
holds the sequences CSplitter::GetSeq's BAM branch (splitter.cpp:326-419) returns for those records — the included ones, in order, reversed and complemented
where the reference reverses them, N for every nibble that is not A C G T (kmc_amd/synth.py bam_reads_as_getseq) — must give the same records per bin, the
same four per-bin sums and the same n_reads through kmc_hip_split_part. An included record without bases has no FASTA line (a blank line is malformed text):
it is left out of the twin and its count added on the BAM side. The FASTA road is pinned to the stage-1 oracle by tests/test_stage1_emulated.py.
The cases are sized to the kernels' seams (a tile of 8192 bytes of records, a unit of 16 codes, a tile of 256 records); the -m gpu file runs them on the device."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import emu
from kmc_amd import capi, synth
from test_stage1_emulated import _parse_bin, _sig_map
from test_stage1_estimate_emulated import EstLib
from test_stage1_multiline_emulated import _exe, _require, _run

TILE = 8192  # S1_BAM_TILE of kmc_amd/csrc/stage1_kernels.hip.h
LINE_CAP = 1 << 17
UNCOVERED = 1  # KMC_HIP_UNCOVERED
NIBBLES = "=ACMGRSVTWYHKDBN"
BAM = capi.SPLIT_FILE_BAM


# ---- the two roads
def split(lib, text, file_type, k=27, m=9, n_bins=37, line_cap=LINE_CAP, max_x=3, both=True, flags=0):
    return lib.split(text, k, m, n_bins, _sig_map(m, n_bins, 5), line_cap, file_type, 0, max_x, both, flags)


def fasta_twin(reads, both):
    """-> (single-line FASTA text with empty titles, as the reference's KMC-database reader writes them; included records; those without bases)"""
    seqs, n = synth.bam_reads_as_getseq(reads, both)
    return b"".join(b">\n" + s + b"\n" for s in seqs if s), n, sum(1 for s in seqs if not s)


def same(got, want, k, extra_reads=0):
    assert got["n_reads"] == want["n_reads"] + extra_reads, (got["n_reads"], want["n_reads"], extra_reads)
    for b in range(len(want["bins"])):
        assert _parse_bin(got["bins"][b], k) == _parse_bin(want["bins"][b], k), b
    for key in ("kmers", "supers", "plus_x"):
        assert np.array_equal(got[key], want[key]), key
    assert [x.size for x in got["bins"]] == [x.size for x in want["bins"]]  # the fourth sum: bytes per bin


def check_bam(lib, reads, records=None, **kw):
    """reads: (stored sequence, flag) per record; records: their BAM records when the case builds them itself"""
    part = synth.bam_part(records if records is not None else [synth.bam_record(s, f, b"r%d" % i, n_cigar=i % 3) for i, (s, f) in enumerate(reads)])
    k, both = kw.get("k", 27), kw.get("both", True)
    rc, got = split(lib, part, capi.SPLIT_FILE_BAM, **kw)
    assert rc == 0, got
    twin, n, empty = fasta_twin(reads, both)
    rc, want = split(lib, twin, 0, **kw)
    assert rc == 0, want
    assert want["n_reads"] == n - empty
    same(got, want, k, empty)
    return got


# ---- inputs
def _seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=n))


def edge_reads(k=27, seed=0):
    """every length around k, every nibble value inside a read long enough to hold k-mers on both sides of it, every flag the branch looks at"""
    rng = np.random.default_rng(seed)
    reads = []
    for flag in (0, 0x10, 0x100, 0x800, 0x900, 0x910, 0x1 | 0x40):
        for n in (0, 1, k - 1, k, k + 1, 151, 150, 16, 17, 31, 32, 33):
            reads.append((_seq(rng, n), flag))
        reads.append((_seq(rng, 40) + NIBBLES + _seq(rng, 41), flag))
        reads.append((_seq(rng, 300, "ACGTN="), flag))
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def seam_case(kind, at, seed=1):
    """A part in which the record `target` lies so that the boundary between the first two tiles (byte TILE) falls `at` bytes behind the start of its `kind`:
    "start" (at 0..3: inside the block_size word; 0 = exactly at the end of the record in front), "header", "name", "bases" (at nibble byte `at`), "end" (the record
    ends at the boundary). Records around it are ordinary reads; one filler record is padded with tag bytes to put the target in place."""
    rng = np.random.default_rng(seed)
    name = b"the_target_read_name_is_long"
    target_seq, flag = _seq(rng, 201 if at & 1 else 200), 0x10 if at & 1 else 0
    target = synth.bam_record(target_seq, flag, name, n_cigar=2, tags=b"XYZ")
    into = {"start": at, "header": 4 + at, "name": 36 + at, "bases": 36 + len(name) + 1 + 8 + at, "end": len(target)}[kind]
    start = TILE - into
    reads, records, used = [], [], 0
    while used < start - 700:
        s, f = _seq(rng, int(rng.integers(20, 260))), int(rng.choice([0, 0x10, 0x100]))
        reads.append((s, f))
        records.append(synth.bam_record(s, f, b"q%d" % len(reads), n_cigar=len(reads) % 2))
        used += len(records[-1])
    s = _seq(rng, 100)
    reads.append((s, 0))
    records.append(synth.bam_record(s, 0, b"filler", pad_to=start - used))
    assert used + len(records[-1]) == start
    reads.append((target_seq, flag))
    records.append(target)
    for i in range(12):
        s, f = _seq(rng, int(rng.integers(20, 260))), int(rng.choice([0, 0x10, 0x800]))
        reads.append((s, f))
        records.append(synth.bam_record(s, f, b"t%d" % i))
    return reads, records


SEAMS = [("start", 0), ("start", 1), ("start", 2), ("start", 3), ("header", 10), ("header", 17), ("name", 5), ("bases", 20), ("bases", 21), ("end", 0)]


def long_record_case(dense_around, seed=2):
    """a record longer than two tiles; with dense_around, block_size-35 records (name "\\0", one base: the smallest record with a base) on both sides"""
    rng = np.random.default_rng(seed)
    small = [(_seq(rng, 1), int(rng.choice([0, 0x10]))) for _ in range(300 if dense_around else 0)]
    long_seq = _seq(rng, 12_001)
    for at in (0, 3000, 3001, 8191, 12_000):
        long_seq = long_seq[:at] + "N" + long_seq[at + 1:]
    reads = small[:150] + [(long_seq, 0x10)] + small[150:] + [(_seq(rng, 90), 0)]
    records = [synth.bam_record(s, f, b"" if len(s) == 1 else b"long") for s, f in reads]
    assert len(records[150 if dense_around else 0]) > 2 * TILE and (not dense_around or len(records[0]) == 39)
    return reads, records


def dense_case(n, seed=3):
    """only block_size-35 records: the densest chain the format allows (hops of 39 bytes, 211 per tile); no k-mer, so n_reads and empty bins are what is compared"""
    rng = np.random.default_rng(seed)
    reads = [(_seq(rng, 1, "ACGTN"), int(rng.choice([0, 0x10, 0x100]))) for _ in range(n)]
    return reads, [synth.bam_record(s, f, b"") for s, f in reads]


def good_reads(seed=4, n=40):
    rng = np.random.default_rng(seed)
    return [(_seq(rng, int(rng.integers(30, 200))), int(rng.choice([0, 0x10]))) for _ in range(n)]


def _patched(rec, block_size=None, l_seq=None):
    b = bytearray(rec)
    if block_size is not None:
        b[0:4] = struct.pack("<i", block_size)
    if l_seq is not None:
        b[20:24] = struct.pack("<i", l_seq)
    return bytes(b)


def malformed_parts(k=27):
    """name -> (part, line_cap): each must come back KMC_HIP_UNCOVERED"""
    reads = good_reads(5, 60)  # ~ one and a half tiles
    recs = [synth.bam_record(s, f, b"m%d" % i) for i, (s, f) in enumerate(reads)]
    last = recs[-1]
    bs = struct.unpack("<i", last[:4])[0]
    cap = k + 4096 + 2
    at_cap = synth.bam_record(("ACGT" * 1100)[:cap], 0, b"cap")
    return {
        "one_byte_past": (b"".join(recs[:-1]) + _patched(last, bs + 1), LINE_CAP),
        "one_byte_short": (b"".join(recs[:-1]) + _patched(last, bs - 1), LINE_CAP),
        "block_size_31": (b"".join(recs[:30]) + _patched(recs[30], 31) + b"".join(recs[31:]), LINE_CAP),
        "block_size_31_first": (_patched(recs[0], 31) + b"".join(recs[1:]), LINE_CAP),
        "block_size_negative": (b"".join(recs[:30]) + _patched(recs[30], -bs) + b"".join(recs[31:]), LINE_CAP),
        "block_size_below_its_fields": (b"".join(recs[:30]) + _patched(recs[30] + recs[31], len(recs[30]) + len(recs[31]) - 4, 4000) + b"".join(recs[32:]), LINE_CAP),
        "l_seq_negative": (b"".join(recs[:30]) + _patched(recs[30], l_seq=-5) + b"".join(recs[31:]), LINE_CAP),
        "l_seq_at_line_cap": (b"".join(recs[:10]) + at_cap + b"".join(recs[10:]), cap),
        "header_cut_off": (b"".join(recs[:-1]) + last[:20], LINE_CAP),
        "header_cut_off_block_size_fits": (b"".join(recs[:-1]) + _patched(last, 16)[:20], LINE_CAP),
        "header_cut_off_32_fit": (b"".join(recs[:-1]) + _patched(last, 32)[:34], LINE_CAP),
    }


class BamLib(EstLib):
    pass


@pytest.fixture(scope="module")
def hostlib():
    lib = BamLib(emu.build_hostlib("small"))
    yield lib
    lib.close()


# ---- 1: the interface
def test_the_library_says_it_covers_bam_records(hostlib):
    L = hostlib.L
    assert L.kmc_hip_abi_version() == 4 and capi.SPLIT_FILE_BAM == 4
    assert [L.kmc_hip_split_covers(t) for t in (0, 1, 2, 3, 4, 5)] == [1, 1, 1, 0, 1, 0]  # 3 stays unknown: callers from before BAM use it as such
    part = synth.bam_part([synth.bam_record("ACGT" * 10)])
    smap = _sig_map(9, 8, 1)
    for unknown in (3, 5):
        rc, msg = hostlib.split(part, 27, 9, 8, smap, LINE_CAP, unknown, flags=0)
        assert rc == -1 and b"unsupported" in msg
    rc, msg = hostlib.split(part, 27, 9, 8, smap, LINE_CAP, BAM, 1, flags=0)  # a long-read part of BAM records does not exist
    assert rc == -1 and b"part_kind" in msg
    assert hostlib.split(part, 27, 9, 8, smap, LINE_CAP, BAM, flags=0)[0] == 0


def test_an_empty_title_line_passes_the_record_check(hostlib):
    """-fkmc: the reference's reader turns a KMC database into ">\\n<k-mer>\\n" per k-mer (binary_reader.h:238-304)"""
    rng = np.random.default_rng(6)
    seqs = [_seq(rng, 27).encode() for _ in range(300)]
    rc, got = split(hostlib, b"".join(b">\n" + s + b"\n" for s in seqs), 0)
    assert rc == 0, got
    rc, want = split(hostlib, b"".join(b">r%d\n" % i + s + b"\n" for i, s in enumerate(seqs)), 0)
    assert rc == 0
    same(got, want, 27)
    assert got["n_reads"] == 300 and int(got["kmers"].sum()) == 300


# ---- 2: the kernels
@pytest.mark.parametrize("both,max_x,k", [(True, 3, 27), (False, 0, 27), (False, 3, 27), (True, 0, 55)], ids=["canonical-x3", "b-x0", "b-x3", "k55-x0"])
def test_nibbles_lengths_and_flags(hostlib, both, max_x, k):
    reads = edge_reads(k)
    got = check_bam(hostlib, reads, both=both, max_x=max_x, k=k)
    assert got["n_reads"] == sum(1 for _, f in reads if not f & 0x900)
    if not both:  # the flag does change the result: the same records taken as forward reads give other bins
        fwd = [(s, f & ~0x10) for s, f in reads]
        rc, other = split(hostlib, synth.bam_part([synth.bam_record(s, f, b"r%d" % i, n_cigar=i % 3) for i, (s, f) in enumerate(fwd)]), BAM, both=False, max_x=max_x, k=k)
        assert rc == 0 and any(_parse_bin(a, k) != _parse_bin(b, k) for a, b in zip(got["bins"], other["bins"]))


@pytest.mark.parametrize("kind,at", SEAMS, ids=["%s+%d" % s for s in SEAMS])
def test_a_record_across_the_tile_seam(hostlib, kind, at):
    reads, records = seam_case(kind, at)
    assert TILE < sum(len(r) for r in records) < 2 * TILE
    check_bam(hostlib, reads, records, both=False)


@pytest.mark.parametrize("dense_around", [False, True], ids=["alone", "among-block-size-35"])
def test_a_record_longer_than_two_tiles(hostlib, dense_around):
    reads, records = long_record_case(dense_around)
    got = check_bam(hostlib, reads, records, both=False)
    assert int(got["kmers"].sum()) > 5000


def test_the_densest_chain(hostlib):
    reads, records = dense_case(700)
    assert 3 * TILE < 39 * len(records) < 4 * TILE
    got = check_bam(hostlib, reads, records)
    assert int(got["kmers"].sum()) == 0 and got["n_reads"] == sum(1 for _, f in reads if not f & 0x900)


def test_trivial_parts(hostlib):
    rc, got = split(hostlib, b"", BAM)
    assert rc == 0 and got["n_reads"] == 0 and int(got["kmers"].sum()) == 0
    check_bam(hostlib, [("ACGT" * 20, 0)])
    check_bam(hostlib, [("ACGT" * 20, 0x100)])
    check_bam(hostlib, [("", 0)])


@pytest.mark.parametrize("name", sorted(malformed_parts()))
def test_malformed_records_are_refused_and_the_context_goes_on(hostlib, name):
    part, line_cap = malformed_parts()[name]
    rc, _ = split(hostlib, part, BAM, line_cap=line_cap)
    assert rc == UNCOVERED
    check_bam(hostlib, good_reads())


def test_a_skipped_record_may_be_as_long_as_it_likes(hostlib):
    """the line cap bounds what the reference writes into its buffer: a secondary record is never written"""
    k = 27
    cap = k + 4096 + 2
    rng = np.random.default_rng(8)
    reads = good_reads(9, 5) + [(_seq(rng, cap + 50), 0x100), (_seq(rng, cap - 1), 0)] + good_reads(10, 5)
    check_bam(hostlib, reads, line_cap=cap)


# ---- 3: with the flags
def test_bam_parts_with_homopolymer_compression(hostlib):
    rng = np.random.default_rng(11)
    reads = [(synth.homopolymer_rich_sequence(rng, int(rng.integers(30, 500)), 2.0).tobytes().decode(), int(rng.choice([0, 0x10, 0x100]))) for _ in range(60)]
    got = check_bam(hostlib, reads, both=False, flags=capi.SPLIT_HOMOPOLYMER)
    plain = check_bam(hostlib, reads, both=False)
    assert int(got["kmers"].sum()) < int(plain["kmers"].sum())


def test_bam_parts_with_the_histogram_estimate(hostlib):
    k, s, r = 27, 2, 12
    reads = edge_reads(k, 12) + good_reads(13, 60)
    counters = []
    for file_type in (BAM, 0):
        assert hostlib.open(k, s, r) == 0
        text = synth.bam_part([synth.bam_record(q, f, b"e%d" % i) for i, (q, f) in enumerate(reads)]) if file_type == BAM else fasta_twin(reads, False)[0]
        rc, got = split(hostlib, text, file_type, both=False, flags=capi.SPLIT_ESTIMATE)
        assert rc == 0, got
        counters.append(hostlib.read_all(r))
        hostlib.close_estimator()
    assert np.array_equal(counters[0], counters[1]) and int(counters[0].sum()) > 100


# ---- 4: the product binary over the emulated library
def _write_bam(path, seed, n_reads):
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n_reads):
        s = _seq(rng, int(rng.integers(0, 320)), "ACGT" if i % 9 else "ACGTNR")
        reads.append((s, [0, 0x10, 0x100, 0x800, 0x1, 0x10, 0x910][int(rng.integers(0, 7))]))
    recs = [synth.bam_record(s, f, b"read_%d" % i, n_cigar=i % 3, tags=b"NMC\x01" if i % 2 else b"") for i, (s, f) in enumerate(reads)]
    synth.write_bam(path, recs, block_bytes=3000, refs=[(b"chr1", 1000)])
    return reads


_state = {"broken": False}
FLAG_SETS = [["-k27", "-ci1"], ["-k27", "-b"], ["-k27", "-hc"], ["-k27", "--opt-out-size"], ["-k55"]]


@pytest.mark.parametrize("flags", FLAG_SETS, ids=["default", "b", "hc", "opt-out-size", "k55"])
def test_kmc_hip_s1_fbam_over_the_emulated_library_writes_the_reference_database(flags, tmp_path):
    _require("kmc", "kmc_hip_s1")
    if _state["broken"]:
        pytest.fail("an earlier run of kmc_hip_s1 -fbam over the emulated library failed")
    inp = str(tmp_path / "in.bam")
    reads = _write_bam(inp, 21, 400)
    common = flags + ["-fbam", "-m2", "-sf1", "-n64"]
    rc, want, log = _run("kmc", common + ["-sp1", "-sr1"], inp, tmp_path, "ref")
    assert rc == 0, log[-1500:]
    assert int(want[1][5]) == sum(1 for _, f in reads if not f & 0x900)  # the reference reads what the generator wrote
    rc, got, log = _run("kmc_hip_s1", common + ["-sp2", "-sr2"], inp, tmp_path, "emu", env={"KMC_HIP_LIB": emu.build_hostlib("small"), "KMC_HIP_VERBOSE": "1"})
    _state["broken"] = rc != 0
    assert rc == 0, log[-1500:]
    assert got == want and len(want[1]) >= 5
    rep = re.findall(r"(\d+) uncovered parts, .* (\d+) BAM parts", log)
    assert rep and sum(int(u) for u, _ in rep) == 0 and sum(int(b) for _, b in rep) >= 1, log[-1500:]


def test_kmc_hip_s1_fkmc_over_the_emulated_library_writes_the_reference_database(tmp_path):
    _require("kmc", "kmc_hip_s1")
    fq = str(tmp_path / "in.fq")
    synth.make_fastq(fq, 3, 20_000, 400, 100)
    rc, _, log = _run("kmc", ["-k27", "-ci1", "-m2", "-sf1", "-sp1", "-sr1", "-n64"], fq, tmp_path, "src")
    assert rc == 0, log[-1500:]
    db = str(tmp_path / "db_src")
    common = ["-k25", "-ci1", "-fkmc", "-m2", "-sf1", "-n64"]
    rc, want, log = _run("kmc", common + ["-sp1", "-sr1"], db, tmp_path, "ref")
    assert rc == 0, log[-1500:]
    rc, got, log = _run("kmc_hip_s1", common + ["-sp2", "-sr2"], db, tmp_path, "emu", env={"KMC_HIP_LIB": emu.build_hostlib("small"), "KMC_HIP_VERBOSE": "1"})
    assert rc == 0, log[-1500:]
    assert got == want and int(want[1][4]) > 10_000
    assert "0 uncovered parts" in log


def test_kmc_hip_s1_fbam_over_a_library_without_the_answer_is_refused(tmp_path):
    """the mock library has no kmc_hip_split_covers: the worker refuses the BAM job by name, as before"""
    _require("kmc_hip_s1")
    inp = str(tmp_path / "in.bam")
    _write_bam(inp, 22, 50)
    rc, _, log = _run("kmc_hip_s1", ["-k27", "-fbam", "-m2", "-sf1", "-sp1", "-sr1"], inp, tmp_path, "mock", env={"KMC_HIP_LIB": emu.build_mock()})
    assert rc != 0 and "does not cover an input format other than FASTA / FASTQ (multi-line FASTA, BAM, KMC)" in log, log[-800:]
