"""CPU: stage 1 on the device with homopolymer compression (-hc) — kmc_hip_split_part with KMC_HIP_SPLIT_HOMOPOLYMER (k_s1_hc_compact in front of
k_s1_cut, kmc_amd/csrc/stage1_chain.h) in the PRODUCT'S host library compiled over the emulated HIP runtime (tests/emu.py build_hostlib).

The oracle is the reference's rule restated: CSplitter::ProcessReads compresses EVERY BUFFER GetSeq returns on its own (HomopolymerCompressSeq,
splitter.cpp:424-435, :575-581) — a whole line, or one piece of a line of line_cap symbols or more / of a long-read part / of a multi-line sequence.
tests/oracle_s1.py parse_part (and getseq_multiline of the -fm tests) return exactly those buffers as code arrays; each is compressed in numpy and goes
through S1.split / split_stream / kxmer_recs. Compared per bin: the record multiset, bin_kmers, bin_superkmers, bin_plus_x; and n_reads.
The cases are sized to the kernel's seams (a thread's 16 bytes, a wave's 1024, a tile's 4096, the piece starts), not to a workload; the -m gpu file
runs the same cases on the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emu
import oracle_s1 as S1
from kmc_amd import capi, synth
from test_stage1_emulated import _parse_bin, _records_text, _sig_map
from test_stage1_multiline_emulated import SplitLib, _exe, _require, _run, _wrap, getseq_multiline, multiline_cases, reader_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)


# ---- the reference's rule
def hc_compress(q):
    """HomopolymerCompressSeq over one code array: the first code and every code that differs from the one before it (all invalid symbols are -1)"""
    if q.size == 0:
        return q
    keep = np.ones(q.size, dtype=bool)
    keep[1:] = q[1:] != q[:-1]
    return q[keep]


def getseq_returns(text, file_type, k, line_cap, long_read=False):
    """the buffers CSplitter::GetSeq hands ProcessReads for this part, as code arrays, and n_reads"""
    if file_type == 2:
        return getseq_multiline(text, k, line_cap)
    return S1.parse_part(text, file_type, k, line_cap, long_read=long_read)


def oracle_of_returns(returns, n_reads, k, m, n_bins, smap, max_x=3, both=True):
    """what the super-k-mer loop + the collectors make of these buffers (as _oracle_split_part of tests/test_stage1_emulated.py)"""
    want = dict(bins=[[] for _ in range(n_bins)], kmers=np.zeros(n_bins, dtype=np.uint64), supers=np.zeros(n_bins, dtype=np.uint64),
                plus_x=np.zeros(n_bins, dtype=np.uint64), n_reads=n_reads, pieces=len(returns))
    for q in returns:
        if q.size < k:
            continue
        sig, off, recs = S1.split([_LETTERS[np.where(q < 0, 4, q)].tobytes()], k, m)
        pos, ln, sg = S1.split_stream(q, k, m)
        assert np.array_equal(sig, sg)
        for i in range(sig.size):
            b = int(smap[sig[i]])
            want["bins"][b].append(bytes(recs[int(off[i]):int(off[i + 1])]))
            want["kmers"][b] += int(ln[i]) - k + 1
            want["supers"][b] += 1
            want["plus_x"][b] += S1.kxmer_recs(q[int(pos[i]):int(pos[i] + ln[i])], k, max_x, both)
    return want


def oracle_hc(text, file_type, k, m, n_bins, smap, line_cap, long_read=False, max_x=3, both=True):
    returns, n_reads = getseq_returns(text, file_type, k, line_cap, long_read)
    return oracle_of_returns([hc_compress(q) for q in returns], n_reads, k, m, n_bins, smap, max_x, both)


def compress_then_cut(line_codes, k, line_cap):
    """NOT the reference's rule: the whole line compressed first, then cut into pieces as GetSeq cuts a line"""
    q, stride = hc_compress(line_codes), line_cap - k + 1
    if q.size < line_cap:
        return [q]
    return [q[s:s + line_cap] for s in range(0, q.size, stride)]


def same_result(a, b):
    return (all(sorted(x) == sorted(y) for x, y in zip(a["bins"], b["bins"])) and all(np.array_equal(a[key], b[key]) for key in ("kmers", "supers", "plus_x")))


# ---- the product's library
class HcLib(SplitLib):
    """kmc_hip_split_part with the flags word (the emulated product library here, libkmc_hip.so in the -m gpu file)"""

    def split(self, text, k, m, n_bins, smap, line_cap, file_type, part_kind=0, max_x=3, both=True, flags=capi.SPLIT_HOMOPOLYMER):
        L = self.L
        assert L.kmc_hip_split_set_map(self.h, 0, smap.ctypes.data, m) == 0
        p = capi.SplitParams(k, m, n_bins, max_x, 1 if both else 0, file_type, line_cap, part_kind, flags)
        t = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(0, dtype=np.uint8)
        recs = np.zeros(2 * t.size + 256 * (n_bins + 1) + 4096, dtype=np.uint8)
        arr = [np.zeros(n_bins, dtype=np.uint64) for _ in range(5)]
        need, n_reads = C.c_uint64(0), C.c_uint64(0)
        rc = L.kmc_hip_split_part(self.h, 0, 0, C.byref(p), t.ctypes.data, t.size, recs.ctypes.data, recs.size, C.byref(need), *[a.ctypes.data for a in arr],
                                  C.byref(n_reads))
        if rc:
            return rc, L.kmc_hip_last_error(self.h)
        off, nbytes, kmers, supers, plus_x = arr
        return 0, dict(bins=[recs[int(off[b]):int(off[b] + nbytes[b])].copy() for b in range(n_bins)], kmers=kmers, supers=supers, plus_x=plus_x,
                       n_reads=n_reads.value)


def check_hc(lib, text, file_type, k, line_cap, long_read=False, m=9, n_bins=37, max_x=3, both=True):
    smap = _sig_map(m, n_bins, 5)
    rc, got = lib.split(text, k, m, n_bins, smap, line_cap, file_type, 1 if long_read else 0, max_x, both)
    assert rc == 0, got
    want = oracle_hc(text, file_type, k, m, n_bins, smap, line_cap, long_read, max_x, both)
    assert got["n_reads"] == want["n_reads"]
    for b in range(n_bins):
        assert _parse_bin(got["bins"][b], k) == sorted(want["bins"][b]), b
    for key in ("kmers", "supers", "plus_x"):
        assert np.array_equal(got[key], want[key]), key
    return want


# ---- inputs
def _rnd(rng, n, alphabet=b"ACGT"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return a[rng.integers(0, a.size, size=n)].tobytes()


def _norun(rng, n):
    """n symbols, no two neighbours equal: what -hc leaves unchanged"""
    return _ACGT[np.cumsum(rng.integers(1, 4, size=n)) & 3].tobytes()


def seam_reads(k, seed=0):
    """The reads of the three-tile part, in stream order. Code stream position = symbols and separators before: the first read puts runs across a thread's
    16-byte boundary (15|16) and a wave's (1023|1024), a later one across the tile boundary (4095|4096); then 9 000 identical symbols, so that the whole
    third tile keeps nothing (its aggregate in the look-back is zero)."""
    rng = np.random.default_rng(1000 * k + seed)
    first = bytearray(_rnd(rng, 1100))
    first[13:19] = b"GGGGGG"
    first[1020:1028] = b"TtTtTtTt"
    expand = lambda t, at, times: t[:at] + t[at:at + 1] * times + t[at + 1:]  # compresses back to t
    squeeze_below = expand(_norun(rng, k - 1), 5, 7)  # k + 5 symbols, k - 1 after compression
    squeeze_to_k = expand(_norun(rng, k), 7, 4)  # k + 3 symbols, exactly k after compression
    reads = [bytes(first), b"aAaAcC" + _rnd(rng, 60) + b"aAaAcC", _rnd(rng, 1), b"", _norun(rng, k - 1), _norun(rng, k), squeeze_below, squeeze_to_k,
             b"NNNN" + _rnd(rng, 90) + b"nnNNN", b"N" + _rnd(rng, 2 * k) + b"N", b"C" * 300, _rnd(rng, 200, b"ACGTacgtN"), _rnd(rng, 150)]
    used = sum(len(r) + 1 for r in reads)
    assert used < 4000
    reads.append(_rnd(rng, 4096 - used - 3) + b"AAAAAaaA" + _rnd(rng, 70))
    reads += [b"T" * 9000, _rnd(rng, 120), b"G" * (k + 5) + _norun(rng, k)]
    return reads


def piece_lines(k, rng):
    """-> (lines, line_cap, special): lines of 1, 2 and 5 pieces, one of exactly the cap and one a symbol short of it, and three built on a run-free base so that
    the one thing planted at the piece start M = stride decides: (a) raw[M] == raw[M - 1], (b) a run inside the k - 1 symbols two pieces share, (c) N at M"""
    line_cap = k + 4105
    stride = line_cap - k + 1
    base = lambda n: _norun(rng, n)
    b_a, b_b, b_c = base(stride + 700), base(stride + 700), bytearray(base(2 * stride + 300))
    line_a = b_a[:stride] + b_a[stride - 1:stride] + b_a[stride:]  # the symbol in front of the piece start once more: raw[M] == raw[M - 1]
    line_b = b_b[:stride + 6] + b_b[stride + 5:stride + 6] + b_b[stride + 6:]  # raw[M + 5] == raw[M + 6], inside the overlap
    b_c[stride] = ord("N")
    b_c[2 * stride] = ord("n")
    special = dict(a=line_a, b=line_b, c=bytes(b_c))
    rich = lambda n: synth.homopolymer_rich_sequence(rng, n, 1.8, 0.2).tobytes()
    lines = [rich(700), rich(line_cap), rich(60), rich(line_cap - 1), rich(4 * stride + 900), line_a, rich(100), line_b, bytes(b_c), rich(stride + 40), _rnd(rng, 300),
             b"A" * (line_cap + 300), rich(2 * stride + 5)]
    return lines, line_cap, special


@pytest.fixture(scope="module")
def hostlib():
    lib = HcLib(emu.build_hostlib("small"))
    yield lib
    lib.close()


# ---- 1
def test_the_library_says_it_covers_homopolymer_compression(hostlib):
    L = hostlib.L
    assert L.kmc_hip_abi_version() == 4
    assert L.kmc_hip_split_covers(capi.SPLIT_COVERS_HOMOPOLYMER) == 1
    assert [L.kmc_hip_split_covers(t) for t in (0, 1, 2, 3, 0x101, 0x200)] == [1, 1, 1, 0, 0, 0]
    smap = _sig_map(9, 8, 1)
    for flags in (2, 3, 0x80000000, 0x100):
        rc, msg = hostlib.split(b">t\nACGTACGT\n", 27, 9, 8, smap, 27 + 4105, 0, flags=flags)
        assert rc == -1 and b"flags" in msg, (flags, rc, msg)  # KMC_HIP_EINVAL
    assert hostlib.split(b">t\nACGTACGT\n", 27, 9, 8, smap, 27 + 4105, 0, flags=1)[0] == 0


def test_the_flag_changes_the_result_and_its_absence_does_not(hostlib):
    """flags = 0 is the part without -hc (the existing oracle), flags = 1 is not"""
    k, rng = 27, np.random.default_rng(2)
    text = _records_text("fq", b"\n", [synth.homopolymer_rich_sequence(rng, 400, 2.0).tobytes() for _ in range(20)])
    smap = _sig_map(9, 37, 5)
    rc, plain = hostlib.split(text, k, 9, 37, smap, 1 << 17, 1, flags=0)
    assert rc == 0
    returns, n_reads = getseq_returns(text, 1, k, 1 << 17)
    assert same_result(dict(plain, bins=[_parse_bin(b, k) for b in plain["bins"]]), oracle_of_returns(returns, n_reads, k, 9, 37, smap))
    want = check_hc(hostlib, text, 1, k, 1 << 17)
    assert int(want["kmers"].sum()) < int(plain["kmers"].sum())


# ---- 2
@pytest.mark.parametrize("fmt,eol,k,both", [("fq", b"\n", 27, True), ("fq", b"\r\n", 21, True), ("fa", b"\n", 55, True), ("fa", b"\r\n", 27, False)],
                         ids=["fq-lf-k27", "fq-crlf-k21", "fa-lf-k55", "fa-crlf-k27-b"])
def test_runs_across_every_seam_of_the_compaction_kernel(hostlib, fmt, eol, k, both):
    reads = seam_reads(k)
    text = _records_text(fmt, eol, reads)
    returns, _ = getseq_returns(text, 1 if fmt == "fq" else 0, k, 1 << 17)
    stream = np.concatenate([np.concatenate([q, np.array([-1], dtype=np.int8)]) for q in returns])
    assert 3 * 4096 < stream.size <= 4 * 4096 and len(returns) == len(reads)
    for seam in (16, 1024, 4096):  # a run lies across the seam
        assert stream[seam - 2] == stream[seam - 1] == stream[seam] == stream[seam + 1] >= 0, seam
    assert np.all(stream[2 * 4096 - 1:3 * 4096 + 1] == stream[2 * 4096])  # the third tile keeps nothing
    lens = sorted(hc_compress(q).size for q in returns)
    assert {0, 1, k - 1, k} <= set(lens) and lens.count(k) >= 2 and lens.count(k - 1) >= 2
    assert np.array_equal(hc_compress(returns[1])[:2], [0, 1])  # aAaAcC -> AC
    check_hc(hostlib, text, 1 if fmt == "fq" else 0, k, 1 << 17, both=both)


# ---- 3
@pytest.mark.parametrize("fmt,eol,k,both", [("fq", b"\n", 27, True), ("fa", b"\r\n", 21, True), ("fa", b"\n", 55, False)], ids=["fq-k27", "fa-crlf-k21", "fa-k55-b"])
def test_every_piece_of_a_long_line_is_compressed_on_its_own(hostlib, fmt, eol, k, both):
    rng = np.random.default_rng(50 + k)
    lines, line_cap, special = piece_lines(k, rng)
    ft = 1 if fmt == "fq" else 0
    want = check_hc(hostlib, _records_text(fmt, eol, lines), ft, k, line_cap, both=both)
    # extra pieces: 1 for the line of the cap, 4 for the five-piece line, 1 + 1 + 2 for (a), (b), (c), 1 for the poly-A line, 1 at least for the last line
    assert want["pieces"] >= len(lines) + 11
    # the planted lines alone: per-piece compression is NOT "compress the line, then cut"
    smap = _sig_map(9, 37, 5)
    for name in ("a", "b"):
        line = special[name]
        per_piece = check_hc(hostlib, _records_text(fmt, eol, [line]), ft, k, line_cap, both=both)
        whole = oracle_of_returns(compress_then_cut(S1.encode([line])[0], k, line_cap), 1, k, 9, 37, smap, 3, both)
        assert not same_result(per_piece, whole), name
        if name == "b":  # the run inside the overlap shortens the tail of the first piece: the k-mer across it exists in neither piece
            assert int(per_piece["kmers"].sum()) == int(whole["kmers"].sum()) - 1
    if fmt == "fa":  # a FASTA part may end inside a long last line
        text = _records_text(fmt, eol, lines[:3] + [special["a"]])
        check_hc(hostlib, text[: len(text) - len(eol)], 0, k, line_cap, both=both)


# ---- 4
@pytest.mark.parametrize("fmt,k", [("fa", 27), ("fq", 21), ("fq", 55)])
def test_long_read_parts_are_compressed_piece_by_piece(hostlib, fmt, k):
    """ReadType::long_read parts: the symbols start AT the title's end of line, pieces start every stride symbols from there (GetSeqLongRead, splitter.cpp:70-86)"""
    rng = np.random.default_rng(70 + k)
    line_cap = k + 4105
    stride = line_cap - k + 1
    ft, marker = (1, b"@") if fmt == "fq" else (0, b">")
    smap = _sig_map(9, 37, 5)
    body = bytearray(synth.homopolymer_rich_sequence(rng, 4 * stride + 1234, 1.8, 0.2).tobytes())
    for titled in (True, False):
        shift = 1 if titled else 0  # the end of line of the title is symbol 0 of the stream
        b = bytearray(body)
        b[stride - shift] = b[stride - shift - 1]  # (a) at the first piece start
        b[2 * stride - shift + 4] = b[2 * stride - shift + 5] = ord("c")  # (b) inside the overlap of the second
        b[3 * stride - shift] = ord("N")  # (c)
        part = (marker + b"read 1 of a long-read file\n" if titled else b"") + bytes(b)
        w = check_hc(hostlib, part, ft, k, line_cap, long_read=True)
        assert w["n_reads"] == shift and w["pieces"] == 5
    # (a) and (b) alone on a run-free base, against "compress, then cut"
    for name, at in (("a", 0), ("b", 5)):
        base = _norun(rng, stride + 700)
        part = base[:stride + at + 1] + base[stride + at:stride + at + 1] + base[stride + at + 1:] if at else base[:stride] + base[stride - 1:stride] + base[stride:]
        per_piece = check_hc(hostlib, part, ft, k, line_cap, long_read=True)
        whole = oracle_of_returns(compress_then_cut(S1.encode([part])[0], k, line_cap), 0, k, 9, 37, smap)
        assert not same_result(per_piece, whole), name
    check_hc(hostlib, marker + b"t\r\n" + bytes(body[:3000]), ft, k, line_cap, long_read=True)
    check_hc(hostlib, bytes(body[:500]) + b"\n", ft, k, line_cap, long_read=True)  # the last part of a FASTQ read
    assert int(check_hc(hostlib, b"AAAAAAAACCCC", ft, k, line_cap, long_read=True)["kmers"].sum()) == 0


# ---- 5
@pytest.mark.parametrize("k,both", [(27, True), (21, False), (55, True)])
def test_multiline_parts_are_compressed_return_by_return(hostlib, k, both):
    rng = np.random.default_rng(90 + k)
    cases, line_cap = multiline_cases(k)
    stride = line_cap - k + 1
    rich = lambda n: synth.homopolymer_rich_sequence(rng, n, 1.8, 0.2, 2000, 9).tobytes()
    long_seq = bytearray(rich(3 * stride + 777))
    long_seq[stride] = long_seq[stride - 1]
    long_seq[2 * stride + 3] = long_seq[2 * stride + 4] = ord("g")
    text = b">long\n" + _wrap(bytes(long_seq), 60, b"\n") + b">e1\n>e2\r\n>cap\n" + _wrap(rich(line_cap), 60, b"\n") + b">short\n" + _wrap(rich(50), 60, b"\n") + \
        b">poly\n" + _wrap(b"A" * 500, 60, b"\n")
    parts = reader_parts(text, 12000, k)
    assert len(parts) >= 2 and any(p[:1] != b">" for p in parts)  # a part that starts inside a sequence
    pieces = 0
    for part in parts:
        pieces += check_hc(hostlib, part, 2, k, line_cap, both=both)["pieces"]
    assert pieces > len(parts) + 4
    for name in ("empty_records", "lower_and_n", "80col_crlf"):
        for part in reader_parts(cases[name], 700, k):
            check_hc(hostlib, part, 2, k, line_cap, both=both)
    w = check_hc(hostlib, rich(2 * stride + 100) + b">next one\n" + rich(300), 2, k, line_cap, both=both)  # no title in front: sequence 0 starts at 0
    assert w["n_reads"] == 1 and w["pieces"] == 4


# ---- 7: the product binary over the emulated library
def _write_reads(path, fmt, seed, n_reads):
    rng = np.random.default_rng(seed)
    synth.make_long_reads(path, seed, [int(x) for x in rng.integers(30, 400, size=n_reads)], fmt=fmt, mean_run=1.8, lower_frac=0.2, n_run_per_mbp=3000, n_run_len=4)


def _write_multiline(path, seed, n_reads):
    rng = np.random.default_rng(seed)
    with open(path, "wb") as f:
        for i in range(n_reads):
            f.write(b">ctg%d\n" % i + _wrap(synth.homopolymer_rich_sequence(rng, int(rng.integers(30, 400)), 1.8, 0.2).tobytes(), 60, b"\n"))


_state = {"broken": False}


@pytest.mark.parametrize("flags,fmt", [(["-k27", "-ci1"], "fq"), (["-k21"], "fa"), (["-k55"], "fq"), (["-k27", "-b"], "fq"), (["-k27", "-fm"], "ml")],
                         ids=["k27ci1", "k21-fa", "k55", "k27b", "k27fm"])
def test_kmc_hip_s1_hc_over_the_emulated_library_writes_the_reference_database(flags, fmt, tmp_path):
    _require("kmc", "kmc_hip_s1")
    if _state["broken"]:
        pytest.fail("an earlier run of kmc_hip_s1 -hc over the emulated library failed")
    inp = str(tmp_path / ("in." + fmt))
    if fmt == "ml":
        _write_multiline(inp, 11, 300)
    else:
        _write_reads(inp, fmt, 12, 300)
    common = flags + (["-fa"] if fmt == "fa" else []) + ["-hc", "-m2", "-sf1", "-n64"]
    rc, want, log = _run("kmc", common + ["-sp1", "-sr1"], inp, tmp_path, "ref")
    assert rc == 0, log[-1500:]
    rc, got, log = _run("kmc_hip_s1", common + ["-sp2", "-sr2"], inp, tmp_path, "emu", env={"KMC_HIP_LIB": emu.build_hostlib("small"), "KMC_HIP_VERBOSE": "1"})
    _state["broken"] = rc != 0
    assert rc == 0, log[-1500:]
    assert got == want and len(want[1]) >= 5
    rep = re.findall(r"(\d+) uncovered parts", log)
    assert rep and sum(int(u) for u in rep) == 0 and "homopolymer-compressed" in log, log[-1500:]
    rc, plain, _ = _run("kmc", [f for f in common if f != "-hc"] + ["-sp1", "-sr1"], inp, tmp_path, "plain")
    assert rc == 0 and plain[0] != want[0]  # -hc does change this input's database


def test_kmc_hip_s1_hc_over_a_library_without_the_query_is_refused(tmp_path):
    """the mock library has no kmc_hip_split_covers, and would ignore the flag silently: the worker refuses the job as before"""
    _require("kmc_hip_s1")
    fq = str(tmp_path / "in.fq")
    _write_reads(fq, "fq", 13, 50)
    rc, _, log = _run("kmc_hip_s1", ["-k27", "-hc", "-m2", "-sf1", "-sp1", "-sr1"], fq, tmp_path, "mock", env={"KMC_HIP_LIB": emu.build_mock()})
    assert rc != 0 and "does not cover homopolymer compression" in log, log[-800:]
