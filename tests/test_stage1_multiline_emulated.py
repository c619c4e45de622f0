"""CPU: stage 1 on the device for multi-line FASTA (-fm) — kmc_hip_split_part with file_type 2 (k_s1_ml_text_to_codes, k_s1_ml_marks and the
rest of kmc_amd/csrc/stage1_chain.h) in the PRODUCT'S host library compiled over the emulated HIP runtime (tests/emu.py build_hostlib), against a
Python restatement of the reference's reader and of CSplitter::GetSeq's multi-line branch fed to the stage-1 oracle; and the product binary
kmc_hip_s1 -fm over that library against the reference's kmc -fm."""
import ctypes as C
import os

import numpy as np
import pytest

import emu
import oracle_s1 as S1
from kmc_amd import synth
from test_stage1_emulated import _parse_bin, _sig_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOL = (10, 13)
_CODES = np.full(256, -1, dtype=np.int8)  # splitter.cpp:42-47
for _c, _v in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
    _CODES[_c] = _v


# ---- the reference, restated
def reader_parts(data: bytes, part_size: int, k: int):
    """CFastqReader::GetPartFromMultilneFasta (fastq_reader.cpp:399-468) over one plain file: blocks of part_size - 1 - carried bytes (:410); a fake end
    of line at the end of the file (FixEOLIfNeeded :471-483); every title is kept with the whole run of end-of-line bytes behind it (SkipNextEOL
    :917-929), every other '\\n' / '\\r' is removed (:427-448); the part ends in front of its last title, which is carried over (:460-466), or — one
    sequence only — the part is all of it and its last k - 1 symbols are carried over (:451-458)."""
    parts, carried, at, contains_next, finished = [], b"", 0, False, False
    while True:
        if not contains_next and finished:  # data_src.Finished() (:403-407)
            return parts
        room = part_size - 1 - len(carried)
        chunk = data[at:at + room]
        at += len(chunk)
        last_in_file = len(chunk) < room  # the source ran dry inside this read
        finished = finished or last_in_file
        buf = bytearray(carried + chunk)
        if last_in_file and buf and buf[-1] not in EOL:
            buf.append(10)
        total, out, last_header, i = len(buf), bytearray(), 0, 0
        while i < total:
            stop = False
            while i < total and buf[i] == ord(">"):
                tmp, j = i, i  # SkipNextEOL: the first end of line that is followed by something else
                while j < total - 1 and not (buf[j] in EOL and buf[j + 1] not in EOL):
                    j += 1
                next_line = j < total - 1
                i = j + 1 if next_line else total
                last_header = len(out)
                out += buf[tmp:i]
                if not next_line:
                    stop = True
                    break
            if stop:
                break  # (the reference then reads the byte behind the buffer: outside what a test can restate)
            if buf[i] not in EOL:
                out.append(buf[i])
            i += 1
        if last_header == 0:
            keep = k - 1
            if len(out) < keep or last_in_file:
                keep = 0
            parts.append(bytes(out))
            carried = bytes(out[len(out) - keep:]) if keep else b""
            contains_next = False
        else:
            parts.append(bytes(out[:last_header]))
            carried = bytes(out[last_header:])
            contains_next = True


def getseq_multiline(part: bytes, k: int, line_cap: int):
    """CSplitter::GetSeq, branch InputType::MULTILINE_FASTA (splitter.cpp:304-323), called until it returns false (ProcessReads :574) -> (pieces as code
    arrays, n_reads)"""
    pieces, n_reads, pp, size = [], 0, 0, len(part)
    while pp < size:  # :97-98
        if part[pp] == ord(">"):  # :306-313
            n_reads += 1
            while pp < size and part[pp] not in EOL:
                pp += 1
            pp += 1
            if pp < size and part[pp] in EOL:
                pp += 1
        lo = pp
        while pp < size and pp - lo < line_cap and part[pp] != ord(">"):  # :314-317
            pp += 1
        pieces.append(_CODES[np.frombuffer(part[lo:pp], dtype=np.uint8)] if pp > lo else np.zeros(0, dtype=np.int8))
        if pp < size and part[pp] != ord(">"):  # :319-322: the cap stopped it
            pp -= k - 1
    return pieces, n_reads


def oracle_part(part, k, m, n_bins, smap, line_cap, max_x=3, both=True):
    """what ProcessReads + the collectors make of the part: records per bin, the three sums, n_reads"""
    pieces, n_reads = getseq_multiline(part, k, line_cap)
    want = dict(bins=[[] for _ in range(n_bins)], kmers=np.zeros(n_bins, dtype=np.uint64), supers=np.zeros(n_bins, dtype=np.uint64),
                plus_x=np.zeros(n_bins, dtype=np.uint64), n_reads=n_reads, pieces=len(pieces))
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)
    for q in pieces:
        if q.size < k:
            continue
        sig, off, recs = S1.split([letters[np.where(q < 0, 4, q)].tobytes()], k, m)
        pos, ln, sg = S1.split_stream(q, k, m)
        assert np.array_equal(sig, sg)
        for i in range(sig.size):
            b = int(smap[sig[i]])
            want["bins"][b].append(bytes(recs[int(off[i]):int(off[i + 1])]))
            want["kmers"][b] += int(ln[i]) - k + 1
            want["supers"][b] += 1
            want["plus_x"][b] += S1.kxmer_recs(q[int(pos[i]):int(pos[i] + ln[i])], k, max_x, both)
    return want


# ---- the product's library
class SplitParams(C.Structure):
    _fields_ = [("kmer_len", C.c_uint32), ("signature_len", C.c_uint32), ("n_bins", C.c_uint32), ("max_x", C.c_uint32), ("both_strands", C.c_uint32),
                ("file_type", C.c_uint32), ("line_cap", C.c_uint64), ("part_kind", C.c_uint32), ("reserved", C.c_uint32)]


class SplitLib:
    """kmc_hip_split_part of a library (the emulated product library here, libkmc_hip.so in the -m gpu file)"""

    def __init__(self, path):
        self.L = L = C.CDLL(path)
        L.kmc_hip_last_error.restype = C.c_char_p
        L.kmc_hip_last_error.argtypes = [C.c_void_p]
        L.kmc_hip_split_set_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
        L.kmc_hip_split_part.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7
        L.kmc_hip_split_covers.argtypes = [C.c_uint32]
        self.h = C.c_void_p()
        assert L.kmc_hip_init(None, 1, C.byref(self.h)) == 0

    def close(self):
        self.L.kmc_hip_destroy(self.h)

    def split_part(self, text, k, m, n_bins, smap, line_cap, file_type=2, part_kind=0, max_x=3, both=True):
        L = self.L
        assert L.kmc_hip_split_set_map(self.h, 0, smap.ctypes.data, m) == 0
        p = SplitParams(k, m, n_bins, max_x, 1 if both else 0, file_type, line_cap, part_kind, 0)
        t = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(0, dtype=np.uint8)
        recs = np.zeros(2 * t.size + 256 * (n_bins + 1) + 4096, dtype=np.uint8)
        arr = [np.zeros(n_bins, dtype=np.uint64) for _ in range(5)]
        need, n_reads = C.c_uint64(0), C.c_uint64(0)
        rc = L.kmc_hip_split_part(self.h, 0, 0, C.byref(p), t.ctypes.data, t.size, recs.ctypes.data, recs.size, C.byref(need),
                                  *[a.ctypes.data for a in arr], C.byref(n_reads))
        if rc:
            return rc, L.kmc_hip_last_error(self.h)
        off, nbytes, kmers, supers, plus_x = arr
        return 0, dict(bins=[recs[int(off[b]):int(off[b] + nbytes[b])].copy() for b in range(n_bins)], kmers=kmers, supers=supers, plus_x=plus_x,
                       n_reads=n_reads.value)


def check_part(lib, text, k, line_cap, m=9, n_bins=37, max_x=3, both=True):
    smap = _sig_map(m, n_bins, 5)
    rc, got = lib.split_part(text, k, m, n_bins, smap, line_cap, max_x=max_x, both=both)
    assert rc == 0, got
    want = oracle_part(text, k, m, n_bins, smap, line_cap, max_x, both)
    assert got["n_reads"] == want["n_reads"]
    for b in range(n_bins):
        assert _parse_bin(got["bins"][b], k) == sorted(want["bins"][b]), b
    for key in ("kmers", "supers", "plus_x"):
        assert np.array_equal(got[key], want[key]), key
    return want


def _rnd(rng, n, alphabet=b"ACGT"):
    a = np.frombuffer(alphabet, dtype=np.uint8)
    return a[rng.integers(0, a.size, size=n)].tobytes()


def _wrap(seq, width, eol):
    return b"".join(seq[i:i + width] + eol for i in range(0, len(seq), width))


def multiline_cases(k):
    """(name, text of a file) covering what the issue of this format lists; the reader's restatement cuts them into parts"""
    rng = np.random.default_rng(k)
    line_cap = k + 4105
    soft = lambda n: bytes(c | 0x20 if (i // 37) % 3 == 0 else c for i, c in enumerate(_rnd(rng, n)))
    cases = {
        "60col": b"".join(b">chr%d assembled\n" % i + _wrap(_rnd(rng, int(rng.integers(100, 900))), 60, b"\n") for i in range(6)),
        "80col_crlf": b"".join(b">ctg%d\r\n" % i + _wrap(_rnd(rng, int(rng.integers(100, 700))), 80, b"\r\n") for i in range(5)),
        "blank_after_title": b">a\n\n" + _wrap(_rnd(rng, 300), 60, b"\n") + b">b\r\n\r\n" + _wrap(_rnd(rng, 200), 60, b"\n") + b">c\n\n\n" + _wrap(_rnd(rng, 150), 60, b"\n"),
        "title_with_gt": b">x>y >z\n" + _wrap(_rnd(rng, 400), 70, b"\n") + b">>\n" + _wrap(_rnd(rng, 120), 70, b"\n"),
        "empty_records": b">e1\n>e2\n" + _wrap(_rnd(rng, 200), 60, b"\n") + b">e3\n>e4\r\n>e5\n" + _wrap(_rnd(rng, 90), 60, b"\n") + b">e6\n",
        "lower_and_n": b">m\n" + _wrap(soft(500) + b"N" * 70 + soft(300) + b"n" * 5 + _rnd(rng, 200, b"ACGTNRY"), 60, b"\n"),
        "long_sequence": b">long\n" + _wrap(_rnd(rng, 3 * (line_cap - k + 1) + 777), 60, b"\n") + b">cap\n" + _wrap(_rnd(rng, line_cap), 60, b"\n")
        + b">short\n" + _wrap(_rnd(rng, 50), 60, b"\n"),
        "tiny_records": b"".join(b">amp%d\n" % i + _rnd(rng, int(rng.integers(0, 40))) + b"\n" for i in range(600)),
    }
    return cases, line_cap


@pytest.fixture(scope="module")
def hostlib():
    lib = SplitLib(emu.build_hostlib("small"))
    yield lib
    lib.close()


def test_the_library_says_it_covers_multiline_fasta(hostlib):
    assert hostlib.L.kmc_hip_abi_version() == 4
    assert [hostlib.L.kmc_hip_split_covers(t) for t in (0, 1, 2, 3)] == [1, 1, 1, 0]


@pytest.mark.parametrize("case", ["60col", "80col_crlf", "blank_after_title", "title_with_gt", "empty_records", "lower_and_n", "long_sequence", "tiny_records"])
def test_multiline_parts_match_getseq(hostlib, case):
    """every part the reader makes of the file (parts of ~700 B: several titles per part, parts ending in front of a title, parts that start inside a
    sequence) through kmc_hip_split_part file_type 2 against GetSeq + ProcessReads + the collectors"""
    k = 27
    cases, line_cap = multiline_cases(k)
    text = cases[case]
    parts = reader_parts(text, 700 if case != "long_sequence" else 12000, k)
    assert len(parts) >= 2
    pieces = 0
    for part in parts:
        pieces += check_part(hostlib, part, k, line_cap)["pieces"]
    if case == "long_sequence":
        assert any(p[:1] != b">" for p in parts)  # the sequence went on across parts
        assert pieces > len(parts) + 1  # the cap cut pieces


@pytest.mark.parametrize("k,both,max_x", [(21, True, 3), (55, False, 0), (27, True, 1)])
def test_whole_records_in_one_part(hostlib, k, both, max_x):
    """whole files as one part, other k / strand / k+x settings; one sequence longer than a small line cap, so that piece marks are set"""
    cases, line_cap = multiline_cases(k)
    for name in ("80col_crlf", "long_sequence", "empty_records"):
        check_part(hostlib, cases[name], k, line_cap, both=both, max_x=max_x)


def test_a_part_starting_inside_a_sequence(hostlib):
    """the reader's continuation: no title, the previous part's last k - 1 symbols in front"""
    k = 27
    rng = np.random.default_rng(4)
    line_cap = k + 4105
    w = check_part(hostlib, _rnd(rng, 2 * (line_cap - k + 1) + 100) + b">next one\n" + _rnd(rng, 300), k, line_cap)
    assert w["n_reads"] == 1 and w["pieces"] == 4
    w = check_part(hostlib, _rnd(rng, 5000, b"ACGTacgtN"), k, line_cap)
    assert w["n_reads"] == 0


def test_titles_beyond_the_line_arrays_of_single_line_fasta(hostlib):
    """the per-title arrays are sized by titles (a title takes 2 bytes), not by the size / 4 + 1024 lines of single-line FASTA: tiny records
    everywhere (the -m gpu file runs a million 20 bp amplicons in one part)"""
    text = b"".join(b">\n" + b"ACGTTGCA"[: i % 3] for i in range(15000)) + b">\n" + b"ACGT" * 20
    assert text.count(b">") > len(text) // 4 + 1024
    check_part(hostlib, text, 27, 27 + 4105)


def test_unterminated_title_is_uncovered_and_bad_arguments_are_refused(hostlib):
    k = 27
    smap = _sig_map(9, 8, 1)
    rc, _ = hostlib.split_part(b">t\nACGTACGT" * 3 + b">a title that never ends", k, 9, 8, smap, k + 4105)
    assert rc == 1  # KMC_HIP_UNCOVERED
    rc, _ = hostlib.split_part(b">only a title", k, 9, 8, smap, k + 4105)
    assert rc == 1
    rc, msg = hostlib.split_part(b">t\nACGT\n", k, 9, 8, smap, k + 4105, part_kind=1)
    assert rc == -1 and b"part_kind" in msg  # KMC_HIP_EINVAL
    rc, _ = hostlib.split_part(b">t\nACGT\n", k, 9, 8, smap, k + 4105, file_type=3)
    assert rc == -1
    assert hostlib.split_part(b">t\n", k, 9, 8, smap, k + 4105)[1]["n_reads"] == 1  # a title at the very end, terminated: one read, nothing else


# ---- the product binary over the emulated library
def _exe(name):
    return os.path.join(ROOT, "kmc_amd", "bin", name) if name.startswith("kmc_hip") else os.path.join(ROOT, "oracle", "_ref", name)


def _run(exe, flags, inp, tmp_path, tag, env=None):
    import hashlib
    import subprocess

    t = tmp_path / ("tmp_" + tag)
    t.mkdir(exist_ok=True)
    db = str(tmp_path / ("db_" + tag))
    r = subprocess.run([_exe(exe), *flags, inp, db, str(t)], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=1500)
    if r.returncode != 0:
        return r.returncode, None, r.stdout + r.stderr
    md5 = tuple(hashlib.md5(open(db + e, "rb").read()).hexdigest() for e in (".kmc_pre", ".kmc_suf"))
    stats = [ln.split(":")[1].strip() for ln in r.stdout.splitlines() if "No. of" in ln or "Total no." in ln]
    return 0, (md5, stats), r.stderr


def _require(*names):
    missing = [n for n in names if not os.path.exists(_exe(n))]
    if missing:
        pytest.skip("needs the reference pipeline binaries (%s not built: the reference source tree was absent at build time)" % ", ".join(missing))


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_kmc_hip_s1_fm_over_the_emulated_library_writes_the_reference_database(eol, tmp_path):
    _require("kmc", "kmc_hip_s1")
    fa = str(tmp_path / "in.fa")
    synth.make_multiline_fasta(fa, seed=7, contig_lens=[60_000, 0, 25_000, 900, 40_000], line_width=60 if eol == b"\n" else 80, lower_frac=0.2,
                               n_run_per_mbp=40, n_run_len=50, n_empty=2, eol=eol)
    common = ["-k27", "-ci1", "-fm", "-m2", "-sf1", "-n64"]
    rc, want, log = _run("kmc", common + ["-sp1", "-sr1"], fa, tmp_path, "ref")
    assert rc == 0, log[-1500:]
    rc, got, log = _run("kmc_hip_s1", common + ["-sp2", "-sr2"], fa, tmp_path, "emu", env={"KMC_HIP_LIB": emu.build_hostlib("small"), "KMC_HIP_VERBOSE": "1"})
    assert rc == 0, log[-1500:]
    assert got == want and len(want[1]) >= 5
    assert "multi-line FASTA parts" in log and "0 uncovered parts" in log


def test_kmc_hip_s1_fm_over_a_library_without_the_query_is_refused(tmp_path):
    """the mock library has no kmc_hip_split_covers: the worker refuses the job as before"""
    _require("kmc_hip_s1")
    fa = str(tmp_path / "in.fa")
    synth.make_multiline_fasta(fa, seed=8, contig_lens=[3000, 2000])
    rc, _, log = _run("kmc_hip_s1", ["-k27", "-fm", "-m2", "-sf1", "-sp1", "-sr1"], fa, tmp_path, "mock", env={"KMC_HIP_LIB": emu.build_mock()})
    assert rc != 0 and "does not cover an input format other than FASTA / FASTQ" in log, log[-800:]
