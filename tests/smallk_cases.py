"""Shared by tests/test_stage1_smallk_emulated.py (the product's host library over the emulated HIP runtime) and tests/test_gpu_stage1_smallk.py (libkmc_hip.so):
the numpy restatement of CSplitter::ProcessReadsSmallK (splitter.cpp:682-805), the ctypes binding of kmc_hip_smallk_*, and the per-part cases.

The restatement, over the buffers CSplitter::GetSeq returns (the Python GetSeq restatements of the -hc / -fm tests): with -hc every return is compressed on
its own first; every window of k codes without an invalid one is a k-mer; it is counted as min(forward, reverse complement) as 2k-bit integers with
both_strands, as the forward k-mer without. tests/golden/smallk_counts.json (tests/make_smallk_golden.py: kmc_dump of the reference's own databases) pins it."""
import ctypes as C

import numpy as np

from kmc_amd import capi, synth
from test_stage1_emulated import _records_text
from test_stage1_hc_emulated import HcLib, _rnd, getseq_returns, hc_compress, seam_reads
from test_stage1_multiline_emulated import _wrap, reader_parts

EINVAL, UNCOVERED = -1, 1
_U = np.uint64
_CODE = np.full(256, -1, dtype=np.int8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _CODE[_ch + 32] = _i


def codes_of(seq):
    return _CODE[np.frombuffer(seq, dtype=np.uint8)]


# ---- the restatement
def smallk_kmers(q, k, both):
    """q: the codes of one GetSeq return (negative = invalid; a piece mark, if any, is masked off) -> the k-mer counted for every window of k valid codes"""
    q = np.asarray(q, dtype=np.int8)
    nw = q.size - k + 1
    if nw <= 0:
        return np.zeros(0, dtype=np.uint64)
    bad = np.concatenate([[0], np.cumsum(q < 0)])
    ok = bad[k:] == bad[:-k]
    c = (q & 3).astype(np.uint64)
    f, r = np.zeros(nw, dtype=np.uint64), np.zeros(nw, dtype=np.uint64)
    for j in range(k):
        w = c[j:j + nw]
        f = (f << _U(2)) | w
        r |= (_U(3) - w) << _U(2 * j)
    return (np.minimum(f, r) if both else f)[ok]


def smallk_nonzero(returns, k, both, hc=False):
    """-> (k-mers, counts): the non-zero entries of the 4^k table, ascending; and the number of windows"""
    keys = [smallk_kmers(hc_compress(np.where(q < 0, np.int8(-1), q & 3)) if hc else q, k, both) for q in returns]
    keys = np.concatenate(keys) if keys else np.zeros(0, dtype=np.uint64)
    ent, cnt = np.unique(keys, return_counts=True)
    return ent.astype(np.uint64), cnt.astype(np.uint64), int(keys.size)


def smallk_table(returns, k, both, hc=False):
    out = np.zeros(1 << (2 * k), dtype=np.uint64)
    ent, cnt, total = smallk_nonzero(returns, k, both, hc)
    out[ent.astype(np.intp)] = cnt
    return out, total


# ---- the product's library
class SmallKLib(HcLib):
    """kmc_hip_smallk_open / _part / _read / _close next to kmc_hip_split_part"""

    def __init__(self, path):
        super().__init__(path)
        L = self.L
        L.kmc_hip_smallk_open.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32]
        L.kmc_hip_smallk_part.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.kmc_hip_smallk_read.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]
        L.kmc_hip_smallk_close.argtypes = [C.c_void_p, C.c_int]

    def open(self, k, both):
        return self.L.kmc_hip_smallk_open(self.h, 0, k, 1 if both else 0)

    def close_table(self):
        assert self.L.kmc_hip_smallk_close(self.h, 0) == 0

    def reopen(self, k, both):
        self.close_table()
        assert self.open(k, both) == 0, self.L.kmc_hip_last_error(self.h)

    def part(self, text, k, both, file_type, line_cap, part_kind=0, flags=0, slot=0, signature_len=0, n_bins=0, max_x=0):
        """-> (rc, n_reads, n_kmers)"""
        p = capi.SplitParams(k, signature_len, n_bins, max_x, 1 if both else 0, file_type, line_cap, part_kind, flags)
        t = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(0, dtype=np.uint8)
        n_reads, n_kmers = C.c_uint64(0), C.c_uint64(0)
        rc = self.L.kmc_hip_smallk_part(self.h, 0, slot, C.byref(p), t.ctypes.data if t.size else None, t.size, C.byref(n_reads), C.byref(n_kmers))
        return rc, n_reads.value, n_kmers.value

    def read(self, first, count):
        out = np.full(max(count, 1), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        rc = self.L.kmc_hip_smallk_read(self.h, 0, first, count, out.ctypes.data)
        assert rc == 0, self.L.kmc_hip_last_error(self.h)
        return out[:count]

    def read_all(self, k):
        return self.read(0, 1 << (2 * k))

    def read_nonzero(self, k, chunk=1 << 22):
        """(k-mers, counts) of the non-zero entries, read in chunks"""
        ent, cnt = [], []
        for first in range(0, 1 << (2 * k), chunk):
            a = self.read(first, min(chunk, (1 << (2 * k)) - first))
            nz = np.flatnonzero(a)
            ent.append(nz.astype(np.uint64) + _U(first))
            cnt.append(a[nz])
        return np.concatenate(ent), np.concatenate(cnt)


def check_part(lib, text, file_type, k, both, line_cap, long_read=False, hc=False, returns=None, n_reads=None):
    """a fresh table, one part, against the restatement: the whole table at k <= 9, the non-zero entries beyond; n_reads and n_kmers -> the GetSeq returns"""
    lib.reopen(k, both)
    rc, got_reads, got_kmers = lib.part(text, k, both, file_type, line_cap, 1 if long_read else 0, capi.SPLIT_HOMOPOLYMER if hc else 0)
    assert rc == 0, (rc, lib.L.kmc_hip_last_error(lib.h))
    if callable(returns):
        returns, n_reads = returns(both)
    elif returns is None:
        returns, n_reads = getseq_returns(text, file_type, k, line_cap, long_read)
    ent, cnt, total = smallk_nonzero(returns, k, both, hc)
    assert got_reads == n_reads and got_kmers == total, (got_reads, n_reads, got_kmers, total)
    if k <= 9:
        want = np.zeros(1 << (2 * k), dtype=np.uint64)
        want[ent.astype(np.intp)] = cnt
        got = lib.read_all(k)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    else:
        g_ent, g_cnt = lib.read_nonzero(k)
        assert np.array_equal(g_ent, ent) and np.array_equal(g_cnt, cnt)
    return returns


# ---- inputs
def seam_text(k, fmt, eol):
    """seam_reads(k) fills three tiles and a bit; the read behind them has an N three codes into the halo of the fourth tile. FASTA: the last read without
    its end of line, so that a window ends on the last code of the stream"""
    reads = seam_reads(k)
    at = sum(len(x) + 1 for x in reads)
    body = bytearray(_rnd(np.random.default_rng(k), 4 * 4096 - at + k + 50))
    body[4 * 4096 - at + 3] = ord("N")
    reads.append(bytes(body))
    text = _records_text(fmt, eol, reads)
    return text[:len(text) - len(eol)] if fmt == "fa" else text


def format_cases(k, seed=0):
    """[(name, text, file_type, line_cap, long_read, returns(both) or None, None)]: a line beyond line_cap in pieces, a long-read part with and without title,
    multi-line parts from reader_parts, one BAM part"""
    rng = np.random.default_rng(700 + 10 * k + seed)
    line_cap = k + 4105
    stride = line_cap - k + 1
    rich = lambda n: synth.homopolymer_rich_sequence(rng, n, 1.8, 0.2, 2000, 9).tobytes()
    cases = []
    lines = [rich(300), rich(line_cap), rich(2 * stride + 345), b"A" * (line_cap + 200), rich(line_cap - 1), _rnd(rng, 200)]
    cases.append(("pieces", _records_text("fa", b"\n", lines), 0, line_cap, False, None, None))
    body = rich(2 * stride + 1234)
    cases.append(("long-titled", b"@read 1 of a long-read file\n" + body, 1, line_cap, True, None, None))
    cases.append(("long-untitled", body, 0, line_cap, True, None, None))
    seq = rich(2 * stride + 777)
    text = b">long\n" + _wrap(seq, 60, b"\n") + b">e1\n>e2\r\n>short\n" + _wrap(_rnd(rng, 50), 60, b"\n") + b">poly\n" + _wrap(b"A" * 500, 60, b"\n")
    parts = reader_parts(text, 9000, k)
    assert len(parts) >= 2 and any(p[:1] != b">" for p in parts)
    for i, part in enumerate(parts):
        cases.append(("multiline-%d" % i, part, 2, line_cap, False, None, None))
    reads = [(synth.homopolymer_rich_sequence(rng, int(rng.integers(1, 400)), 2.0).tobytes().decode(), int(rng.choice([0, 0x10, 0x100]))) for _ in range(50)]
    reads.append(("ACGTNNRYACGT" * 20, 0x10))
    bam = synth.bam_part([synth.bam_record(s, f, b"r%d" % i, n_cigar=i % 3) for i, (s, f) in enumerate(reads)])
    def bam_returns(both):  # the stored sequence, reversed and complemented for flag 0x10 without both_strands; records with 0x100 / 0x800 skipped
        seqs, n = synth.bam_reads_as_getseq(reads, both)
        return [codes_of(x) for x in seqs], n

    cases.append(("bam", bam, capi.SPLIT_FILE_BAM, 1 << 17, False, bam_returns, None))
    return cases


# ---- kmc_hip_s1 against kmc
E2E_SETS = [(["-k13", "-ci1"], "fq"), (["-k9", "-hc"], "fq"), (["-k5", "-b", "-fa"], "fa"), (["-k12", "-fm"], "ml"), (["-k4", "-okff"], "fq")]
E2E_IDS = ["k13ci1", "k9hc", "k5b-fa", "k12fm", "k4kff"]
REPORT = r"small k on the device: (\d+) parts, (\d+) k-mers"


def run_kmc(exe, flags, inp, tmp_path, tag, env=None, timeout=1500):
    """-> (rc, (md5 of every database file written, the statistics lines), stdout + stderr)"""
    import hashlib
    import os
    import subprocess

    t = tmp_path / ("tmp_" + tag)
    t.mkdir(exist_ok=True)
    db = str(tmp_path / ("db_" + tag))
    r = subprocess.run([exe, *flags, inp, db, str(t)], capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=timeout)
    if r.returncode != 0:
        return r.returncode, None, r.stdout + r.stderr
    files = [db + e for e in (".kmc_pre", ".kmc_suf", ".kff") if os.path.exists(db + e)]
    md5 = tuple((os.path.basename(f).split(".", 1)[1], hashlib.md5(open(f, "rb").read()).hexdigest()) for f in files)
    stats = [ln.split(":")[1].strip() for ln in r.stdout.splitlines() if "No. of" in ln or "Total no." in ln]
    return 0, (md5, stats), r.stdout + r.stderr


def check_e2e(kmc, kmc_hip_s1, flags, inp, tmp_path, hip_env, timeout=1500, on_device=True):
    """kmc and kmc_hip_s1 on one input with the issue's flags (-m2 -sf1 -sp2): the same database bytes and statistics lines, the reference says
    "Small k optimization on!", the product's log carries the report line with parts counted on the device (or, on_device=False, none at all)"""
    import re

    common = flags + ["-v", "-m2", "-sf1", "-sp2", "-sr2"]
    rc, want, ref_log = run_kmc(kmc, common, inp, tmp_path, "ref", timeout=timeout)
    assert rc == 0, ref_log[-1500:]
    assert "Small k optimization on!" in ref_log
    rc, got, log = run_kmc(kmc_hip_s1, common, inp, tmp_path, "hip", env=dict(hip_env, KMC_HIP_VERBOSE="1"), timeout=timeout)
    assert rc == 0, log[-1500:]
    assert len(want[0]) in (1, 2) and got[0] == want[0], (got[0], want[0])  # .kmc_pre and .kmc_suf, or .kff, byte for byte
    assert got[1] == want[1] and len(want[1]) >= 5, (got[1], want[1])
    sk = [ln for ln in ref_log.splitlines() if "super-k-mers" in ln]
    assert sk and sk[0].split(":")[1].strip() == "0", sk
    rep = re.findall(REPORT, log)
    if not on_device:
        assert not rep, log[-1500:]
        return want, got
    total = [ln.split(":")[1].strip() for ln in ref_log.splitlines() if "Total no. of k-mers" in ln]
    assert rep and sum(int(p) for p, _ in rep) > 0 and total and sum(int(n) for _, n in rep) == int(total[0]), (rep, total, log[-1500:])
    return want, got
