"""Shared by tests/test_stage1_sigstats_emulated.py (the product's host library over the emulated HIP runtime) and tests/test_gpu_stage1_sigstats.py
(libkmc_hip.so): two oracles of the stage-0 signature statistics, the ctypes binding of kmc_hip_sigstats_*, and the per-part cases.

stats[s] = what CSplitter::CalcStats (splitter.cpp:439-533) adds per signature over the buffers CSplitter::GetSeq returns (compressed one by one with -hc):
  (a) stats_from_superkmers: the existing stage-1 oracle, which the bin tests pin to the reference's bins — oracle_s1.split_stream over every return, then
      np.add.at(stats, signature, len - k + 1);
  (b) stats_calcstats: the CalcStats loop itself restated in Python with CMmer's semantics (a normalised m-mer value per position, the current signature and
      where it starts, a run length that restarts at k - 1), for the small cases.
check_part asks both before it asks the device, and they must agree. The cases are sized from the kernel's own tile (kernel_lib builds tests/hipemu/emu_sigstats.cpp over the kernel
header, tile_constants asks it; nothing is copied here)."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu
import oracle_s1 as S1
from kmc_amd import capi, synth
from test_stage1_emulated import _records_text
from test_stage1_hc_emulated import HcLib, _rnd, getseq_returns, hc_compress
from test_stage1_multiline_emulated import _wrap, reader_parts

EINVAL, UNCOVERED = -1, 1
KM = [(5, 5), (6, 5), (11, 11), (12, 11), (27, 9), (28, 7), (55, 9), (256, 11), (255, 5)]
KM_IDS = ["k%d-m%d" % km for km in KM]
RESTATEMENT_MAX_CODES = 30_000  # (b) walks symbol by symbol in Python


# ---- the kernel alone, and its geometry
_KERNEL_LIBS = {}


def kernel_lib(geometry="small"):
    """tests/hipemu/libkmc_emu_sigstats_<geometry>.so: k_s1_sig_stats under the CPU emulation, launched by tests/hipemu/emu_sigstats.cpp"""
    if geometry not in _KERNEL_LIBS:
        so = os.path.join(emu.EMU_DIR, "libkmc_emu_sigstats_%s.so" % geometry)
        srcs = [os.path.join(emu.EMU_DIR, "emu_sigstats.cpp"), os.path.join(emu.EMU_DIR, "include", "hip", "hip_runtime.h"),
                os.path.join(emu.ROOT, "kmc_amd", "csrc", "kernels.hip.h"), os.path.join(emu.ROOT, "kmc_amd", "csrc", "stage1_kernels.hip.h")]
        if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in srcs):
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-pthread", "-w", "-fno-gnu-unique", "-fvisibility=hidden", "-Wl,-Bsymbolic",
                                   *emu.GEOMETRY_FLAGS[geometry], "-I", os.path.join(emu.EMU_DIR, "include"), srcs[0], "-o", so])
        L = C.CDLL(so)
        L.emu_s1_sig_stats.restype = C.c_uint64
        L.emu_s1_sig_stats.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int]
        L.emu_s1_sig_stats_geometry.argtypes = [C.c_void_p]
        _KERNEL_LIBS[geometry] = L
    return _KERNEL_LIBS[geometry]


def tile_constants(geometry="small") -> dict:
    """S1_STATS_TILE (start positions per workgroup tile), S1_STATS_PER (per thread strip), S1_STATS_LDS_M (largest m with an LDS table), S1_WG_TILE of the build"""
    g = (C.c_uint32 * 4)()
    kernel_lib(geometry).emu_s1_sig_stats_geometry(g)
    return dict(zip(("tile", "per", "lds_m", "wg_tile"), (int(x) for x in g)))


# ---- the oracles
def _plain(q):
    """a GetSeq return as codes 0..3 / -1 (a piece mark, if any, masked off)"""
    q = np.asarray(q, dtype=np.int8)
    return np.where(q < 0, np.int8(-1), q & 3).astype(np.int8)


def prepared_returns(returns, hc=False):
    return [hc_compress(_plain(q)) if hc else _plain(q) for q in returns]


def stats_from_superkmers(returns, k, m, hc=False) -> np.ndarray:
    """(a)"""
    stats = np.zeros(4**m + 1, dtype=np.uint32)
    for q in prepared_returns(returns, hc):
        if q.size < k:
            continue
        _, ln, sg = S1.split_stream(q, k, m)
        np.add.at(stats, sg, (ln.astype(np.int64) - k + 1).astype(np.uint32))
    return stats


def stats_calcstats(returns, k, m, hc=False) -> np.ndarray:
    """(b)"""
    norm, mask = S1.norm_table(m), 4**m - 1
    stats = np.zeros(4**m + 1, dtype=np.int64)

    def packed(seq, at):
        v = 0
        for c in seq[at:at + m]:
            v = (v << 2) | c
        return v

    for q in prepared_returns(returns, hc):
        seq, n = [int(c) for c in q], int(q.size)
        i = run = 0
        cur = None  # the current signature's normalised value
        while i + k - 1 < n:
            bad = next((j for j in range(m) if seq[i + j] < 0), None)  # the first m-mer after an invalid symbol or at the start of the buffer
            if bad is not None:
                i += bad + 1
                continue
            i += m
            run, start = m, i - m
            end_str = packed(seq, start)
            cur = int(norm[end_str])
            broke = False
            while i < n:
                if seq[i] < 0:
                    if run >= k:
                        stats[cur] += 1 + run - k
                    run, i, broke = 0, i + 1, True
                    break
                end_str = ((end_str << 2) | seq[i]) & mask
                end = int(norm[end_str])
                if end < cur:  # a smaller signature at the end of the current k-mer
                    if run >= k:
                        stats[cur] += 1 + run - k
                        run = k - 1
                    cur, start = end, i - m + 1
                elif end == cur:
                    start = i - m + 1
                elif start + k - 1 < i:  # the signature left the k-mer: the smallest of what is inside, the last one among equals
                    assert run >= k
                    stats[cur] += 1 + run - k
                    run = k - 1
                    start += 1
                    end_str = packed(seq, start)
                    cur = int(norm[end_str])
                    for j in range(start + m, i + 1):
                        end_str = ((end_str << 2) | seq[j]) & mask
                        if int(norm[end_str]) <= cur:
                            cur, start = int(norm[end_str]), j - m + 1
                run += 1
                i += 1
            if not broke:
                break
        if run >= k:
            stats[cur] += 1 + run - k
    return (stats & 0xFFFFFFFF).astype(np.uint32)


def oracle_stats(returns, k, m, hc=False) -> np.ndarray:
    """both oracles where (b) is affordable; they must agree"""
    a = stats_from_superkmers(returns, k, m, hc)
    if sum(int(q.size) for q in returns) <= RESTATEMENT_MAX_CODES:
        b = stats_calcstats(returns, k, m, hc)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, ("the two oracles disagree", k, m, bad[:8], a[bad[:8]], b[bad[:8]])
    return a


# ---- the product's library
class SigStatsLib(HcLib):
    """kmc_hip_sigstats_open / _part / _read / _close next to kmc_hip_split_part"""

    def __init__(self, path):
        super().__init__(path)
        capi.bind_sigstats(self.L)

    def open(self, k, m):
        return self.L.kmc_hip_sigstats_open(self.h, 0, k, m)

    def close_table(self):
        return self.L.kmc_hip_sigstats_close(self.h, 0)

    def reopen(self, k, m):
        assert self.close_table() == 0
        assert self.open(k, m) == 0, self.L.kmc_hip_last_error(self.h)

    def part(self, text, k, m, file_type, line_cap, part_kind=0, flags=0, slot=0, n_bins=0, max_x=0, both=True):
        """-> (rc, n_reads, n_kmers)"""
        p = capi.SplitParams(k, m, n_bins, max_x, 1 if both else 0, file_type, line_cap, part_kind, flags)
        t = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(0, dtype=np.uint8)
        n_reads, n_kmers = C.c_uint64(0), C.c_uint64(0)
        rc = self.L.kmc_hip_sigstats_part(self.h, 0, slot, C.byref(p), t.ctypes.data if t.size else None, t.size, C.byref(n_reads), C.byref(n_kmers))
        return rc, n_reads.value, n_kmers.value

    def read(self, first, count):
        out = np.full(max(count, 1), 0xDEADBEEF, dtype=np.uint32)
        rc = self.L.kmc_hip_sigstats_read(self.h, 0, first, count, out.ctypes.data)
        assert rc == 0, self.L.kmc_hip_last_error(self.h)
        return out[:count]

    def read_all(self, m):
        return self.read(0, 4**m + 1)


def check_part(lib, text, file_type, k, m, line_cap, long_read=False, hc=False, returns=None, n_reads=None, want=None):
    """a fresh table, one part, against the oracles: the whole table, n_kmers == its sum, n_reads -> (stats, returns)"""
    lib.reopen(k, m)
    rc, got_reads, got_kmers = lib.part(text, k, m, file_type, line_cap, 1 if long_read else 0, capi.SPLIT_HOMOPOLYMER if hc else 0)
    assert rc == 0, (rc, lib.L.kmc_hip_last_error(lib.h))
    if callable(returns):
        returns, n_reads = returns(True)
    elif returns is None:
        returns, n_reads = getseq_returns(text, file_type, k, line_cap, long_read)
    if want is None:
        want = oracle_stats(returns, k, m, hc)
    got = lib.read_all(m)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert got_reads == n_reads and got_kmers == int(want.sum(dtype=np.uint64)), (got_reads, n_reads, got_kmers, int(want.sum(dtype=np.uint64)))
    return want, returns


# ---- inputs: one record per part wherever a position of the code stream matters (the stream is then the sequence: position = symbol)
def one_record(seq, fmt="fa", eol=b"\n", final_eol=True):
    text = _records_text(fmt, eol, [seq])
    return text if final_eol else text[:len(text) - len(eol)]


def size_cases(T, k, seed=0):
    """[(name, text, file_type)]: parts of k - 1, k, k + 1 symbols; of T - 1, T, T + 1 and 3T + 5 start positions (no end of line behind the last symbol: the
    stream ends with the last window); a read whose last window starts at a tile's last position; a read whose first code is a tile's last"""
    rng = np.random.default_rng(100 * k + seed)
    out = [("sym_%+d" % d, one_record(_rnd(rng, k + d), "fa", b"\n", d != 0), 0) for d in (-1, 0, 1)]
    for name, pos in (("pos_T-1", T - 1), ("pos_T", T), ("pos_T+1", T + 1), ("pos_3T+5", 3 * T + 5)):
        out.append((name, one_record(_rnd(rng, pos + k - 1), "fa", b"\n", False), 0))
    out.append(("read_ends_at_tile_end", _records_text("fq", b"\n", [_rnd(rng, T + k - 1), _rnd(rng, T // 2 + k)]), 1))  # windows 0 .. T - 1, a separator at T + k - 1
    out.append(("read_starts_at_tile_end", _records_text("fa", b"\n", [_rnd(rng, T - 2), _rnd(rng, T // 2 + k)]), 0))  # codes 0 .. T - 3, separator at T - 2, the next read from T - 1
    return out


def seam_n_text(T, k, d, seed=0):
    """one record of T + 2k + 5 symbols with an N at T + d"""
    body = bytearray(_rnd(np.random.default_rng(7 * k + seed), T + 2 * k + 5))
    body[T + d] = ord("N")
    return one_record(bytes(body))


def repeat_cases(T, k):
    """a 3T-symbol homopolymer of A (every window on the special signature), one of C, an (AC)n and an (AAC)n satellite, each between two random reads"""
    rng = np.random.default_rng(900 + k)
    n = max(3 * T, 2 * k)
    mk = lambda unit: _records_text("fa", b"\n", [_rnd(rng, 2 * k), (unit * (n // len(unit) + 1))[:n], _rnd(rng, 3 * k)])
    return [("poly_A", mk(b"A"), 0), ("poly_C", mk(b"C"), 0), ("sat_AC", mk(b"AC"), 0), ("sat_AAC", mk(b"AAC"), 0)]


def format_cases(T, k, seed=0):
    """[(name, text, file_type, line_cap, long_read, returns(both) or None)]: the four file types, an over-long line and long-read parts (piece marks),
    \\r\\n, lower case, a part without a final end of line"""
    rng = np.random.default_rng(700 + 10 * k + seed)
    line_cap = k + 4105
    stride = line_cap - k + 1
    rich = lambda n: synth.homopolymer_rich_sequence(rng, n, 1.8, 0.2, 2000, 9).tobytes()  # lower case and runs of N inside
    cases = []
    reads = [rich(int(x)) for x in rng.integers(k - 2, 5 * k + 40, size=30)] + [_rnd(rng, T // 3), b"acgtn" * 30 + _rnd(rng, k)]
    cases.append(("fastq", _records_text("fq", b"\n", reads), 1, line_cap, False, None))
    cases.append(("fastq_crlf", _records_text("fq", b"\r\n", reads), 1, line_cap, False, None))
    fa = _records_text("fa", b"\r\n", reads)
    cases.append(("fasta_crlf_no_final_eol", fa[:len(fa) - 2], 0, line_cap, False, None))
    lines = [rich(300), rich(line_cap), rich(2 * stride + 345), b"A" * (line_cap + 200), rich(line_cap - 1), _rnd(rng, 200)]
    cases.append(("pieces", _records_text("fa", b"\n", lines), 0, line_cap, False, None))
    body = rich(2 * stride + 1234)
    cases.append(("long_titled", b"@read 1 of a long-read file\n" + body, 1, line_cap, True, None))
    cases.append(("long_untitled", body, 0, line_cap, True, None))
    seq = rich(2 * stride + 777)
    text = b">long\n" + _wrap(seq, 60, b"\n") + b">e1\n>e2\r\n>short\n" + _wrap(_rnd(rng, 50 + k), 60, b"\n") + b">poly\n" + _wrap(b"A" * (500 + k), 60, b"\n")
    parts = reader_parts(text, 9000, k)
    assert len(parts) >= 2 and any(p[:1] != b">" for p in parts)
    for i, part in enumerate(parts):
        cases.append(("multiline_%d" % i, part, 2, line_cap, False, None))
    breads = [(synth.homopolymer_rich_sequence(rng, int(rng.integers(1, 400 + 2 * k)), 2.0).tobytes().decode(), int(rng.choice([0, 0x10, 0x100]))) for _ in range(50)]
    breads.append(("ACGTNNRYACGT" * (20 + k // 4), 0x10))
    bam = synth.bam_part([synth.bam_record(s, f, b"r%d" % i, n_cigar=i % 3) for i, (s, f) in enumerate(breads)])

    def bam_returns(both):
        seqs, n = synth.bam_reads_as_getseq(breads, both)
        return [S1._CODES[np.frombuffer(x, dtype=np.uint8)] for x in seqs], n

    cases.append(("bam", bam, capi.SPLIT_FILE_BAM, 1 << 17, False, bam_returns))
    return cases


# ---- the front end's planted input: two signatures the fixed map sends to one bin, each with a large share of the k-mers
def planted_input(k=27, m=5, n_bins=64, seed=5, n_background=113, n_planted=22):
    """-> (FASTA text, the two planted signatures). A read of the form  unit x N  whose every window has ONE signature s carries N - k + 1 k-mers of s; the
    pair (s1, s2) is chosen among allowed signatures that tools.count_signature_map sends to the same bin. CSignatureMapper::Init adds 1000 to every allowed
    signature's count, so a signature stands out of the mean bin only when the sample is large against 1000 x the allowed signatures / n_bins: m = 5 (about 600
    allowed signatures) keeps that at ten thousand k-mers."""
    from kmc_amd import tools

    rng = np.random.default_rng(seed)
    fixed = tools.count_signature_map(m, n_bins)
    norm = S1.norm_table(m)
    found = {}
    pair = None
    while pair is None:  # random periodic reads: keep those whose windows all share one signature
        unit = _rnd(rng, int(rng.integers(3, 7)))
        read = (unit * (4 * k))[:3 * k]
        _, ln, sg = S1.split_stream(S1._CODES[np.frombuffer(read, dtype=np.uint8)], k, m)
        if sg.size != 1 or int(sg[0]) == 4**m:
            continue
        s = int(sg[0])
        assert int(norm[s]) == s
        b = int(fixed[s])
        if b in found and found[b][0] != s:
            pair = (found[b], (s, unit))
        found.setdefault(b, (s, unit))
    (s1, u1), (s2, u2) = pair
    reads = [_rnd(rng, 150) for _ in range(n_background)]  # the background: 124 k-mers each at k = 27, over many signatures
    for u in (u1, u2):
        reads += [(u * 400)[:500] for _ in range(n_planted)]  # 474 k-mers each on one signature
    order = rng.permutation(len(reads))
    return _records_text("fa", b"\n", [reads[i] for i in order]), (s1, s2)


def balance_of(stats, sig_map, n_bins) -> float:
    """k-mers of the largest bin / of the mean bin, as tools.count reports it"""
    per_bin = np.zeros(n_bins, dtype=np.int64)
    np.add.at(per_bin, sig_map[stats > 0].astype(np.int64), stats[stats > 0].astype(np.int64))
    return int(per_bin.max()) * n_bins / max(int(stats.sum(dtype=np.uint64)), 1)
