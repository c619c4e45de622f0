"""Reads against a k-mer database (`kmc_tools filter`): the semantics of CKMCFile::GetCountersForRead and of the three per-read rules of CFastqFilter restated on numpy
arrays and Python ints — no code shared with the kernels —, the command lines of the goldens under tests/golden/filter_*, the planted databases and reads, and the
helper that runs kmc_hip_db_query_reads_device. TEST INFRASTRUCTURE shared by tests/make_filter_golden.py, tests/test_db_query_emulated.py and tests/test_gpu_db_query.py."""
from __future__ import annotations

import gzip
import os

import numpy as np

import setops_cases as S

ROOT = S.ROOT
GOLDEN = S.GOLDEN
U32 = S.U32
STATS = ("n_valid_windows", "n_found", "n_cut", "n_invalid_windows")

CODE = np.full(256, 4, dtype=np.uint8)  # CKmerAPI::num_codes: ACGTacgt -> 0..3, everything else invalid
for _i, _c in enumerate("ACGT"):
    CODE[ord(_c)] = CODE[ord(_c.lower())] = _i


# ---- the semantics
def window_kmers(seq: np.ndarray, k: int, both_strands: bool):
    """-> (the k-mer of every window as a Python int — with both_strands the smaller of it and its reverse complement —, bool: the window has no invalid symbol)"""
    codes = CODE[np.asarray(seq, dtype=np.uint8)]
    n_win = codes.size - k + 1
    if n_win <= 0:
        return [], np.zeros(0, dtype=bool)
    words = (k + 31) // 32
    c = (codes & 3).astype(np.uint64)
    fw, rc = np.zeros((n_win, words), dtype=np.uint64), np.zeros((n_win, words), dtype=np.uint64)
    for j in range(k):  # symbol j of a window: the first one is the most significant of the k-mer and, complemented, the least significant of the reverse complement
        s = c[j:j + n_win]
        b = 2 * (k - 1 - j)
        fw[:, b // 64] |= s << np.uint64(b % 64)
        b = 2 * j
        rc[:, b // 64] |= (np.uint64(3) - s) << np.uint64(b % 64)
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    valid = (bad[k:] - bad[:-k]) == 0
    q = fw
    if both_strands:
        less, decided = np.zeros(n_win, dtype=bool), np.zeros(n_win, dtype=bool)
        for w in reversed(range(words)):
            less |= ~decided & (fw[:, w] < rc[:, w])
            decided |= fw[:, w] != rc[:, w]
        q = np.where(less[:, None], fw, rc)
    be = np.ascontiguousarray(q[:, ::-1]).astype(">u8")
    return [int.from_bytes(be[i].tobytes(), "big") for i in range(n_win)], valid


def restate_counters(seq, k, both_strands, db, ci, cx):
    """db: (kmers, counts) as the body holds them. -> (uint32[len(seq)]: the counter of the window that starts at every byte, 0 where there is none; tallies)"""
    seq = np.asarray(seq, dtype=np.uint8)
    counts = dict(zip(*db))
    out = np.zeros(seq.size, dtype=np.uint32)
    st = dict.fromkeys(STATS, 0)
    kmers, valid = window_kmers(seq, k, both_strands)
    for i, x in enumerate(kmers):
        if not valid[i]:
            st["n_invalid_windows"] += 1
            continue
        st["n_valid_windows"] += 1
        c = counts.get(x)
        if c is None:
            continue
        if ci <= c <= cx:
            out[i] = c
            st["n_found"] += 1
        else:
            st["n_cut"] += 1
    return out, st


def restate_reads(seq, counters, read_off, k, threshold):
    """The three rules per read: -> (n_valid uint32[n_reads], trim_len uint32[n_reads], masked uint8[len(seq)])"""
    seq = np.asarray(seq, dtype=np.uint8)
    n_reads = len(read_off) - 1
    n_valid, trim = np.zeros(n_reads, dtype=np.uint32), np.zeros(n_reads, dtype=np.uint32)
    masked = seq.copy()
    for r in range(n_reads):
        a, length = int(read_off[r]), int(read_off[r + 1]) - 1 - int(read_off[r])
        n_win = length - k + 1
        if n_win <= 0:
            continue
        c = counters[a:a + n_win]
        n_valid[r] = np.count_nonzero(c)
        low = c < threshold
        if not low[0]:
            later = np.flatnonzero(low[1:])
            trim[r] = k - 1 + (int(later[0]) + 1 if later.size else n_win)
        covered = np.convolve(low.astype(np.int64), np.ones(k, dtype=np.int64)) > 0  # base b: a low window among b - k + 1 .. b
        masked[a:a + length][covered] = ord("N")
    return n_valid, trim, masked


def restate(case):
    counters, st = restate_counters(case["seq"], case["k"], case["both"], case["db"], *case["cut"])
    return (counters, *restate_reads(case["seq"], counters, case["read_off"], case["k"], case["threshold"]), st)


def layout(reads):
    """reads: list of bytes -> (uint8 array: every read followed by '\\n', uint64 offsets[n + 1])"""
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) + 1 for r in reads])
    return np.frombuffer(b"".join(r + b"\n" for r in reads), dtype=np.uint8).copy(), off


# ---- the device call
class LibContext(S.LibContext):
    """setops_cases.LibContext + kmc_hip_db_query_reads_device"""

    def __init__(self, path):
        super().__init__(path)
        C, vp = self.C, self.C.c_void_p
        self.L.kmc_hip_db_query_reads_device.argtypes = [vp, C.c_int, C.POINTER(self.capi.DbView), C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp,
                                                         C.POINTER(C.c_uint64)]

    def db_query_reads_device(self, db, kmer_len, both_strands, d_seq, n_bytes, d_read_off, n_reads, threshold, d_counters, d_n_valid=0, d_trim_len=0, d_masked=0):
        st = (self.C.c_uint64 * 4)()
        self._chk(self.L.kmc_hip_db_query_reads_device(self.h, 0, self.C.byref(db), kmer_len, 1 if both_strands else 0, d_seq or None, n_bytes, d_read_off or None, n_reads, threshold,
                                                       d_counters or None, d_n_valid or None, d_trim_len or None, d_masked or None, st))
        return dict(zip(STATS, (int(x) for x in st)))


class Runner:
    """Device buffers kept across the calls of a test (grow-only), one database body at a time."""

    def __init__(self, ctx):
        self.ctx, self.bufs, self.db_allocs, self.view = ctx, {}, [], None

    def _buf(self, name, nbytes):
        d, cap = self.bufs.get(name, (0, 0))
        if nbytes > cap:
            if d:
                self.ctx.free(d)
            d, cap = self.ctx.malloc(2 * nbytes + 256), 2 * nbytes + 256
            self.bufs[name] = (d, cap)
        return d

    def set_db(self, k, p, cb, db, cut):
        from kmc_amd import capi

        for d in self.db_allocs:
            self.ctx.free(d)
        lut, recs = S.encode_body(k, p, cb, *db)
        self.db_allocs = [self.ctx.malloc(recs.nbytes + 256), self.ctx.malloc(lut.nbytes + 256)]
        if recs.nbytes:
            self.ctx.h2d(self.db_allocs[0], recs)
        self.ctx.h2d(self.db_allocs[1], lut)
        self.view = capi.DbView(self.db_allocs[0], len(db[0]), self.db_allocs[1], p, cb, cut[0], cut[1])

    def run(self, k, both, seq, read_off, threshold, want=("counters", "n_valid", "trim_len", "masked")):
        """-> (counters, n_valid, trim_len, masked, tallies); outputs not in `want` are not asked for (NULL) and come back as None"""
        seq, read_off = np.ascontiguousarray(seq, dtype=np.uint8), np.ascontiguousarray(read_off, dtype=np.uint64)
        n, n_reads = seq.size, read_off.size - 1
        d_seq, d_off, d_cnt = self._buf("seq", n), self._buf("off", read_off.nbytes), self._buf("cnt", 4 * n)
        d_nv = self._buf("nv", 4 * n_reads) if "n_valid" in want else 0
        d_tl = self._buf("tl", 4 * n_reads) if "trim_len" in want else 0
        d_mk = self._buf("mk", n) if "masked" in want else 0
        if n:
            self.ctx.h2d(d_seq, seq)
        self.ctx.h2d(d_off, read_off)
        st = self.ctx.db_query_reads_device(self.view, k, both, d_seq, n, d_off, n_reads, threshold, d_cnt, d_nv, d_tl, d_mk)

        def back(d, dtype, m):
            a = np.zeros(m, dtype=dtype)
            if d and m:
                self.ctx.d2h(a, d)
            return a if d else None

        return back(d_cnt, np.uint32, n), back(d_nv, np.uint32, n_reads), back(d_tl, np.uint32, n_reads), back(d_mk, np.uint8, n), st

    def close(self):
        for d, _ in self.bufs.values():
            self.ctx.free(d)
        for d in self.db_allocs:
            self.ctx.free(d)
        self.bufs, self.db_allocs = {}, []


def check_case(runner, case):
    """The device call must equal the restatement: every counter, the per-read results, the masked bytes and the four tallies. -> the tallies"""
    k = case["k"]
    runner.set_db(k, case["p"], case["cb"], case["db"], case["cut"])
    got = runner.run(k, case["both"], case["seq"], case["read_off"], case["threshold"])
    want = restate(case)
    for name, g, w in zip(("counters", "n_valid", "trim_len", "masked"), got, want):
        if not np.array_equal(g, w):
            at = np.flatnonzero(g != w)
            raise AssertionError(f"{case['name']}: {name} differ at {at[:8]} ({at.size} places): got {g[at[:8]]}, want {w[at[:8]]}")
    assert got[4] == want[4], (case["name"], got[4], want[4])
    return got[4]


# ---- planted databases and reads
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


def product_tile(k):
    """window starts of a k_dbq_lookup tile: DQ_THREADS x dq_default_ipt (kmc_amd/csrc/order_db.hip.h)"""
    return 256 * (4 if (k + 31) // 32 <= 2 else 8)


def kmer_int(s: bytes) -> int:
    x = 0
    for ch in s:
        x = (x << 2) | int(CODE[ch])
    return x


def kmer_text(x: int, k: int) -> bytes:
    return bytes(b"ACGT"[(x >> (2 * (k - 1 - j))) & 3] for j in range(k))


def db_of(text: np.ndarray, k, both, rng, lo=2, hi=200):
    """every window of `text` as a database: dict k-mer -> count in [lo, hi)"""
    kmers, valid = window_kmers(text, k, both)
    assert valid.all()
    uniq = sorted(set(kmers))
    return dict(zip(uniq, (int(c) for c in rng.integers(lo, hi, size=len(uniq)))))


def _sorted_db(d):
    ks = sorted(d)
    return ks, [d[x] for x in ks]


# (k, lut_prefix_len): what the GPU test runs; at k = 33 and 65 one prefix length lies across a 64-bit word of the k-mer (33: 2 (k - p) = 56 + 10 bits; 65: 120 + 10) and one does not
PLANTED = [(27, 3), (32, 4), (33, 5), (33, 1), (64, 4), (65, 5), (65, 1), (127, 3), (129, 5), (224, 4)]
PLANTED_IDS = [f"{k}-p{p}" for k, p in PLANTED]
assert S.straddles(33, 5) and not S.straddles(33, 1) and S.straddles(65, 5) and not S.straddles(65, 1)
for _k, _p in PLANTED:
    assert (_k - _p) % 4 == 0


def planted_cases(k, p, tile, seed=3):
    """-> list of cases: dict(name, k, p, cb, db (kmers, counts), cut, both, seq, read_off, threshold). `tile`: window starts of a lookup tile of the library under test.
    The main layout is a little more than four tiles: read 0 ends on the first seam (its terminator is the last byte of tile 0), read 1 is longer than three tiles, then
    reads of 0, k - 1 and k symbols and the reads for the trimming rule."""
    assert tile - 1 >= 3 * k + 8, "read 0 is to end on the first seam and hold its masked runs"
    rng = np.random.default_rng(seed + 1000 * k + p)
    g = BASES[rng.integers(0, 4, size=4 * tile + tile // 4 + 4 * k)]  # the genome: every read is cut from it, so by default every window is found
    gb = g.tobytes()
    cases = []

    def reads_main():
        r0 = bytearray(gb[:tile - 1])
        long_len = 3 * tile + 7
        r1 = bytearray(gb[tile:tile + long_len])
        seam2, seam3 = tile - 0, 2 * tile  # positions inside read 1 (it starts on a seam) of the next two seams
        for at in (seam2 - 1, seam2 + k // 2, seam3 + 3):  # substituted bases: the k windows over each are (almost surely) absent
            r1[at] = b"ACGT"[(b"ACGT".index(r1[at]) + 1 + at % 3) % 4]
        r1[seam3 - k // 3] = ord("N")
        r1[5 * k:5 * k + 2 * k] = bytes(r1[5 * k:7 * k]).lower()  # lower case is valid
        r1[long_len - 2] = ord("n")
        tail = 4 * tile + 8
        return [bytes(r0), bytes(r1), b"", gb[5:5 + k - 1], gb[9:9 + k], gb[tail:tail + 2 * k + 5], gb[tail + k:tail + 2 * k + 9], revcomp(gb[tail + 3:tail + 3 + k + 6]), b"", gb[-k:]]

    def low_windows(reads):
        """windows given the count 1 (low under threshold 2): in read 0 the first (the run reaches the read's start), two k apart (their runs touch), one two further (overlap)
        and the last (reaches the end); window 7 of the first trimming read"""
        n_win0 = len(reads[0]) - k + 1
        idx0 = [0, k + 2, 2 * k + 2, 2 * k + 4, n_win0 - 1]
        return [reads[0][i:i + k] for i in idx0] + [reads[5][7:7 + k]]

    def canon(s, both):
        x = kmer_int(s)
        return min(x, kmer_int(revcomp(s))) if both else x

    reads = reads_main()
    seq, off = layout(reads)
    for name, cb, both, thr, cut, hi in (("main_cb1_thr2", 1, True, 2, (1, 255), 200), ("main_cb2_thr1_cut", 2, True, 1, (30, 150), 200),
                                         ("main_cb3_forward_thr2", 3, False, 2, (1, U32), 1 << 24), ("main_cb4_thr2", 4, True, 2, (1, U32), 1 << 32)):
        d = db_of(g, k, both, rng, 2, hi)
        for s in low_windows(reads):
            d[canon(s, both)] = 1
        cases.append(dict(name=name, k=k, p=p, cb=cb, db=_sorted_db(d), cut=cut, both=both, seq=seq, read_off=off, threshold=thr))
    # the database's bounds, forward k-mers so that the keys are what is written here: prefix x1 holds m records, the last prefix holds the last records, x0 is empty
    n_pref, sbits = 1 << (2 * p), 2 * (k - p)
    x1, x0, xl = n_pref // 3, n_pref // 3 + 1, n_pref - 1
    sufs = sorted({int.from_bytes(rng.bytes((sbits + 7) // 8), "big") % ((1 << sbits) - 4) + 2 for _ in range(7)})
    last_sufs = sorted({int.from_bytes(rng.bytes((sbits + 7) // 8), "big") % ((1 << sbits) - 4) + 2 for _ in range(3)})
    d = {(x1 << sbits) | s: 10 + i for i, s in enumerate(sufs)}
    d.update({(xl << sbits) | s: 40 + i for i, s in enumerate(last_sufs)})
    d[5] = 77  # the first record of the first prefix
    queries = [(x1 << sbits) | sufs[0], (x1 << sbits) | sufs[-1], (x1 << sbits) | (sufs[0] - 1), (x1 << sbits) | (sufs[-1] + 1), (x1 << sbits) | (sufs[3] + 1), (x0 << sbits) | sufs[2],
               (xl << sbits) | last_sufs[-1], (xl << sbits) | last_sufs[0], (xl << sbits) | (last_sufs[-1] + 1), (xl << sbits) | (last_sufs[0] - 1), 5, 4, 6, (1 << (2 * k)) - 1, 0]
    assert all((q in d) == want for q, want in zip(queries, (1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 0, 0)))
    bseq, boff = layout([kmer_text(q, k) for q in queries])
    cases.append(dict(name="bounds", k=k, p=p, cb=1, db=_sorted_db(d), cut=(1, 255), both=False, seq=bseq, read_off=boff, threshold=1))
    # both_strands 0 and a query whose reverse complement alone is in the database: 0
    only_rc = [kmer_text(q, k) for q in queries[:2]]
    rseq, roff = layout([revcomp(s) for s in only_rc] + only_rc)
    assert all(kmer_int(revcomp(s)) not in d for s in only_rc)
    cases.append(dict(name="reverse_complement_alone_forward_db", k=k, p=p, cb=1, db=_sorted_db(d), cut=(1, 255), both=False, seq=rseq, read_off=roff, threshold=1))
    # ... and with both_strands 1 on a canonical database both are found
    dc = {min(kmer_int(s), kmer_int(revcomp(s))): 9 + i for i, s in enumerate(only_rc)}
    cases.append(dict(name="reverse_complement_canonical_db", k=k, p=p, cb=1, db=_sorted_db(dc), cut=(1, 255), both=True, seq=rseq, read_off=roff, threshold=1))
    if k % 2 == 0:  # a k-mer that is its own reverse complement
        half = gb[17:17 + k // 2]
        pal = half + revcomp(half)
        assert revcomp(pal) == pal
        dp = dict(dc)
        dp[kmer_int(pal)] = 123
        pseq, poff = layout([pal, gb[40:60] + pal + gb[70:90]])
        cases.append(dict(name="own_reverse_complement", k=k, p=p, cb=1, db=_sorted_db(dp), cut=(1, 255), both=True, seq=pseq, read_off=poff, threshold=1))
    cases.append(dict(name="empty_database", k=k, p=p, cb=2, db=([], []), cut=(1, 255), both=True, seq=seq, read_off=off, threshold=1))
    return cases


def shifted_invalid(k, p, tile, seed=4):
    """One read across the first seam with one 'N' k symbols in front of the seam, and the database of every window of the read without the 'N'. Shifted by d = 0 .. 2 k
    bytes (a read of d - 1 'N' in front) the invalid symbol lies at every offset within k of the seam. -> (case without the shift, function d -> (seq, read_off))"""
    rng = np.random.default_rng(seed + 1000 * k + p)
    g = BASES[rng.integers(0, 4, size=tile + 3 * k + 9)]
    d = db_of(g, k, True, rng)
    r = bytearray(g.tobytes())
    r[tile - k] = ord("N")
    base_seq, base_off = layout([bytes(r)])

    def shifted(dist):
        if dist == 0:
            return base_seq, base_off
        return layout([b"N" * (dist - 1), bytes(r)])

    return dict(name="shifted_invalid", k=k, p=p, cb=1, db=_sorted_db(d), cut=(1, 255), both=True, seq=base_seq, read_off=base_off, threshold=1), shifted


# ---- the goldens: command lines of `kmc_tools filter` (tests/make_filter_golden.py) — (name, k, database, [mode], database options, reads, reads options, output options)
# the fixtures are kept gzipped (the front end reads them as they are); *_k: no read shorter than k = 33 (for -t and fractions)
FQ, FA, FQ_LONG, FA_LONG = "filter_reads.fq.gz", "filter_reads.fa.gz", "filter_reads_k.fq.gz", "filter_reads_k.fa.gz"
LINES = []
for _mode, _mname in (([], "normal"), (["-t"], "trim"), (["-hm"], "mask")):
    _fq, _fa = (FQ, FA) if _mode != ["-t"] else (FQ_LONG, FA_LONG)
    LINES += [(f"k27_{_mname}_fq_fq", 27, "a", _mode, [], _fq, ["-ci3"], []), (f"k27_{_mname}_fq_fa", 27, "a", _mode, [], _fq, ["-ci3"], ["-fa"]),
              (f"k27_{_mname}_fa_fa", 27, "a", _mode, [], _fa, ["-ci3", "-fa"], [])]
LINES += [
    ("k27_normal_defaults", 27, "a", [], [], FQ, [], []),
    ("k27_normal_ci20_cx120", 27, "a", [], [], FQ, ["-ci20", "-cx120"], []),
    ("k27_normal_fraction", 27, "a", [], [], FQ_LONG, ["-ci0.3", "-cx0.9"], []),
    ("k27_normal_fraction_fa", 27, "a", [], [], FA_LONG, ["-ci0.5", "-cx1.0", "-fa"], []),
    ("k27_normal_db_ci3_cx6", 27, "a", [], ["-ci3", "-cx6"], FQ, ["-ci10"], []),
    ("k27_mask_db_ci4", 27, "a", ["-hm"], ["-ci4"], FQ, ["-ci1"], ["-fa"]),
    ("k27_trim_ci1", 27, "a", ["-t"], [], FQ_LONG, ["-ci1"], []),
    ("k33_normal", 33, "a", [], [], FQ, ["-ci5"], []),
    ("k33_mask", 33, "a", ["-hm"], [], FQ, ["-ci2"], []),
    ("k33_normal_raw", 33, "raw_a", [], [], FQ, ["-ci5"], []),
    ("k33_mask_raw", 33, "raw_a", ["-hm"], [], FQ, ["-ci2"], []),
]
LINE_IDS = [ln[0] for ln in LINES]


def golden_out(name) -> bytes:
    """what `kmc_tools -t1 filter` wrote for the line of that name"""
    return gzip.open(os.path.join(GOLDEN, "filter_out_" + name + ".gz"), "rb").read()


def command_line(line, out, plain_dir=None):
    """plain_dir: where the reads fixtures lie unpacked (kmc_tools takes a name that ends in .gz for a packed file), without their '.gz'"""
    name, k, db, mode, db_opts, reads, reads_opts, out_opts = line
    reads = os.path.join(plain_dir, reads[:-3]) if plain_dir else os.path.join(GOLDEN, reads)
    return ["filter", *mode, S.golden_path(k, db), *db_opts, reads, *reads_opts, out, *out_opts]


def database_kmers(path):
    """(header, (kmers, counts)) of a golden database, KMC1 or as `kmc` wrote it (KMC2: one body per signature bin)"""
    from kmc_amd import dbio

    d = dbio.read_database(path)
    if not d.kmc2:
        return d, S.decode_body(d.kmer_len, d.lut_prefix_len, d.counter_size, d.lut, d.recs)
    both = {}
    for recs, per_prefix in d.bins:
        lut = np.concatenate([[0], np.cumsum(per_prefix)[:-1]])
        both.update(zip(*S.decode_body(d.kmer_len, d.lut_prefix_len, d.counter_size, lut, recs)))
    ks = sorted(both)
    return d, (ks, [both[x] for x in ks])


def restate_filter(line) -> bytes:
    """What `kmc_tools filter` writes for a golden command line, from restate_counters / restate_reads and the helpers' rules (fastq_filter.cpp:379-650) record by record:
    normal copies the record (FASTQ: without the text behind '+'; to FASTA: the first two lines, '>' for '@'), -t and -hm write header, sequence[, '+', quality] with '\\n'."""
    name, k, dbname, mode, db_opts, reads, reads_opts, out_opts = line
    hdr, db = database_kmers(S.golden_path(k, dbname))
    ci, cx = S._opt(db_opts, "-ci") or hdr.min_count, S._opt(db_opts, "-cx") or hdr.max_count
    fa_in = "-fa" in reads_opts
    fa_out = fa_in or "-fa" in out_opts
    bounds = {o[:3]: o[3:] for o in reads_opts if o[:3] in ("-ci", "-cx")}
    use_float = any("." in v for v in bounds.values())
    lines = gzip.open(os.path.join(GOLDEN, reads), "rb").read().split(b"\n")[:-1]  # every line still with its '\r', if it has one
    per = 2 if fa_in else 4
    recs = [lines[i:i + per] for i in range(0, len(lines), per)]
    strip = lambda s: s[:-1] if s.endswith(b"\r") else s  # noqa: E731
    seq, off = layout([strip(r[1]) for r in recs])
    threshold = int(bounds.get("-ci", "2")) if not use_float else 0
    counters, _ = restate_counters(seq, k, hdr.both_strands, db, ci, cx)
    n_valid, trim, masked = restate_reads(seq, counters, off, k, threshold)
    out = bytearray()
    for r, rec in enumerate(recs):
        length = len(strip(rec[1]))
        head = (b">" + strip(rec[0])[1:]) if fa_out else strip(rec[0])
        if mode == []:
            if use_float:
                if length < k:
                    continue
                n_win = np.float32(length - k + 1)
                lo, hi = np.uint32(np.float32(bounds.get("-ci", "0.0")) * n_win), np.uint32(np.float32(bounds.get("-cx", "1.0")) * n_win)
            else:
                lo, hi = int(bounds.get("-ci", "2")), int(bounds.get("-cx", "1000000000"))
            if not lo <= n_valid[r] <= hi:
                continue
            if fa_in:
                out += rec[0] + b"\n" + rec[1] + b"\n"
            elif fa_out:
                out += b">" + rec[0][1:] + b"\n" + rec[1] + b"\n"
            else:
                out += rec[0] + b"\n" + rec[1] + b"\n+" + (b"\r" if rec[2].endswith(b"\r") else b"") + b"\n" + rec[3] + b"\n"
            continue
        if mode == ["-t"]:
            if trim[r] == 0:
                continue
            body, qual = strip(rec[1])[:trim[r]], None if fa_in else strip(rec[3])[:trim[r]]
        else:
            body, qual = masked[int(off[r]):int(off[r]) + length].tobytes(), None if fa_in else strip(rec[3])
        out += head + b"\n" + body + b"\n"
        if not fa_out:
            out += b"+\n" + qual + b"\n"
    return bytes(out)
