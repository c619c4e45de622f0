"""TEST INFRASTRUCTURE shared by tests/test_count_emulated.py (CPU, the product's host library over the emulated HIP runtime), tests/test_gpu_count.py (-m gpu,
libkmc_hip.so) and tests/make_count_golden.py: the counting session (kmc_hip_count_*, `python -m kmc_amd.tools count`) against an independent oracle.

The oracle counts with numpy: the canonical k-mers of every read (the forward ones with -b, those of the homopolymer-compressed read with -hc), windows with an invalid
symbol and reads shorter than k skipped; k-mers are uint64 up to k = 32 and fixed-width byte rows above; np.unique with counts; then the writer's rule (drop below ci,
drop above cx, clamp to cs), setops_cases.encode_body and dbio.write_kmc1. It is held to what `kmc` followed by `kmc_tools transform sort` wrote (tests/golden/count_*,
made by tests/make_count_golden.py), byte for byte, so it is pinned to the reference and not to the code under test.

The builders are seeded; each asserts what its input contains. Nothing here reads a file outside tests/."""
import gzip
import os

import numpy as np

import setops_cases as S
from kmc_amd import capi, dbio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_CODES = np.full(256, -1, dtype=np.int8)  # splitter.cpp:42-47
for _c, _v in zip(b"ACGTacgt", [0, 1, 2, 3, 0, 1, 2, 3]):
    _CODES[_c] = _v


# ---- the oracle
def sequences(data: bytes, fmt: str) -> list:
    """the sequence of every record of a text: fmt 'fq' (4 lines), 'fa' (2 lines), 'fm' (a title, then lines up to the next title)"""
    lines = data.replace(b"\r\n", b"\n").split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    if fmt == "fq":
        return lines[1::4]
    if fmt == "fa":
        return lines[1::2]
    seqs = []
    for ln in lines:
        if ln.startswith(b">"):
            seqs.append(b"")
        else:
            seqs[-1] += ln
    return seqs


def _pack_rows(win: np.ndarray) -> np.ndarray:
    """[n, k] codes 0..3 -> [n, ceil(k / 4)] bytes, most significant first, the k-mer right-aligned"""
    n, k = win.shape
    nb = (k + 3) // 4
    padded = np.zeros((n, 4 * nb), dtype=np.uint8)
    padded[:, 4 * nb - k:] = win
    q = padded.reshape(n, nb, 4)
    return (q[:, :, 0] << 6) | (q[:, :, 1] << 4) | (q[:, :, 2] << 2) | q[:, :, 3]


def kmers_of_reads(reads, k: int, both: bool = True, hc: bool = False) -> np.ndarray:
    """every window of k valid symbols of every read as one k-mer: uint64[n] for k <= 32, uint8[n, ceil(k / 4)] above"""
    out = []
    for r in reads:
        c = _CODES[np.frombuffer(r, dtype=np.uint8)]
        if hc and c.size:  # HomopolymerCompressSeq (splitter.cpp:424-435): the first symbol and every symbol whose code differs from the one before it
            c = c[np.concatenate([[True], c[1:] != c[:-1]])]
        if c.size < k:
            continue
        win = np.lib.stride_tricks.sliding_window_view(c, k)
        win = win[(win >= 0).all(axis=1)].astype(np.uint8)
        if not win.shape[0]:
            continue
        rc = (3 - win[:, ::-1]).astype(np.uint8)
        if k <= 32:
            sh = (2 * np.arange(k - 1, -1, -1)).astype(np.uint64)
            f = (win.astype(np.uint64) << sh).sum(axis=1, dtype=np.uint64)
            out.append(np.minimum(f, (rc.astype(np.uint64) << sh).sum(axis=1, dtype=np.uint64)) if both else f)
        else:
            f, g = _pack_rows(win), _pack_rows(rc)
            if both:
                differ = f != g
                at = np.argmax(differ, axis=1)
                rows = np.arange(f.shape[0])
                take_rc = differ.any(axis=1) & (g[rows, at] < f[rows, at])
                f = np.where(take_rc[:, None], g, f)
            out.append(f)
    if not out:
        return np.zeros(0, dtype=np.uint64) if k <= 32 else np.zeros((0, (k + 3) // 4), dtype=np.uint8)
    return np.concatenate(out)


def count_oracle(reads, k, ci=2, cx=10**9, cs=255, both=True, hc=False) -> dict:
    """-> dict(kmers: ascending Python ints, counts: after the writer's rule, raw_counts: np array of every distinct k-mer's count, summary: the numbers `kmc` prints)"""
    all_k = kmers_of_reads(reads, k, both, hc)
    if k <= 32:
        u, n = np.unique(all_k, return_counts=True)
        as_int = [int(x) for x in u]
    else:
        u, n = np.unique(all_k, axis=0, return_counts=True)
        as_int = [int.from_bytes(row.tobytes(), "big") for row in u]
    keep = (n >= ci) & (n <= cx)
    kmers = [x for x, kp in zip(as_int, keep) if kp]
    counts = [min(int(c), cs) for c in n[keep]]
    summary = dict(n_below_min=int((n < ci).sum()), n_above_max=int((n > cx).sum()), n_unique=int(n.size), n_total=int(n.sum()))
    return dict(kmers=kmers, counts=counts, raw_counts=n, summary=summary)


def write_oracle_database(path, want, k, ci, cx, cs, both) -> None:
    p = S.best_p(k, len(want["kmers"]))
    csb = min(S.byte_log(cs), S.byte_log(cx))
    lut, recs = S.encode_body(k, p, csb, want["kmers"], want["counts"])
    dbio.write_kmc1(path, k, csb, p, ci, cx, both, lut, recs)


def database_bytes(path) -> tuple:
    with open(path + ".kmc_pre", "rb") as f, open(path + ".kmc_suf", "rb") as g:
        return f.read(), g.read()


# ---- the inputs of the goldens (seeded; about 6 KB of sequence each)
def _rnd(rng, n):
    return _ACGT[rng.integers(0, 4, size=n)].tobytes()


def golden_reads(seed: int, k: int, read_len: int = 100, n_reads: int = 60, clamp: bool = False) -> list:
    """60 reads of 100 symbols from a 1.5 kbp genome with 1 % substitutions; among them one read with N, one with lower case, one shorter than k, one of exactly k.
    clamp: a motif of k + 5 symbols in 45 of the reads and another in 10 of them (k-mers counted 45 and 10 times)"""
    rng = np.random.default_rng(seed)
    genome = _rnd(rng, 1500)
    reads = []
    for _ in range(n_reads):
        at = int(rng.integers(0, len(genome) - read_len))
        r = bytearray(genome[at:at + read_len])
        for e in np.flatnonzero(rng.random(read_len) < 0.01):
            r[e] = _ACGT[rng.integers(0, 4)]
        reads.append(bytes(r))
    if clamp:
        often, some = _rnd(rng, k + 5), _rnd(rng, k + 5)
        for i in range(45):
            reads[i] = reads[i][:20] + often + reads[i][20 + k + 5:]
        for i in range(45, 55):
            reads[i] = reads[i][:10] + some + reads[i][10 + k + 5:]
    reads[3] = reads[3][:40] + b"N" + reads[3][41:70] + b"NN" + reads[3][72:]
    reads[7] = reads[7][:50].lower() + reads[7][50:]
    reads[11] = reads[11][:k - 1]
    reads[13] = reads[13][:k]
    reads[17] = reads[17][:30] + b"A" * 9 + reads[17][39:]  # a run for -hc
    assert any(b"N" in r for r in reads) and any(len(r) < k for r in reads)
    return reads


def fastq_text(reads, eol=b"\n") -> bytes:
    return b"".join(b"@r%d" % i + eol + r + eol + b"+" + eol + b"I" * len(r) + eol for i, r in enumerate(reads))


def fasta_text(reads, eol=b"\n") -> bytes:
    return b"".join(b">r%d" % i + eol + r + eol for i, r in enumerate(reads))


def multiline_text(seqs, width=60) -> bytes:
    return b"".join(b">s%d some title\n" % i + b"".join(s[j:j + width] + b"\n" for j in range(0, len(s), width)) for i, s in enumerate(seqs))


def _k27_fm_seqs():
    rng = np.random.default_rng(105)
    genome = _rnd(rng, 1500)
    seqs = [genome[:700], genome[650:1500], genome[100:400] + b"NNNN" + genome[400:600].lower(), _rnd(rng, 20), genome[900:1300]]
    assert any(len(s) < 27 for s in seqs) and any(b"N" in s for s in seqs)
    return seqs


# name -> (flags of the `kmc` line, the oracle's (k, ci, cx, cs, both, hc), [(file name, format, bytes)])
def _cases():
    c = {}
    c["k27_fq"] = (["-k27"], (27, 2, 10**9, 255, True, False), [("count_k27_fq.fq", "fq", fastq_text(golden_reads(101, 27)))])
    c["k27_fa_b"] = (["-k27", "-ci1", "-b", "-fa"], (27, 1, 10**9, 255, False, False), [("count_k27_fa_b.fa", "fa", fasta_text(golden_reads(102, 27), b"\r\n"))])
    c["k28_fq"] = (["-k28", "-ci1"], (28, 1, 10**9, 255, True, False), [("count_k28_fq.fq", "fq", fastq_text(golden_reads(103, 28)))])
    c["k55_clamp"] = (["-k55", "-ci1", "-cs3", "-cx40"], (55, 1, 40, 3, True, False), [("count_k55_clamp.fq", "fq", fastq_text(golden_reads(104, 55, clamp=True)))])
    c["k27_fm"] = (["-k27", "-fm"], (27, 2, 10**9, 255, True, False), [("count_k27_fm.fa", "fm", multiline_text(_k27_fm_seqs()))])
    c["k27_hc"] = (["-k27", "-hc"], (27, 2, 10**9, 255, True, True), [("count_k27_hc.fq", "fq", fastq_text(golden_reads(106, 27)))])
    two = golden_reads(107, 27)
    c["k27_list"] = (["-k27", "-fa"], (27, 2, 10**9, 255, True, False), [("count_k27_list_1.fa", "fa", fasta_text(two[:35])), ("count_k27_list_2.fa", "fa", fasta_text(two[25:]))])
    c["k27_gz"] = (["-k27"], (27, 2, 10**9, 255, True, False), [("count_k27_gz.fq.gz", "fq", fastq_text(golden_reads(108, 27)))])
    return c


CASES = _cases()
CASE_IDS = list(CASES)


def case_reads(name) -> list:
    return [s for _, fmt, data in CASES[name][2] for s in sequences(data, fmt)]


def case_oracle(name) -> dict:
    k, ci, cx, cs, both, hc = CASES[name][1]
    want = count_oracle(case_reads(name), k, ci, cx, cs, both, hc)
    raw = want["raw_counts"]
    assert (raw < ci).any() or ci == 1, name  # a k-mer below the threshold
    if name == "k55_clamp":
        assert ((raw > cs) & (raw <= cx)).any() and (raw > cx).any(), name  # one clamped, one above the maximum
    return want


def golden_input_paths(name) -> list:
    return [os.path.join(GOLDEN, f) for f, _, _ in CASES[name][2]]


def golden_out(name) -> str:
    return os.path.join(GOLDEN, "count_" + name + "_out")


def input_argument(name, tmp_dir) -> str:
    """what goes in the place of <input> on the command line: the file, or @list of the case's files (written into tmp_dir)"""
    paths = golden_input_paths(name)
    if len(paths) == 1:
        return paths[0]
    lst = os.path.join(str(tmp_dir), "inputs.lst")
    with open(lst, "w") as f:
        f.write("\n".join(paths) + "\n")
    return "@" + lst


def committed_input(path) -> bytes:
    with open(path, "rb") as f:
        data = f.read()
    return gzip.decompress(data) if path.endswith(".gz") else data


# ---- the library under test
class CountContext(S.LibContext):
    """S.LibContext + the counting session, its test hook and the histogram entry: the interface of capi.Context on a library given by path"""

    def __init__(self, path):
        super().__init__(path)
        C, vp = self.C, self.C.c_void_p
        capi.bind_count(self.L)
        self.L.kmc_hip_db_histogram_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.c_uint32, C.c_uint32, C.c_uint64, vp, C.POINTER(C.c_uint64)]
        self.L.kmc_hip_split_covers.argtypes = [C.c_uint32]


for _name in ("debug_gather_segments", "db_histogram_device", "_need"):  # capi.Context's own (they use only self.L, self.h, self._chk): the binding the product ships
    setattr(CountContext, _name, getattr(capi.Context, _name))


def view_histogram(ctx, k, view, hi) -> np.ndarray:
    """the view's counters counted by kmc_hip_db_histogram_device into [1, hi]; -> uint64[hi + 1] indexed by count (entry 0 is 0)"""
    d_hist = ctx.malloc(8 * hi)
    try:
        st = ctx.db_histogram_device(k, view, 1, 1, hi, d_hist)
        h = np.zeros(hi, dtype=np.uint64)
        ctx.d2h(h, d_hist)
    finally:
        ctx.free(d_hist)
    assert st["n_cut_in"] == 0 and st["n_outside"] == 0 and st["n_counted"] == view.n_recs, st
    return np.concatenate([[0], h]).astype(np.uint64)


# ---- the gather kernel on planted tables
GATHER_LENGTHS = (0, 1, 15, 16, 17, 255, 256, 4097, 70000)


def gather_long_pairs(every_pair: bool) -> list:
    """the (source offset, destination offset) pairs mod 16 that get the 70 000-byte length — the only one at which a thread runs the 16-byte loop more than once: all
    256, or the 31 with one side at 0, which still hold every source offset, every destination offset and every shift (source - destination) mod 16"""
    if every_pair:
        return [(sa, da) for sa in range(16) for da in range(16)]
    return [(sa, 0) for sa in range(16)] + [(0, da) for da in range(1, 16)]


def gather_table(every_long_pair=False):
    """Segments for every source offset mod 16 x every destination offset mod 16: each of the lengths up to 4097 at all 256 pairs, 70 000 at gather_long_pairs(), a
    zero-length segment between the others. -> (table uint64[n, 3], source bytes, destination size). The source ends 16 bytes behind the last segment; segments keep
    their order in both buffers with gaps between them."""
    rng = np.random.default_rng(2024)
    segs = [(sa, da, ln) for ln in GATHER_LENGTHS[:-1] for sa in range(16) for da in range(16)]
    segs += [(sa, da, GATHER_LENGTHS[-1]) for sa, da in gather_long_pairs(every_long_pair)]
    order = rng.permutation(len(segs))
    table, s_at, d_at = [], 0, 0
    for i in order:
        sa, da, ln = segs[i]
        s_at = (s_at + 15) // 16 * 16 + sa
        d_at = (d_at + 15) // 16 * 16 + 16 + da  # at least one byte of gap in front of every destination segment
        table.append((s_at, d_at, ln))
        if len(table) % 7 == 0:
            table.append((s_at, d_at, 0))
        s_at += ln
        d_at += ln
    assert {(t[0] % 16, t[1] % 16) for t in table if t[2] == 17} == {(a, b) for a in range(16) for b in range(16)}
    longs = {(t[0] % 16, t[1] % 16) for t in table if t[2] == 70000}
    assert {(a - b) % 16 for a, b in longs} == {a for a, _ in longs} == {b for _, b in longs} == set(range(16))  # every shift of the register path, every offset
    if every_long_pair:
        assert longs == {(a, b) for a in range(16) for b in range(16)}
    src = rng.integers(0, 256, size=s_at + 16, dtype=np.uint8)
    return np.array(table, dtype=np.uint64), src, d_at + 64


def check_gather(ctx, table, src, dst_size):
    """the table through kmc_hip_debug_gather_segments: every segment arrived, every other byte of the destination is still 0xA5"""
    d_src, d_dst = ctx.malloc(src.size), ctx.malloc(dst_size)
    try:
        ctx.h2d(d_src, src)
        ctx.h2d(d_dst, np.full(dst_size, 0xA5, dtype=np.uint8))
        ctx.debug_gather_segments(d_src, d_dst, table)
        got = np.zeros(dst_size, dtype=np.uint8)
        ctx.d2h(got, d_dst)
    finally:
        ctx.free(d_src)
        ctx.free(d_dst)
    want = np.full(dst_size, 0xA5, dtype=np.uint8)
    for s, d, n in table.tolist():
        want[d:d + n] = src[s:s + n]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (int(bad[0]), int(bad.size))


# ---- a small input for the runs that are repeated (invariance, the session tests): two parts at part_bytes = 1024
def small_reads(k=27):
    rng = np.random.default_rng(77)
    genome = _rnd(rng, 300)
    reads = [genome[at:at + 70] for at in (0, 40, 80, 120, 160, 200, 230, 10, 50, 90, 130, 170)] + [genome[100:150] + b"N" + genome[151:200], genome[:k - 1], b"acgt" * 10]
    assert any(b"N" in r for r in reads) and any(len(r) < k for r in reads)
    return reads


def view_body(ctx, k, view) -> tuple:
    """-> (lut, recs) of a kmc_hip_db_view, copied down"""
    rb = (k - view.lut_prefix_len) // 4 + view.counter_size
    recs, lut = np.zeros(view.n_recs * rb, dtype=np.uint8), np.zeros(1 << (2 * view.lut_prefix_len), dtype=np.uint64)
    if view.n_recs:
        ctx.d2h(recs, view.d_recs)
    ctx.d2h(lut, view.d_lut)
    return lut, recs
