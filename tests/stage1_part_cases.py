"""TEST INFRASTRUCTURE shared by tests/test_stage1_parts_emulated.py (CPU, the product's host library over the emulated HIP runtime) and
tests/test_gpu_stage1_parts.py (-m gpu, libkmc_hip.so): plain FASTA / FASTQ parts — kmc_hip_split_part with file_type 0 or 1 and no flags, what
kmc_hip_s1 calls for nearly every part — against the reference's GetSeq + ProcessReads restatement (tests/oracle_s1.py), over k, the signature
length, the piece marks of over-long lines, the second cut attempt and the sorted emit.

check_plain compares one part; the builders below make the parts, seeded and deterministic, and assert what each part is built to contain. Both
files use the same builders; only the sizes differ (`codes`: the length of the code stream the part must exceed, `supers`: the number of
super-k-mers). Nothing here reads a file outside tests/."""
import numpy as np

import oracle_s1 as S1
from test_stage1_emulated import _parse_bin, _records_text, _sig_map
from test_stage1_hc_emulated import getseq_returns, oracle_of_returns

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

# constants of the code under test that the cases are sized to (kmc_amd/csrc/stage1_kernels.hip.h, stage1_chain.h)
S1_SIG_PER = 5           # windows narrower than this take the branch `w < S1_SIG_PER` of s1_signatures_to_lds
S1_TILE = 1024           # super-k-mers per workgroup of k_s1_emit_sorted
S1_WG_TILE = 4 * S1_TILE  # positions per workgroup of k_s1_cut (the small emulated geometry: 2 * S1_TILE)
S1_SK_TILE = 1024        # super-k-mers per workgroup of k_s1_bin_totals / k_s1_bin_plus_x / k_s1_emit (the small emulated geometry: 64)
S1_MAX_BINS = 2048
SK_GUESS_DIV, SK_GUESS_ADD = 8, 4096  # S1PartParams::sk_guess_div and the constant of s1_split_part: the first cut attempt has room for codes / 8 + 4096 super-k-mers


def check_plain(lib, text, file_type, k, line_cap, long_read=False, m=9, n_bins=37, max_x=3, both=True, exact=False):
    """one plain part through lib (an HcLib) against the oracle: n_reads, per bin the records and the three sums. exact: every bin byte for byte the
    oracle's records in read order (what the sorted emit promises), otherwise as a sorted multiset. Returns the oracle's dict."""
    smap = _sig_map(m, n_bins, 5)
    rc, got = lib.split(text, k, m, n_bins, smap, line_cap, file_type, 1 if long_read else 0, max_x, both, flags=0)
    assert rc == 0, got
    returns, n_reads = getseq_returns(text, file_type, k, line_cap, long_read)
    want = oracle_of_returns(returns, n_reads, k, m, n_bins, smap, max_x, both)
    assert got["n_reads"] == want["n_reads"]
    for b in range(n_bins):
        if exact:
            assert got["bins"][b].tobytes() == b"".join(want["bins"][b]), b
        else:
            assert _parse_bin(got["bins"][b], k) == sorted(want["bins"][b]), b
    for key in ("kmers", "supers", "plus_x"):
        assert np.array_equal(got[key], want[key]), key
    return want


def rnd(rng, n):
    return _ACGT[rng.integers(0, 4, size=n)].tobytes()


def n_codes(reads):
    """length of the code stream of these sequence lines: every line is followed by one separator"""
    return sum(len(r) + 1 for r in reads)


def n_supers(reads, k, m):
    return int(S1.split(reads, k, m)[0].size)


# ---- (a) the (k, m) grid
GRID = [(5, 5), (13, 10), (14, 11), (9, 9), (15, 11), (16, 11),  # window widths w = k - m + 1 around S1_SIG_PER: 1, 4, 4, 1, 5, 6
        (27, 5), (27, 6), (27, 7), (27, 8), (27, 10), (27, 11),  # every signature length the C-ABI takes (9 is everywhere else)
        (32, 11), (33, 7), (64, 8), (65, 6), (128, 10), (129, 9), (255, 8), (256, 5), (256, 11)]  # record widths; (256, 5): w = 252, the end of S1SigLds::mm
_FORMATS = [("fq", b"\n"), ("fa", b"\r\n"), ("fa", b"\n"), ("fq", b"\r\n")]


def grid_cases():
    """-> list of dict(k, m, fmt, eol, max_x, both), one per GRID entry: format x end of line and (max_x, strands) rotate over the grid. The two w = 1
    parts are FASTQ: there a record is 3 or 4 bytes per symbol, and HcLib's record buffer is twice the text."""
    cases = []
    for i, (k, m) in enumerate(GRID):
        fmt, eol = _FORMATS[i % 4]
        cases.append(dict(k=k, m=m, fmt=fmt, eol=eol, max_x=(i + i // 8) % 4, both=(i // 4) % 2 == 0))
    assert {(c["max_x"], c["both"]) for c in cases} == {(x, b) for x in range(4) for b in (True, False)}
    assert {(c["fmt"], c["eol"]) for c in cases} == set(_FORMATS)
    assert all(c["fmt"] == "fq" for c in cases if c["k"] == c["m"])
    assert len({(c["k"], c["m"]) for c in cases}) == len(GRID) == 21
    return cases


def grid_ids():
    return ["k%d-m%d" % km for km in GRID]


def grid_reads(k, m, codes, supers=0, seed=0):
    """the reads of one grid part, as _reads of tests/test_stage1_emulated.py: the fixed ones, then random reads of k .. k + 120 symbols until the code
    stream is longer than `codes` and holds more than `supers` super-k-mers"""
    rng = np.random.default_rng(1000 * k + m + seed)
    per = rnd(rng, 11)
    reads = [rnd(rng, 150) + b"N" + rnd(rng, 80) + b"NN" + rnd(rng, k - 1) + b"N" + rnd(rng, k) + b"n" + rnd(rng, 200),  # stretches of k - 1 and of k valid symbols
             (per * (k // 11 + 40))[:k + 400],  # 11-periodic
             rnd(rng, k), rnd(rng, k - 1), rnd(rng, k + 1),
             b"A" * (k + 300),  # 301 k-mers of one signature: the 256-k-mer cap, a record of k + 255 symbols
             (b"AC" * (k + 60))[:k + 100], (b"ACGT" * (k + 60))[:k + 101], (b"AT" * (k + 60))[:k + 100],  # repeats: the k-mer's first symbols equal its reverse complement's
             b"N" * 40]
    fixed = len(reads)
    while n_codes(reads) <= codes or len(reads) < fixed + 8:
        reads.append(rnd(rng, int(rng.integers(k, k + 121))))
    while supers and n_supers(reads, k, m) <= supers:
        reads += [rnd(rng, int(rng.integers(k, k + 121))) for _ in range(16)]
    order = rng.permutation(len(reads))  # the fixed reads among the others, not in front of them
    return [reads[i] for i in order]


def grid_text(case, codes, supers=0):
    """-> (text, file_type) of the case's part"""
    reads = grid_reads(case["k"], case["m"], codes, supers)
    assert n_codes(reads) > codes
    return _records_text(case["fmt"], case["eol"], reads), 1 if case["fmt"] == "fq" else 0


def check_grid_case(lib, case, codes, supers=0, n_bins=37, exact=False):
    """the case's part through lib; then what the part was built for, from the oracle's result"""
    k, m = case["k"], case["m"]
    text, ft = grid_text(case, codes, supers)
    want = check_plain(lib, text, ft, k, 1 << 17, m=m, n_bins=n_bins, max_x=case["max_x"], both=case["both"], exact=exact)
    assert int(want["supers"].sum()) > supers
    assert any(r[0] == 255 for recs in want["bins"] for r in recs)  # a record of k + 255 symbols
    assert (int(want["plus_x"].sum()) > 0) == (case["max_x"] > 0)
    assert want["pieces"] == want["n_reads"]  # no line was cut: the marks are case (b)'s
    return want


# ---- (b) lines beyond the line cap, long-read parts
PIECE_KM = [(27, 9, True), (27, 9, False), (14, 11, True), (256, 11, True)]


def piece_line_cap(k):
    return k + 4105  # the library refuses anything below k + S1_WG_TILE + 2; the stride is then just beyond one workgroup window of k_s1_cut


def piece_lines(k, seed=0):
    """-> (lines, line_cap): as test_lines_beyond_the_line_cap_are_cut_where_the_reference_cuts_them — lines of exactly the cap, a symbol short of it and a
    symbol beyond it, of 2 stride + 5 symbols and of 5 pieces (N exactly at a piece start, n three symbols before another), poly-A beyond the cap, short reads between them"""
    rng = np.random.default_rng(7000 + k + seed)
    line_cap = piece_line_cap(k)
    stride = line_cap - k + 1
    long5 = bytearray(rnd(rng, 4 * stride + 900))
    long5[stride] = ord("N")  # an invalid symbol exactly where a piece starts: no mark is needed there, none may be invented
    long5[2 * stride - 3] = ord("n")
    short = lambda: rnd(rng, int(rng.integers(k, k + 200)))
    lines = [short(), rnd(rng, line_cap), short(), rnd(rng, line_cap - 1), rnd(rng, 60), rnd(rng, line_cap + 1), short(), rnd(rng, 2 * stride + 5), bytes(long5), short(),
             b"A" * (line_cap + 300), short()]
    return lines, line_cap


def pieces_of(lines, k, line_cap):
    """how many buffers GetSeq hands out for these lines: while line_cap symbols or more are left it hands out line_cap of them and goes on k - 1 symbols before
    their end; what is left then, if anything, is the last piece"""
    stride, n = line_cap - k + 1, 0
    for ln in lines:
        left = len(ln)
        while left >= line_cap:
            left -= stride
            n += 1
        n += 1
    return n


def uncut_supers(text, file_type, k, m, both=True):
    """the super-k-mers of the part if no line were cut (a line cap beyond every line)"""
    returns, _ = getseq_returns(text, file_type, k, 1 << 17)
    assert all(q.size < (1 << 17) for q in returns)
    return sum(int(S1.split_stream(q, k, m)[0].size) for q in returns if q.size >= k)


def check_piece_part(lib, k, m, both, fmt, eol, exact=False, cut_last=False):
    """the piece lines as one part (cut_last: a FASTA part that ends inside a long last line): parity, the oracle's piece count, and more super-k-mers than
    the same text gives uncut — so that a cut which ignored the marks cannot pass"""
    lines, line_cap = piece_lines(k)
    stride = line_cap - k + 1
    ft = 1 if fmt == "fq" else 0
    if cut_last:
        lines = lines[:4] + [rnd(np.random.default_rng(k), 3 * stride + k + 50)]  # four pieces, the last of k + 50 symbols
    text = _records_text(fmt, eol, lines)
    if cut_last:
        assert fmt == "fa"
        text = text[: len(text) - len(eol)]
    want = check_plain(lib, text, ft, k, line_cap, m=m, both=both, exact=exact)
    # extra pieces: 1 each for the lines of the cap, one beyond it, 2 stride + 5 and poly-A, 4 for the five-piece line; cut_last: 1 + 3
    assert want["pieces"] == pieces_of(lines, k, line_cap) == len(lines) + (4 if cut_last else 8)
    assert want["n_reads"] == len(lines)
    assert int(want["supers"].sum()) > uncut_supers(text, ft, k, m)
    return want


def check_long_read_parts(lib, k, m, fmt, both=True):
    """ReadType::long_read parts on the plain path, as test_long_read_parts_go_through_the_kernels: with title, CRLF behind the title, a continuation without
    title, a last part ending in an end of line, a part shorter than k"""
    rng = np.random.default_rng(7100 + k)

    def body_of(n):  # an invalid symbol every 1500 symbols or so: stretches of valid k-mers at every k, across the piece starts
        b = bytearray(rnd(rng, n))
        for at in rng.integers(0, n, size=n // 1500 + 1):
            b[at] = ord("N")
        return bytes(b)

    line_cap = piece_line_cap(k)
    stride = line_cap - k + 1
    ft, marker = (1, b"@") if fmt == "fq" else (0, b">")
    kw = dict(long_read=True, m=m, both=both)
    body = body_of(3 * stride + 1234)
    w = check_plain(lib, marker + b"read 1 of a long-read file\n" + body, ft, k, line_cap, **kw)
    assert w["n_reads"] == 1 and w["pieces"] == 4  # the title's end of line is symbol 0 of the stream
    returns, _ = getseq_returns(marker + b"t\n" + body, ft, k, 1 << 17, True)
    assert int(w["supers"].sum()) > sum(int(S1.split_stream(q, k, m)[0].size) for q in returns)  # the marks of k_s1_mark_raw did cut
    w = check_plain(lib, marker + b"t\r\n" + body[:3000], ft, k, line_cap, **kw)  # CRLF behind the title: two invalid symbols in front
    assert w["n_reads"] == 1 and w["pieces"] == 1
    cont = body[-(k - 1):] + body_of(2 * stride + 17)  # a continuation: no title, no read counted
    w = check_plain(lib, cont, ft, k, line_cap, **kw)
    assert w["n_reads"] == 0 and w["pieces"] == 3
    w = check_plain(lib, cont[:500] + b"\n", ft, k, line_cap, **kw)  # the last part of a FASTQ read: the end of line comes along as an invalid symbol
    assert w["n_reads"] == 0 and w["pieces"] == 1
    w = check_plain(lib, b"ACGT", ft, k, line_cap, **kw)  # shorter than a k-mer
    assert int(w["kmers"].sum()) == 0 and int(w["supers"].sum()) == 0


# ---- (c) the second cut attempt
def retry_text(n_reads, seed=3):
    """FASTA, random reads of 150 symbols: at a narrow window nearly every k-mer is a super-k-mer of its own"""
    rng = np.random.default_rng(seed)
    reads = [rnd(rng, 150) for _ in range(n_reads)]
    return _records_text("fa", b"\n", reads), n_codes(reads)


def check_retry(lib, k, m, n_reads):
    text, codes = retry_text(n_reads)
    want = check_plain(lib, text, 0, k, 1 << 17, m=m)
    # the precondition: the first attempt of s1_split_part (room for codes / sk_guess_div + 4096 super-k-mers) was too small
    assert int(want["supers"].sum()) > codes // SK_GUESS_DIV + SK_GUESS_ADD
    return want


# ---- (d) the sorted emit
def sorted_walk_text(supers):
    """(text, k, m) of a FASTQ part at (14, 11) with more than `supers` super-k-mers: several tiles of k_s1_emit_sorted, so its look-back walks"""
    k, m = 14, 11
    rng = np.random.default_rng(41)
    reads = [rnd(rng, int(rng.integers(100, 200))) for _ in range(40)] + [b"A" * 400, rnd(rng, 90) + b"N" + rnd(rng, 90)]
    while n_supers(reads, k, m) <= supers:
        reads += [rnd(rng, int(rng.integers(100, 200))) for _ in range(8)]
    return _records_text("fq", b"\n", reads), k, m
