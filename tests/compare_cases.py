"""`kmc_tools compare`, `check` and `info`: the compare restated on Python ints — no code shared with the kernels —, the planted pairs of databases, the helper that
runs kmc_hip_db_compare_device on KMC1 bodies, and the command lines recorded under tests/golden/toolsline_* (stdout, stderr and exit status of the reference).
TEST INFRASTRUCTURE shared by tests/make_compare_golden.py, tests/test_compare_emulated.py and tests/test_gpu_compare.py."""
from __future__ import annotations

import json
import os

import numpy as np

import kff_cases as K
import query_cases as Q
import setops_cases as S

ROOT = S.ROOT
GOLDEN = S.GOLDEN
U32 = S.U32
KINDS = ("equal", "counter", "kmer", "a_ended", "b_ended")
RESULT = ("kind", "ordinal", "n_a", "n_b", "counter_a", "counter_b", "record_a", "record_b")
THREADS = 256  # threads of a k_db_compare workgroup, and records of a compaction tile


# ---- the semantics (operations.h:258-295 over kmc1_db_reader.h:574-576,618)
def restate(a, b, a_cut=(1, U32), b_cut=(1, U32)) -> dict:
    """a, b: (kmers, counts) in ascending order; *_cut: (cutoff_min, cutoff_max) -> the eight result words by name"""
    pa, pb = ([(j, x, c) for j, (x, c) in enumerate(zip(*d)) if cut[0] <= c <= cut[1]] for d, cut in ((a, a_cut), (b, b_cut)))
    res = dict.fromkeys(RESULT, 0)
    res.update(n_a=len(pa), n_b=len(pb))
    i = next((i for i, (ra, rb) in enumerate(zip(pa, pb)) if ra[2] != rb[2] or ra[1] != rb[1]), None)
    if i is None and len(pa) == len(pb):
        return res
    if i is None:
        i, res["kind"] = min(len(pa), len(pb)), 3 if len(pa) < len(pb) else 4
    else:
        res["kind"] = 1 if pa[i][2] != pb[i][2] else 2  # the counter first
    res["ordinal"] = i
    for q, present, body in (("a", pa, a), ("b", pb, b)):
        res["counter_" + q], res["record_" + q] = (present[i][2], present[i][0]) if i < len(present) else (0, len(body[0]))
    return res


# ---- the device call on bodies
class CompareContext(K.KffContext):
    """K.KffContext (set operations, transform, KFF import) with the reads query and kmc_hip_db_compare_device: the interface of capi.Context on a library given by path"""

    def __init__(self, path):
        super().__init__(path)
        C, capi = self.C, self.capi
        vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
        self.L.kmc_hip_db_compare_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.POINTER(capi.DbView), u64p]
        self.L.kmc_hip_db_query_reads_device.argtypes = [vp, C.c_int, C.POINTER(capi.DbView), C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, u64p]


def _bind():
    from kmc_amd import capi

    CompareContext.db_compare_device = capi.Context.db_compare_device  # the binding under test is the one the product ships
    CompareContext.db_query_reads_device = Q.LibContext.db_query_reads_device


_bind()


def run_device(ctx, k, a_body, b_body, a_cut=(1, U32), b_cut=(1, U32)) -> dict:
    """a_body, b_body: (p, counter bytes, lut, recs) -> the dict of kmc_hip_db_compare_device"""
    from kmc_amd import capi

    allocs = []

    def up(arr):
        d = ctx.malloc(arr.nbytes + 256)
        allocs.append(d)
        if arr.nbytes:
            ctx.h2d(d, np.ascontiguousarray(arr))
        return d

    try:
        views = []
        for (p, cb, lut, recs), cut in ((a_body, a_cut), (b_body, b_cut)):
            n = recs.size // ((k - p) // 4 + cb)
            views.append(capi.DbView(up(recs) if n else None, n, up(np.asarray(lut, dtype=np.uint64)), p, cb, cut[0], cut[1]))  # an empty input: d_recs NULL
        return ctx.db_compare_device(k, views[0], views[1])
    finally:
        for d in allocs:
            ctx.free(d)


def check_case(ctx, k, a, b, a_fmt, b_fmt, a_cut=(1, U32), b_cut=(1, U32)) -> dict:
    """a, b: (kmers, counts); *_fmt: (p, counter bytes). All eight words of the device call on the encoded bodies must be the restatement's."""
    bodies = [(p, cb, *S.encode_body(k, p, cb, *x)) for x, (p, cb) in ((a, a_fmt), (b, b_fmt))]
    want = restate(a, b, a_cut, b_cut)
    got = run_device(ctx, k, bodies[0], bodies[1], a_cut, b_cut)
    assert got == want, (got, want)
    return got


# ---- planted pairs
WIDTHS = [(27, 3), (32, 4), (33, 5), (64, 4), (65, 5), (127, 3), (224, 4)]  # SIZE 1, 1, 2, 2, 3, 4, 7: as the KFF planted cases
WIDTH_IDS = [f"{k}-p{p}" for k, p in WIDTHS]


def tile_records(k, steps=8):
    """whole records in front of the first tile seam of k_db_compare: a tile is THREADS x steps words, a record (k + 31) // 32 + 1 of them"""
    return THREADS * steps // ((k + 31) // 32 + 1)


def seam_records(k, steps=8, n=None):
    """the records that hold the last word of a wave's 64 words, or of a tile, and their neighbours (below n)"""
    w = (k + 31) // 32 + 1
    out = set()
    for words in (64, 128, THREADS * steps, 2 * THREADS * steps, 3 * THREADS * steps):
        r = (words - 1) // w  # the record of the last word in front of the seam
        out |= {r - 1, r, r + 1, r + 2}
    return sorted(x for x in out if x >= 0 and (n is None or x < n))


def planted_cases(k, p, steps=8, seed=3, reduced=False):
    """-> list of (name, a, b, kwargs of check_case). Databases of up to three tiles and a third; differences by kind and by place. A k-mer is changed in place by one
    bit that keeps the order (the lowest bit of the lowest word, bit 1 of the highest symbol's neighbour), so both inputs stay ascending sets."""
    rng = np.random.default_rng(seed + k)
    tile = tile_records(k, steps)
    n_max = 3 * tile + tile // 3
    # even k-mers, so that the lowest bit can be set without meeting a neighbour; the top symbol 0..2, so that the highest word can change upwards
    base = sorted({(int.from_bytes(rng.bytes((2 * k + 7) // 8), "big") & ((1 << (2 * k)) - 1) & ~1) for _ in range(n_max + 64)})
    top_bit = 2 * k - 1
    base = [x & ~(1 << top_bit) for x in base]
    base = sorted(set(base))[:n_max]
    assert len(base) == n_max
    cnt = [int(c) for c in rng.integers(1, 250, size=n_max)]
    fm = dict(a_fmt=(p, 1), b_fmt=(p, 1))
    cases = []

    def pair(n):
        return (base[:n], cnt[:n]), (base[:n], cnt[:n])

    def changed(d, i, counter=None, kmer_bit=None):
        ks, cs = list(d[0]), list(d[1])
        if counter is not None:
            cs[i] = counter
        if kmer_bit is not None:
            ks[i] = ks[i] ^ (1 << kmer_bit)
            assert (i == 0 or ks[i - 1] < ks[i]) and (i + 1 == len(ks) or ks[i] < ks[i + 1]), "the changed k-mer left its place"
        return ks, cs

    sizes = [0, 1, tile - 1, tile, tile + 1, n_max]
    for n in sizes:
        a, b = pair(n)
        cases.append((f"equal_n{n}", a, b, fm))
        if n == 0:
            continue
        for name, i in (("first", 0), ("last", n - 1)):
            cases.append((f"counter_{name}_n{n}", a, changed(b, i, counter=cnt[i] % 250 + 1), fm))
            if not reduced:
                cases.append((f"kmer_low_{name}_n{n}", a, changed(b, i, kmer_bit=0), fm))
    n = n_max
    a, b = pair(n)
    # the highest key word: the top bit of the last record only (every record above it would leave the order otherwise)
    cases.append(("kmer_high_word_last", a, changed(b, n - 1, kmer_bit=top_bit), fm))
    cases.append(("kmer_high_word_last_in_a", changed(a, n - 1, kmer_bit=top_bit), b, fm))
    for i in seam_records(k, steps, n):
        cases.append((f"counter_at_seam_{i}", a, changed(b, i, counter=cnt[i] % 250 + 1), fm))
        if not reduced or i % 2:
            cases.append((f"kmer_at_seam_{i}", changed(a, i, kmer_bit=0), b, fm))
    mid = n // 2 + 1
    cases.append(("both_counter_and_kmer", a, changed(b, mid, counter=cnt[mid] % 250 + 1, kmer_bit=0), fm))  # kind 1 must win
    far = changed(changed(b, 5, kmer_bit=0), n - 3, counter=cnt[n - 3] % 250 + 1)
    cases.append(("two_far_apart", a, far, fm))
    # the record across the first tile seam differs in its LAST word only (the counter), and an earlier record of the tile in front differs too: with the tiles taken last
    # to first the seam's record is published first, and the tile in front — the one its first word lies in — must still be walked
    seam = THREADS * steps // ((k + 31) // 32 + 1)  # where the tile is no multiple of the record, the record that lies across the seam; the first one behind it otherwise
    two = changed(changed(b, seam, counter=cnt[seam] % 250 + 1), 9, counter=cnt[9] % 250 + 1)
    cases.append(("two_with_the_later_across_a_tile_seam", a, two, fm))
    cases.append(("a_one_shorter", (base[:n - 1], cnt[:n - 1]), b, fm))
    cases.append(("b_one_shorter", a, (base[:n - 1], cnt[:n - 1]), fm))
    cases.append(("empty_against_non_empty", ([], []), b, fm))
    cases.append(("non_empty_against_empty", a, ([], []), fm))
    cases.append(("a_short_and_an_earlier_difference", (base[:n - 1], cnt[:n - 1]), changed(b, 3, counter=cnt[3] % 250 + 1), fm))
    # views
    if k == 27:
        cases.append(("prefix_3_against_7", a, b, dict(a_fmt=(3, 1), b_fmt=(7, 1))))
        cases.append(("prefix_3_against_7_kmer_differs", a, changed(b, mid, kmer_bit=0), dict(a_fmt=(3, 1), b_fmt=(7, 1))))
    cases.append(("counter_size_1_against_2", a, b, dict(a_fmt=(p, 1), b_fmt=(p, 2))))
    big = changed(b, mid, counter=cnt[mid] + 256)
    cases.append(("counter_size_1_against_2_high_byte_differs", a, big, dict(a_fmt=(p, 1), b_fmt=(p, 2))))
    # cutoffs: counts 300 and 2 are cut by (3, 255); B holds extra records that its cutoffs remove, or both hold records only one side's cutoffs remove
    cut = (3, 255)

    def with_extra(d, where):
        """d with records of count 300 / 2 added in front of the records at `where` (k-mers: the odd neighbours below)"""
        ks, cs = list(d[0]), list(d[1])
        for j, i in enumerate(sorted(where, reverse=True)):
            ks.insert(i, d[0][i] - 1)
            cs.insert(i, 300 if j % 2 else 2)
        return ks, cs

    kept = (base[1:n], [max(c, 3) for c in cnt[1:n]])  # base[0] may be 0: no room below it
    m = len(kept[0])
    f2 = dict(a_fmt=(p, 2), b_fmt=(p, 2))
    for name, where in (("first", [0]), ("last_but_one", [m - 1]), ("every_second", list(range(0, m, 2))), ("tile_seams", [x for x in seam_records(k, steps, m)])):
        cases.append((f"cut_makes_equal_{name}", kept, with_extra(kept, where), dict(f2, b_cut=cut)))
        cases.append((f"uncut_differs_{name}", kept, with_extra(kept, where), f2))
        cases.append((f"cut_in_a_{name}", with_extra(kept, where), kept, dict(f2, a_cut=cut)))
    behind = (kept[0] + [kept[0][-1] + 1], kept[1] + [2])
    cases.append(("cut_last_record", kept, behind, dict(f2, b_cut=cut)))
    cases.append(("all_of_b_cut", kept, kept, dict(f2, b_cut=(1000, 2000))))
    cases.append(("all_of_both_cut", kept, (kept[0][: m // 2], kept[1][: m // 2]), dict(f2, a_cut=(1000, 2000), b_cut=(1000, 2000))))
    cases.append(("cut_makes_different", kept, kept, dict(f2, b_cut=(1, 100))))  # B alone loses what is counted more than 100 times
    thinned = with_extra(kept, list(range(0, m, 2)))
    at = thinned[0].index(kept[0][m - 2])
    cases.append(("cut_and_a_difference_behind", kept, changed(thinned, at, counter=251), dict(f2, b_cut=cut)))
    return cases


# ---- the recorded command lines: (name, arguments with {g} = tests/golden)
RC_ONLY_27 = "CGCAGAGAAACGCGAGTCAGGTTTTTT"  # the reverse complement of the first k-mer of setops_k27_a: the database holds canonical k-mers
LINES = [
    ("cmp_k33_kmc1_kmc2", ["compare", "{g}/setops_k33_a", "{g}/setops_k33_raw_a"]),
    ("cmp_k33_kmc2_kmc1", ["compare", "{g}/setops_k33_raw_a", "{g}/setops_k33_a"]),
    ("cmp_k27_a_b", ["compare", "{g}/setops_k27_a", "{g}/setops_k27_b"]),
    ("cmp_k55_a_b", ["compare", "{g}/setops_k55_a", "{g}/setops_k55_b"]),
    ("cmp_k27_kff", ["compare", "{g}/setops_k27_a", "{g}/kff_k27_a.kff"]),
    ("cmp_k33_kff", ["compare", "{g}/setops_k33_a", "{g}/kff_k33_a"]),  # the name + '.kff'
    ("cmp_k55_kff", ["compare", "{g}/kff_k55_a.kff", "{g}/setops_k55_a"]),
    ("cmp_k33_kmc2_kff", ["compare", "{g}/setops_k33_raw_a", "{g}/kff_k33_a.kff"]),
    ("cmp_k27_kff_cs2", ["compare", "{g}/kff_k27_a.kff", "{g}/kff_k27_a_cs2.kff"]),
    ("cmp_k27_multi_self", ["compare", "{g}/kff_k27_multi.kff", "{g}/kff_k27_multi.kff"]),
    ("cmp_k27_kff_ci2", ["compare", "{g}/setops_k27_a", "-ci2", "{g}/kff_k27_a.kff"]),
    ("cmp_k27_self_ci2_one_side", ["compare", "{g}/setops_k27_a", "{g}/setops_k27_a", "-ci2"]),
    ("cmp_k27_self_ci2_both", ["compare", "{g}/setops_k27_a", "-ci2", "{g}/setops_k27_a", "-ci2"]),
    ("cmp_k27_self_ci2_cx9_both", ["compare", "{g}/setops_k27_a", "-ci2", "-cx9", "{g}/kff_k27_a.kff", "-cx9", "-ci2"]),
    ("cmp_k27_a_ends_first", ["compare", "{g}/setops_k27_a", "-ci200", "{g}/setops_k27_b"]),
    ("cmp_k27_b_ends_first", ["compare", "{g}/setops_k27_a", "{g}/setops_k27_b", "-ci200"]),
    ("cmp_k27_both_empty", ["compare", "{g}/setops_k27_a", "-ci200", "{g}/setops_k27_b", "-ci200"]),
    ("chk_k27_present", ["check", "{g}/setops_k27_a", "AAAAAAGGGATCCTCGCAGGTCGCAAA"]),
    ("chk_k27_first", ["check", "{g}/setops_k27_a", "AAAAAACCTGACTCGCGTTTCTCTGCG"]),
    ("chk_k27_last", ["check", "{g}/setops_k27_a", "TTTCGTACGAACAATCTTGACGGCAAA"]),
    ("chk_k27_lower_case", ["check", "{g}/setops_k27_a", "aaaaaaGGGATCCTCGCAGGTcgcaaa"]),
    ("chk_k27_absent", ["check", "{g}/setops_k27_a", "AAAAAAGGGATCCTCGCAGGTCGCAAC"]),
    ("chk_k27_rc_only", ["check", "{g}/setops_k27_a", RC_ONLY_27]),
    ("chk_k27_below_ci", ["check", "{g}/setops_k27_a", "-ci5", "AAAAAAGGGATCCTCGCAGGTCGCAAA"]),
    ("chk_k27_at_ci", ["check", "{g}/setops_k27_a", "-ci4", "AAAAAAGGGATCCTCGCAGGTCGCAAA"]),
    ("chk_k27_at_cx", ["check", "{g}/setops_k27_union_a_ci2_b_cx5", "-cx5", "AAAAACACCTGCTCATACGCACTGCCA"]),  # a counter equal to cutoff_max: 0 in this mode alone
    ("chk_k27_below_cx", ["check", "{g}/setops_k27_union_a_ci2_b_cx5", "-cx6", "AAAAACACCTGCTCATACGCACTGCCA"]),
    ("chk_k27_ci_and_cx", ["check", "{g}/setops_k27_a", "-cx4", "-ci4", "AAAAAAGGGATCCTCGCAGGTCGCAAA"]),
    ("chk_k33_kmc2_present", ["check", "{g}/setops_k33_raw_a", "CACCGCGCCTAGTGCTCCGCACCACCGTAGGTG"]),
    ("chk_k33_kmc2_last", ["check", "{g}/setops_k33_raw_a", "TTTATAACTATTAGGAGACGTTGACACCGAAAA"]),
    ("chk_k33_kmc2_absent", ["check", "{g}/setops_k33_raw_a", "CACCGCGCCTAGTGCTCCGCACCACCGTAGGTT"]),
    ("chk_k33_kmc2_rc_only", ["check", "{g}/setops_k33_raw_a", "CACCTACGGTGGTGCGGAGCACTAGGCGCGGTG"]),
    ("chk_k27_kff_present", ["check", "{g}/kff_k27_a.kff", "AAAAAAGGGATCCTCGCAGGTCGCAAA"]),
    ("chk_k27_kff_absent", ["check", "{g}/kff_k27_a.kff", "AAAAAAGGGATCCTCGCAGGTCGCAAC"]),  # a KFF file that does not hold it: no line at all
    ("chk_k27_kff_rc_only", ["check", "{g}/kff_k27_a", RC_ONLY_27]),
    ("chk_k27_kff_at_cx", ["check", "{g}/kff_k27_a.kff", "-cx4", "AAAAAAGGGATCCTCGCAGGTCGCAAA"]),
    ("chk_k27_multi_present", ["check", "{g}/kff_k27_multi.kff", "CACGTTCTTGTGTGTCGGTTGTGACTA"]),
    ("chk_k27_too_short", ["check", "{g}/setops_k27_a", "AAAAAAGGGATCCTCGCAGGTCGCAA"]),
    ("chk_k27_too_long", ["check", "{g}/kff_k27_a.kff", "AAAAAAGGGATCCTCGCAGGTCGCAAAA"]),
    ("chk_k27_with_n", ["check", "{g}/setops_k27_a", "AAAAAAGGGATCCNCGCAGGTCGCAAA"]),
    ("chk_k27_kff_with_n", ["check", "{g}/kff_k27_a.kff", "NAAAAAGGGATCCTCGCAGGTCGCAAA"]),
    ("info_k27_kmc1", ["info", "{g}/setops_k27_a"]),
    ("info_k55_kmc1", ["info", "{g}/setops_k55_b"]),
    ("info_k33_kmc2", ["info", "{g}/setops_k33_raw_a"]),
    ("info_k27_kff", ["info", "{g}/kff_k27_a.kff"]),
    ("info_k27_kff_cs2", ["info", "{g}/kff_k27_a_cs2"]),
    ("info_k27_kff_multi", ["info", "{g}/kff_k27_multi.kff"]),
]
LINE_IDS = [ln[0] for ln in LINES]
# the two lines a GPU test runs against a live kmc_tools as well
LIVE_LINES = ("cmp_k33_kmc2_kff", "cmp_k27_self_ci2_one_side")


def argv_of(line) -> list:
    return [a.format(g=GOLDEN) for a in line[1]]


def golden_file(line) -> str:
    return os.path.join(GOLDEN, f"toolsline_{line[0]}.json")


def read_golden(line) -> dict:
    """-> dict(stdout, stderr, status) as kmc_tools -t1 -hp left them"""
    with open(golden_file(line)) as f:
        return json.load(f)


def compare_inputs(line):
    """the two inputs of a recorded compare line as the restatement takes them: ((kmers, counts), (cutoff_min, cutoff_max)) x 2 — from the files, through dbio and the
    restatements of the KMC1 body and of the KFF container, not through the code under test"""
    from kmc_amd import dbio

    out = []
    argv = argv_of(line)[1:]
    pos = 0
    while pos < len(argv):
        path, opts = argv[pos], []
        pos += 1
        while pos < len(argv) and argv[pos].startswith("-"):
            opts.append(argv[pos])
            pos += 1
        if dbio.is_kff(path) and not os.path.exists(path + ".kmc_pre"):
            raw = open(dbio.kff_path(path), "rb").read()
            h, sections = K.file_sections(raw)
            recs = sorted((x, c) for ks, cs in sections for x, c in zip(ks, cs))
            body, lo, hi = ([x for x, _ in recs], [c for _, c in recs]), h["min_count"], h["max_count"]
        else:
            db = dbio.read_database(path)
            if db.kmc2:
                recs = sorted((x, c) for r, lut in db.bins for x, c in zip(*S.decode_body(db.kmer_len, db.lut_prefix_len, db.counter_size, np.concatenate([[0], np.cumsum(lut)[:-1]]), r)))
                body = ([x for x, _ in recs], [c for _, c in recs])
            else:
                body = S.decode_body(db.kmer_len, db.lut_prefix_len, db.counter_size, db.lut, db.recs)
            lo, hi = db.min_count, db.max_count
        out.append((body, (S._opt(opts, "-ci") or lo, S._opt(opts, "-cx") or hi)))
    return out


def report(res: dict) -> tuple:
    """what kmc_tools prints for a restated result, and its exit status"""
    kind = KINDS[res["kind"]] if isinstance(res["kind"], int) else res["kind"]
    if kind == "equal":
        return "DB Equals\n", 0
    return ("one of input is not finished\n" if kind in ("a_ended", "b_ended") else "") + "DB Differs\n", 1
