"""TEST INFRASTRUCTURE shared by tests/test_smallk_db_emulated.py (CPU, the product's host library over the emulated HIP runtime), tests/test_gpu_smallk_db.py (-m gpu,
libkmc_hip.so) and tests/make_smallk_db_golden.py: the small-k table (k <= 13) as a database on the device (kmc_hip_smallk_tally / _view_device, capi.SmallK,
`python -m kmc_amd.tools count-small`).

The restatement is numpy over the whole table: CSmallKCompleter::CompleteKMCFormat / CompleteKFFFormat (kmc_core/kb_completer.h:149-378) — an entry c != 0 is unique,
c < ci below, c > cx above, the rest kept in index order with min(c, counter_max); the KMC1 record is the low (k - p) / 4 bytes of the index, most significant first, then
the counter bytes least significant first, LUT entry j the kept entries in front of index j x 4^(k - p); the KFF record is ceil(k / 4) index bytes and data_size counter
bytes, both most significant first. tests/golden/smallkdb_* (tests/make_smallk_db_golden.py: what `kmc` itself wrote with its small-k optimisation on) pins it and the
verb to the reference. Nothing here reads a file outside tests/."""
import ctypes as C
import os

import numpy as np

import count_cases as CC
import setops_cases as S
from kmc_amd import capi

EINVAL, ECAPACITY = -1, -5
GOLDEN = CC.GOLDEN
_U = np.uint64
POISON = 0xA5


# ---- the restatement
def byte_log(x: int) -> int:
    return 1 if x < 1 << 8 else 2 if x < 1 << 16 else 3 if x < 1 << 24 else 4


def counter_size(cx: int, cm: int) -> int:
    """defs.h:154-159"""
    return 0 if cm == 1 else min(byte_log(cx), byte_log(cm))


def classify(table, ci, cx):
    """-> (kept mask, [unique, below, above, kept])"""
    t = np.asarray(table, dtype=np.uint64)
    nz = t != _U(0)
    below = nz & (t < _U(ci))
    above = nz & ~below & (t > _U(cx))
    kept = nz & ~below & ~above
    return kept, [int(nz.sum()), int(below.sum()), int(above.sum()), int(kept.sum())]


def complete(table, k, ci, cx, cm, p=0, framing=0, data_size=0) -> dict:
    """-> dict(recs uint8[], lut uint64[] (KMC1), stats [4], counter_size, rec_bytes)"""
    t = np.asarray(table, dtype=np.uint64)
    assert t.size == 1 << (2 * k)
    kept, stats = classify(t, ci, cx)
    idx = np.flatnonzero(kept).astype(np.uint64)
    c = np.minimum(t[kept], _U(cm))
    cs = counter_size(cx, cm)
    if framing == 0:
        sb = (k - p) // 4
        cols = [(idx >> _U(8 * (sb - 1 - j))) & _U(255) for j in range(sb)] + [(c >> _U(8 * j)) & _U(255) for j in range(cs)]
        before = np.concatenate([[0], np.cumsum(kept)]).astype(np.uint64)
        lut = before[np.arange(1 << (2 * p), dtype=np.int64) << (2 * (k - p))]
    else:
        kb = (k + 3) // 4
        cols = [(idx >> _U(8 * (kb - 1 - j))) & _U(255) for j in range(kb)] + [(c >> _U(8 * (data_size - 1 - j))) & _U(255) for j in range(data_size)]
        lut = None
    recs = np.stack(cols, axis=1).astype(np.uint8).reshape(-1) if idx.size else np.zeros(0, dtype=np.uint8)
    return dict(recs=recs, lut=lut, stats=stats, counter_size=cs, rec_bytes=len(cols))


def legal_prefixes(k):
    return [p for p in range(1, k + 1) if (k - p) % 4 == 0]


# ---- cutoffs and counter_max by the counter size they give: 1, 2, 3, 4 bytes (the last one with a cutoff_max above 2^32: counts beyond 32 bits are kept and clamped)
PARAMS = {1: (2, 200, 255), 2: (3, 60000, 300), 3: (2, (1 << 24) - 1, 10**9), 4: (1, 1 << 33, (1 << 32) - 1)}
for _cs, (_ci, _cx, _cm) in PARAMS.items():
    assert counter_size(_cx, _cm) == _cs
FILLS = ("zero", "all_kept", "first", "last", "all_below", "all_above", "alternate", "half", "sparse64", "seam_end", "seam_start", "drawn")
DEFAULT_TILE = 2048


def drawn_values(ci, cx, cm):
    """the counters the issue lists: around both cutoffs, around counter_max, around 2^32, and 2^63"""
    return np.array([ci - 1, ci, cx, cx + 1, cm, cm + 1, (1 << 32) - 1, 1 << 32, 1 << 63], dtype=np.uint64)


def planted(k, fill, ci, cx, cm, seed=0, tile=DEFAULT_TILE):
    """a table of 4^k counters; kept values are drawn from [ci, min(cx, ci + 1000)], so that some exceed a small counter_max"""
    n = 1 << (2 * k)
    rng = np.random.default_rng([k, FILLS.index(fill), seed])
    kept_values = lambda m: rng.integers(ci, min(cx, ci + 1000) + 1, size=m, dtype=np.uint64)  # noqa: E731
    t = np.zeros(n, dtype=np.uint64)
    seam = tile if n > tile else n // 2
    if fill == "all_kept":
        t[:] = kept_values(n)
    elif fill == "first":
        t[0] = ci
    elif fill == "last":
        t[n - 1] = cx
    elif fill == "all_below":
        t[:] = max(ci - 1, 0)  # ci == 1: nothing is below, the table stays empty
    elif fill == "all_above":
        t[:] = _U(cx + 1)
    elif fill == "alternate":
        t[::2] = kept_values((n + 1) // 2)
    elif fill in ("half", "sparse64"):
        at = rng.random(n) < (0.5 if fill == "half" else 1 / 64)
        t[at] = kept_values(int(at.sum()))
    elif fill == "seam_end":
        run = min(300, seam)
        t[seam - run:seam] = kept_values(run)
    elif fill == "seam_start":
        run = min(300, n - seam)
        t[seam:seam + run] = kept_values(run)
    elif fill == "drawn":
        t[:] = drawn_values(ci, cx, cm)[rng.integers(0, 9, size=n)]
        t[rng.random(n) < 0.25] = 0
    return t


# ---- the library under test
class SkContext(S.LibContext):
    """S.LibContext + the small-k entries and the database entries a small-k view goes on to: the interface of capi.Context on a library given by path"""

    def __init__(self, path):
        super().__init__(path)
        L, vp, u64p = self.L, C.c_void_p, C.POINTER(C.c_uint64)
        capi.bind_smallk_db(L)
        L.kmc_hip_split_covers.argtypes = [C.c_uint32]
        L.kmc_hip_smallk_open.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32]
        L.kmc_hip_smallk_part.argtypes = [vp, C.c_int, C.c_int, C.POINTER(capi.SplitParams), vp, C.c_uint64, u64p, u64p]
        L.kmc_hip_smallk_read.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, vp]
        L.kmc_hip_smallk_close.argtypes = [vp, C.c_int]
        L.kmc_hip_db_histogram_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.c_uint32, C.c_uint32, C.c_uint64, vp, u64p]
        L.kmc_hip_db_dump_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, vp, C.c_uint64, u64p, u64p]
        L.kmc_hip_db_kff_export_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, vp, C.c_uint64]

    def last_error(self) -> str:
        return self.L.kmc_hip_last_error(self.h).decode()


for _name in ("db_histogram_device", "db_dump_device", "db_set_op_device", "db_kff_export_device", "_need"):  # capi.Context's own (they use only self.L, self.h, self._chk)
    setattr(SkContext, _name, getattr(capi.Context, _name))


class Planted:
    """a table uploaded to the device (behind 16 bytes, so that `offset` 8 gives a table that is not 16-byte aligned)"""

    def __init__(self, ctx, table, offset=0):
        self.ctx, self.n = ctx, table.size
        self.base = ctx.malloc(table.nbytes + 32)
        self.d = self.base + offset
        buf = np.zeros(table.size + 4, dtype=np.uint64)
        buf[offset // 8:offset // 8 + table.size] = table
        ctx.h2d(self.base, buf)

    def free(self):
        self.ctx.free(self.base)


def run_tally(ctx, d_table, k, ci, cx):
    """-> (rc, stats list)"""
    st = np.full(4, 0xDEAD, dtype=np.uint64)
    rc = ctx.L.kmc_hip_smallk_tally(ctx.h, 0, d_table or None, k, ci, cx, st.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, [int(x) for x in st]


def run_view(ctx, d_table, k, ci, cx, cm, p=0, framing=0, data_size=0, n_out=None, n_lut=None, both=1, guard=64):
    """kmc_hip_smallk_view_device into poisoned buffers of n_out record bytes and n_lut LUT entries (by default: exactly what the restatement's sizes are, which
    the caller passes) with `guard` bytes behind each -> dict(rc, recs (the whole buffer), lut (the whole buffer), view, n_kmers, stats)"""
    u64p = C.POINTER(C.c_uint64)
    d_out, d_lut = ctx.malloc(n_out + guard), ctx.malloc(8 * n_lut + guard)
    try:
        ctx.h2d(d_out, np.full(n_out + guard, POISON, dtype=np.uint8))
        ctx.h2d(d_lut, np.full(8 * n_lut + guard, POISON, dtype=np.uint8))
        v, n, st = capi.DbView(), C.c_uint64(0xDEAD), np.full(4, 0xDEAD, dtype=np.uint64)
        rc = ctx.L.kmc_hip_smallk_view_device(ctx.h, 0, d_table or None, k, both, ci, cx, cm, framing, p, data_size, d_out, n_out, d_lut if framing == 0 else None,
                                              C.byref(v), C.byref(n), st.ctypes.data_as(u64p))
        recs, lut = np.zeros(n_out + guard, dtype=np.uint8), np.zeros(8 * n_lut + guard, dtype=np.uint8)
        ctx.d2h(recs, d_out)
        ctx.d2h(lut, d_lut)
    finally:
        ctx.free(d_out)
        ctx.free(d_lut)
    return dict(rc=rc, recs=recs, lut=lut, view=v, n_kmers=n.value, stats=[int(x) for x in st], d_out=d_out, d_lut=d_lut)


def check_view(ctx, d_table, table, k, ci, cx, cm, p=0, framing=0, data_size=0, want=None):
    """one view call against the restatement, byte for byte: body, every LUT word, the guard bytes behind both, the tallies, n_kmers and the view's fields"""
    want = want or complete(table, k, ci, cx, cm, p, framing, data_size)
    n_out, n_lut = want["recs"].size, (1 << (2 * p)) if framing == 0 else 0
    got = run_view(ctx, d_table, k, ci, cx, cm, p, framing, data_size, n_out, n_lut)
    assert got["rc"] == 0, (got["rc"], ctx.last_error())
    assert got["stats"] == want["stats"] and got["n_kmers"] == want["stats"][3], (got["stats"], want["stats"], got["n_kmers"])
    bad = np.flatnonzero(got["recs"][:n_out] != want["recs"])
    assert bad.size == 0, (int(bad[0]), int(bad.size), want["rec_bytes"])
    assert (got["recs"][n_out:] == POISON).all(), "bytes behind the body were written"
    if framing == 0:
        lut = got["lut"][:8 * n_lut].view(np.uint64)
        bad = np.flatnonzero(lut != want["lut"])
        assert bad.size == 0, (int(bad[0]), int(bad.size), int(lut[bad[0]]), int(want["lut"][bad[0]]))
        v = got["view"]
        assert (v.d_recs, v.n_recs, v.d_lut, v.lut_prefix_len, v.counter_size, v.cutoff_min, v.cutoff_max) == (got["d_out"], want["stats"][3], got["d_lut"], p, want["counter_size"],
                                                                                                                 min(ci, 0xFFFFFFFF), cx)
    assert (got["lut"][8 * n_lut:] == POISON).all(), "bytes behind the LUT were written"
    return want


# ---- the recorded runs of `kmc` itself (tests/make_smallk_db_golden.py): name -> (flags, [(file name, format, bytes)], "kmc" or "kff")
def _short_reads(seed):
    rng = np.random.default_rng(seed)
    return [CC._rnd(rng, int(n)) for n in rng.integers(1, 9, size=40)] + [b"ACGTNACGTN", b"NNNNNNNNNNNN"]


def _fm_seqs(seed):
    rng = np.random.default_rng(seed)
    g = CC._rnd(rng, 1500)
    return [g[:700], g[650:1500], g[100:400] + b"NNNN" + g[400:600].lower(), CC._rnd(rng, 9), g[900:1300]]


def _cases():
    c = {}
    fq = lambda name, seed, k: [("smallkdb_%s.fq" % name, "fq", CC.fastq_text(CC.golden_reads(seed, max(k, 2))))]  # noqa: E731
    c["k1"] = (["-k1"], fq("k1", 201, 1), "kmc")
    c["k3_ci1"] = (["-k3", "-ci1"], fq("k3_ci1", 203, 3), "kmc")
    c["k4"] = (["-k4"], fq("k4", 204, 4), "kmc")
    c["k5"] = (["-k5"], fq("k5", 205, 5), "kmc")
    c["k9_hc"] = (["-k9", "-hc"], fq("k9_hc", 209, 9), "kmc")
    c["k12_fm"] = (["-k12", "-fm"], [("smallkdb_k12_fm.fa", "fm", CC.multiline_text(_fm_seqs(212)))], "kmc")
    c["k13_ci1"] = (["-k13", "-ci1"], fq("k13_ci1", 213, 13), "kmc")
    c["k7_b"] = (["-k7", "-b", "-fa"], [("smallkdb_k7_b.fa", "fa", CC.fasta_text(CC.golden_reads(207, 7), b"\r\n"))], "kmc")
    c["k2_cs300"] = (["-k2", "-ci1", "-cs300"], fq("k2_cs300", 202, 2), "kmc")  # counts of several hundred: two counter bytes, some clamped
    c["k8_gz"] = (["-k8"], [("smallkdb_k8_gz.fq.gz", "fq", CC.fastq_text(CC.golden_reads(208, 8)))], "kmc")
    two = CC.golden_reads(218, 8)
    c["k8_list"] = (["-k8", "-fa"], [("smallkdb_k8_list_1.fa", "fa", CC.fasta_text(two[:35])), ("smallkdb_k8_list_2.fa", "fa", CC.fasta_text(two[25:]))], "kmc")
    c["k9_empty"] = (["-k9"], [("smallkdb_k9_empty.fq", "fq", CC.fastq_text(_short_reads(210)))], "kmc")  # no read holds a window of 9 valid symbols
    c["k4_kff"] = (["-k4"], fq("k4_kff", 224, 4), "kff")
    c["k9_kff"] = (["-k9", "-ci1", "-cx50", "-cs20"], fq("k9_kff", 229, 9), "kff")
    return c


CASES = _cases()
CASE_IDS = list(CASES)
KMC_CASE_IDS = [n for n in CASES if CASES[n][2] == "kmc"]
KFF_CASE_IDS = [n for n in CASES if CASES[n][2] == "kff"]
REF_FLAGS = ["-v", "-m2", "-sf1", "-sp2", "-sr2"]  # the reference run of every golden, as smallk_cases.check_e2e runs it


def golden_input_paths(name) -> list:
    return [os.path.join(GOLDEN, f) for f, _, _ in CASES[name][1]]


def golden_out(name) -> str:
    return os.path.join(GOLDEN, "smallkdb_" + name + "_out")


def golden_report(name) -> str:
    return os.path.join(GOLDEN, "smallkdb_" + name + "_report.txt")


def input_argument(name, tmp_dir) -> str:
    paths = golden_input_paths(name)
    if len(paths) == 1:
        return paths[0]
    lst = os.path.join(str(tmp_dir), "inputs.lst")
    with open(lst, "w") as f:
        f.write("\n".join(paths) + "\n")
    return "@" + lst


def report_lines(text: str) -> list:
    """the statistics lines of a `kmc` log or of tools.count_report, each as (label, number)"""
    out = []
    for ln in text.splitlines():
        if ("No. of" in ln or "Total no." in ln) and ":" in ln:
            label, value = ln.split(":", 1)
            out.append((label.strip(), int(value.split()[0])))
    return out


def header_of(pre: bytes) -> dict:
    """kmer_len, counter_size, lut_prefix_len, cutoff_min, cutoff_max, n_kmers of a .kmc_pre file (its 64-byte header in front of the last 8 bytes)"""
    h = np.frombuffer(pre[-72:-8], dtype=np.uint8)
    w = h[0:24].view(np.uint32)
    return dict(k=int(w[0]), counter_size=int(w[2]), p=int(w[3]), ci=int(w[4]), cx=int(w[5]), n=int(h[24:32].view(np.uint64)[0]))


# ---- the checks both test files run (ctx: an SkContext)
def with_ipt(monkeypatch, ipt):
    if ipt is None:
        monkeypatch.delenv("KMC_HIP_SMALLK_IPT", raising=False)
    else:
        monkeypatch.setenv("KMC_HIP_SMALLK_IPT", str(ipt))


def check_planted(ctx, k, fill, cs, prefixes=None, data_sizes=None, offset=0):
    """one planted table through the tally, every legal prefix length (or `prefixes`) and KFF at `data_sizes` (default: the counter size alone)"""
    ci, cx, cm = PARAMS[cs]
    table = planted(k, fill, ci, cx, cm)
    dev = Planted(ctx, table, offset)
    try:
        rc, st = run_tally(ctx, dev.d, k, ci, cx)
        assert rc == 0 and st == classify(table, ci, cx)[1], (rc, st)
        for p in (legal_prefixes(k) if prefixes is None else prefixes):
            check_view(ctx, dev.d, table, k, ci, cx, cm, p)
        for ds in (data_sizes or [cs]):
            check_view(ctx, dev.d, table, k, ci, cx, cm, framing=1, data_size=ds)
        back = np.zeros(table.size, dtype=np.uint64)
        ctx.d2h(back, dev.d)
        assert np.array_equal(back, table), "the table was modified"
    finally:
        dev.free()


# the open table: name -> (k, both, hc, file_type, [parts of text]); the parts are whole records (multi-line: what the reader hands over)
def open_table_cases():
    from test_stage1_multiline_emulated import reader_parts

    c = {}
    r = CC.golden_reads(301, 9)
    c["fq"] = (7, True, False, 1, [CC.fastq_text(r[:20]), CC.fastq_text(r[20:45]), CC.fastq_text(r[45:])])
    c["fa_b"] = (6, False, False, 0, [CC.fasta_text(r[:30]), CC.fasta_text(r[30:])])
    c["fq_hc"] = (9, True, True, 1, [CC.fastq_text(r[:33]), CC.fastq_text(r[33:])])
    parts = reader_parts(CC.multiline_text(_fm_seqs(302)), 900, 8)
    assert len(parts) >= 2
    c["fm"] = (8, True, False, 2, parts)
    return c


OPEN_IDS = ("fq", "fa_b", "fq_hc", "fm")


def check_open_table(ctx, name):
    """reads through kmc_hip_smallk_part in several parts, then d_table = NULL: the restatement over smallk_cases.smallk_table; the table reads back unchanged"""
    import smallk_cases as SK
    from test_stage1_hc_emulated import getseq_returns

    k, both, hc, file_type, parts = open_table_cases()[name]
    line_cap = capi.SPLIT_LINE_CAP
    sk = capi.SmallK(ctx, k, both)
    try:
        returns, reads, kmers = [], 0, 0
        for i, text in enumerate(parts):
            r, n = sk.part(text, file_type=file_type, flags=capi.SPLIT_HOMOPOLYMER if hc else 0, slot=i % 2)
            ret, n_reads = getseq_returns(text, file_type, k, line_cap)
            returns += ret
            reads, kmers = reads + r - n_reads, kmers + n
        table, total = SK.smallk_table(returns, k, both, hc)
        assert reads == 0 and kmers == total and total > 0
        ci, cx, cm = 2, 40, 9
        st = sk.tally(ci, cx)
        assert [st[n] for n in capi.SMALLK_STATS] == classify(table, ci, cx)[1]
        for p in legal_prefixes(k):
            check_view(ctx, 0, table, k, ci, cx, cm, p)
        check_view(ctx, 0, table, k, ci, cx, cm, framing=1, data_size=2)
        assert np.array_equal(sk.read(), table), "the table was modified"
        # the class's own view: sized by its tally
        view, st2 = sk.view(ci, cx, cm, legal_prefixes(k)[0])
        want = complete(table, k, ci, cx, cm, legal_prefixes(k)[0])
        recs = np.zeros(want["recs"].size, dtype=np.uint8)
        if recs.size:
            ctx.d2h(recs, view.d_recs)
        assert st2 == st and view.n_recs == want["stats"][3] and np.array_equal(recs, want["recs"])
        # another kmer_len than the open table's
        rc, _ = run_tally(ctx, 0, k + 1 if k < 13 else k - 1, ci, cx)
        assert rc == EINVAL and "kmc_hip_smallk_tally" in ctx.last_error()
    finally:
        sk.close()


def check_golden(ctx, name, tmp_path):
    """`count-small` on a recorded input: the bytes `kmc` wrote, its report lines, and the prefix length of its header from smallk_lut_prefix_len"""
    from kmc_amd import tools

    flags, _, fmt = CASES[name]
    out = str(tmp_path / "out")
    res = tools.count_small([*flags, "-t4", "-m2", "-p5", "-n64", input_argument(name, tmp_path), out, str(tmp_path)], ctx=ctx, part_bytes=2048, output_format=fmt)
    with open(golden_report(name)) as f:
        want_lines = report_lines(f.read())
    assert report_lines(tools.count_report(res)) == want_lines, (tools.count_report(res), want_lines)
    assert res["n_parts"] >= (2 if name != "k9_empty" else 1)
    if fmt == "kff":
        with open(out + ".kff", "rb") as f, open(golden_out(name) + ".kff", "rb") as g:
            assert f.read() == g.read(), name
        return res
    got, want = CC.database_bytes(out), CC.database_bytes(golden_out(name))
    h = header_of(want[0])
    o = tools.parse_count_small([*flags, "in", "out"])
    assert tools.smallk_lut_prefix_len(h["k"], dict(want_lines)["No. of unique k-mers"], h["counter_size"]) == h["p"], h
    assert h["counter_size"] == counter_size(o["cx"], o["cs"]) and h["k"] == o["k"]
    assert got[0] == want[0], (name, "kmc_pre", header_of(got[0]), h)
    assert got[1] == want[1], (name, "kmc_suf")
    return res


def check_going_on(ctx, tmp_path):
    """count_small(keep=True) at k = 9: the view through the dump and histogram entries, and as the second operand of an intersect with a database read by dbio"""
    import smallk_cases as SK
    from kmc_amd import dbio, tools

    k, ci, cx, cm = 9, 1, 10**9, 255
    reads = CC.golden_reads(209, 9)
    inp = tmp_path / "in.fq"
    inp.write_bytes(CC.fastq_text(reads))
    res, sk, view = tools.count_small(["-k9", "-ci1", str(inp), str(tmp_path / "db")], ctx=ctx, part_bytes=4096, keep=True)
    other = None
    allocs = []
    try:
        table, total = SK.smallk_table([SK.codes_of(r) for r in reads], k, True)
        assert res["totals"]["n_kmers"] == total
        p = view.lut_prefix_len
        assert p == tools.smallk_lut_prefix_len(k, res["stats"]["n_unique"], 1) and k - p >= 4
        want = complete(table, k, ci, cx, cm, p)
        kmers = np.flatnonzero(table).astype(np.uint64)
        counts = np.minimum(table[table != 0], _U(cm)).astype(np.int64)
        assert view.n_recs == kmers.size == want["stats"][3]
        # dump
        cap = kmers.size * (k + 12)
        d_text = ctx.malloc(cap + 16)
        allocs.append(d_text)
        n_bytes, st = ctx.db_dump_device(k, view, 1, 0, view.n_recs, 1, 10**9, 255, d_text, cap)
        text = np.zeros(n_bytes, dtype=np.uint8)
        ctx.d2h(text, d_text)
        sym = np.frombuffer(b"ACGT", dtype=np.uint8)
        lines = [sym[(int(x) >> (2 * np.arange(k - 1, -1, -1))) & 3].tobytes() + b"\t%d\n" % c for x, c in zip(kmers, counts)]
        assert text.tobytes() == b"".join(lines) and st["n_written"] == kmers.size
        # histogram
        hist = CC.view_histogram(ctx, k, view, 255)
        assert np.array_equal(hist, np.bincount(counts, minlength=256).astype(np.uint64))
        # intersect: a database written and read by dbio is A, the small-k view is B
        rng = np.random.default_rng(9)
        a_k = np.unique(np.concatenate([kmers[rng.random(kmers.size) < 0.4], rng.integers(0, 1 << 18, size=300, dtype=np.uint64)]))
        a_c = rng.integers(1, 200, size=a_k.size)
        lut, recs = S.encode_body(k, 5, 1, [int(x) for x in a_k], [int(c) for c in a_c])
        dbio.write_kmc1(str(tmp_path / "a"), k, 1, 5, 1, 10**9, True, lut, recs)
        other = tools._DeviceDb(ctx, dbio.read_database(str(tmp_path / "a")))
        both_in = np.isin(a_k, kmers)
        w_k = a_k[both_in]
        w_c = np.minimum(a_c[both_in], counts[np.searchsorted(kmers, w_k)])
        d_out, d_lut = ctx.malloc(w_k.size * 2 + 256), ctx.malloc(8 << 10)
        allocs += [d_out, d_lut]
        op = capi.DbOp(capi.DB_OPS["intersect"], capi.DB_COUNTER_OPS["min"], 1, 255, 10**9, 5)
        n, st = ctx.db_set_op_device(k, other.view(1, 10**9), view, op, d_out, min(a_k.size, kmers.size) * 2, d_lut)
        g_recs, g_lut = np.zeros(n * 2, dtype=np.uint8), np.zeros(1 << 10, dtype=np.uint64)
        ctx.d2h(g_recs, d_out)
        ctx.d2h(g_lut, d_lut)
        w_lut, w_recs = S.encode_body(k, 5, 1, [int(x) for x in w_k], [int(c) for c in w_c])
        assert n == w_k.size > 0 and np.array_equal(g_recs, w_recs) and np.array_equal(g_lut, w_lut)
    finally:
        for d in allocs:
            ctx.free(d)
        if other is not None:
            other.free()
        sk.close()


def check_refusals(ctx):
    """every KMC_HIP_EINVAL and KMC_HIP_ECAPACITY of the two entries, each naming the entry; a capacity failure writes nothing"""
    k, (ci, cx, cm) = 5, PARAMS[1]
    table = planted(k, "half", ci, cx, cm)
    want = complete(table, k, ci, cx, cm, 1)
    n_out = want["recs"].size
    dev = Planted(ctx, table)
    u64p = C.POINTER(C.c_uint64)
    try:
        def view(d_table=dev.d, k=k, ci=ci, cx=cx, cm=cm, framing=0, p=1, ds=1, n_out=n_out):
            return run_view(ctx, d_table, k, ci, cx, cm, p, framing, ds, n_out, 4 if framing == 0 else 0)

        assert view()["rc"] == 0
        bad = [dict(k=0), dict(k=14), dict(d_table=0), dict(ci=0), dict(cx=ci - 1), dict(cm=1), dict(cx=1 << 33, cm=1 << 33), dict(p=0), dict(p=6), dict(p=2), dict(p=3),
               dict(framing=1, ds=0), dict(framing=1, ds=5), dict(framing=2)]
        for kw in bad:
            got = view(**kw)
            assert got["rc"] == EINVAL and "kmc_hip_smallk_view_device" in ctx.last_error(), (kw, got["rc"], ctx.last_error())
            assert (got["recs"] == POISON).all() and (got["lut"] == POISON).all(), kw
        for kw in (dict(k=0), dict(k=14), dict(d_table=0), dict(ci=0), dict(cx=ci - 1)):
            a = dict(d_table=dev.d, k=k, ci=ci, cx=cx)
            a.update(kw)
            rc, _ = run_tally(ctx, a["d_table"], a["k"], a["ci"], a["cx"])
            assert rc == EINVAL and "kmc_hip_smallk_tally" in ctx.last_error(), (kw, rc, ctx.last_error())
        # NULL outputs
        L, v, n, st = ctx.L, capi.DbView(), C.c_uint64(0), (C.c_uint64 * 4)()
        d_out, d_lut = ctx.malloc(n_out + 16), ctx.malloc(64)
        try:
            args = lambda out, lut, view, nk, stats: (ctx.h, 0, dev.d, k, 1, ci, cx, cm, 0, 1, 0, out, n_out, lut, view, nk, stats)  # noqa: E731
            for a in (args(None, d_lut, C.byref(v), C.byref(n), st), args(d_out, None, C.byref(v), C.byref(n), st), args(d_out, d_lut, None, C.byref(n), st),
                      args(d_out, d_lut, C.byref(v), None, st), args(d_out, d_lut, C.byref(v), C.byref(n), None)):
                assert L.kmc_hip_smallk_view_device(*a) == EINVAL and "kmc_hip_smallk_view_device" in ctx.last_error()
            assert L.kmc_hip_smallk_tally(ctx.h, 0, dev.d, k, ci, cx, None) == EINVAL and "kmc_hip_smallk_tally" in ctx.last_error()
            # KFF takes no LUT and no view
            kff = complete(table, k, ci, cx, cm, framing=1, data_size=1)
            d_kff = ctx.malloc(kff["recs"].size + 16)
            try:
                assert L.kmc_hip_smallk_view_device(ctx.h, 0, dev.d, k, 1, ci, cx, cm, 1, 0, 1, d_kff, kff["recs"].size, None, None, C.byref(n), st) == 0, ctx.last_error()
                assert n.value == kff["stats"][3]
            finally:
                ctx.free(d_kff)
        finally:
            ctx.free(d_out)
            ctx.free(d_lut)
        # capacity: one byte short, in both framings; the poisoned buffers stay poisoned
        for kw in (dict(n_out=n_out - 1), dict(framing=1, ds=2, n_out=want["stats"][3] * 4 - 1)):
            got = view(**kw)
            assert got["rc"] == ECAPACITY and "kmc_hip_smallk_view_device" in ctx.last_error(), (kw, got["rc"])
            assert (got["recs"] == POISON).all() and (got["lut"] == POISON).all(), kw
        assert [ctx.L.kmc_hip_split_covers(w) for w in (0x108, 0x109, 0x10a)] == [0, 1, 0]
    finally:
        dev.free()


def check_parser():
    """the verb's own refusals and what it shares with `count`"""
    import pytest

    from kmc_amd import tools

    o = tools.parse_count_small(["-k9", "-ci3", "-cx100", "-cs50", "-b", "-hc", "-fm", "-t8", "-m4", "-p7", "-n300", "-sf2", "-sp3", "-sr4", "-r", "-v", "in", "out", "tmp"])
    assert (o["k"], o["ci"], o["cx"], o["cs"], o["both"], o["hc"], o["file_type"], o["inputs"], o["out"]) == (9, 3, 100, 50, False, True, 2, ["in"], "out")
    for bad, word in (("-k14", "count"), ("-k0", "1..13"), (None, "count"), ("-cs1", "-cs1"), ("-okff", "-okff"), ("-x", "-x"), ("-e", "-e"), ("-fbam", "-fbam"), ("-w", "-w")):
        with pytest.raises(tools.UsageError) as e:
            tools.parse_count_small(([bad] if bad else []) + (["-k9"] if bad and not bad.startswith("-k") else []) + ["in", "out"])
        assert word in str(e.value), (bad, str(e.value))
    with pytest.raises(tools.UsageError) as e:
        tools.parse_count_small(["-k9", "-cx5000000000", "-cs5000000000", "in", "out"])
    assert "four counter bytes" in str(e.value)
    with pytest.raises(tools.UsageError):
        tools.parse_count_small(["-k9", "in"])
    with pytest.raises(tools.UsageError) as e:  # `count` still refuses small k, and says where to go
        tools.parse_count(["-k13", "in", "out"])
    assert "-k13" in str(e.value) and "kmc_hip_smallk_" in str(e.value) and "count-small" in str(e.value)
    # the prefix length: p = k for k <= 4, a suffix of at least one byte for k >= 5, whatever the table holds
    for k in range(1, 14):
        for cs in (1, 2, 3, 4):
            for n in (0, 1, (1 << (2 * k)) // 3, 1 << (2 * k)):
                p = tools.smallk_lut_prefix_len(k, n, cs)
                assert (p == k) if k <= 4 else (1 <= p < k and (k - p) % 4 == 0), (k, cs, n, p)
