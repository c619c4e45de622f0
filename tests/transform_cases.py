"""One k-mer database transformed (`kmc_tools transform`): the three operations restated on Python ints — no code shared with the kernels —, the command lines of the
goldens under tests/golden/transform_*, the planted databases, and the helpers that run kmc_hip_db_reduce_device, kmc_hip_db_histogram_device and kmc_hip_db_dump_device
on database bodies. TEST INFRASTRUCTURE shared by tests/make_transform_golden.py, tests/test_db_transform_emulated.py and tests/test_gpu_db_transform.py."""
from __future__ import annotations

import bisect
import gzip
import os

import numpy as np

import setops_cases as S

GOLDEN = S.GOLDEN
U32 = S.U32
DB_OPS = ("sort", "reduce", "compact", "set_counts")
REDUCE_TILE = 256  # records of a k_tr_compact tile (TR_THREADS x TR_REDUCE_IPT)
IMAGE_BYTES = 32 * 1024  # text of a dump tile by default (TR_IMAGE_BYTES)
HIST_LDS_BINS = 10240  # TR_HIST_LDS_BINS: the widest range k_tr_hist keeps in LDS


def default_dump_tile(k):
    return max(1, IMAGE_BYTES // (k + 12))


# ---- the command lines of the goldens: (name, fixture, options of the input, [(operation tokens, options of the output)])
LINES = [
    ("k27_reduce", "setops_k27_a", [], [(["reduce"], ["-ci3", "-cx20", "-cs10"])]),
    ("k27_compact", "setops_k27_a", [], [(["compact"], [])]),
    ("k27_set7", "setops_k27_a", [], [(["set_counts", "7"], [])]),
    ("k27_set300", "setops_k27_a", [], [(["set_counts", "300"], [])]),
    ("k27_set0", "setops_k27_a", [], [(["set_counts", "0"], [])]),
    ("k27_hist", "setops_k27_a", [], [(["histogram"], [])]),
    ("k27_hist_ci2_cx12", "setops_k27_a", [], [(["histogram"], ["-ci2", "-cx12"])]),
    ("k27_dump", "setops_k27_a", [], [(["dump"], [])]),
    ("k27_dump_cut", "setops_k27_a", [], [(["dump"], ["-ci2", "-cx20", "-cs10"])]),
    # patterned on the reference's own example (kmc_tools/config.h:378)
    ("k27_multi", "setops_k27_a", ["-ci2", "-cx15"], [(["reduce"], ["-cx10"]), (["histogram"], []), (["dump"], []), (["dump", "-s"], ["-ci4"])]),
    ("k33raw_dump", "setops_k33_raw_a", [], [(["dump"], [])]),
    ("k33raw_dump_s", "setops_k33_raw_a", [], [(["dump", "-s"], [])]),
    ("k33raw_sort", "setops_k33_raw_a", [], [(["sort"], [])]),
    ("k33raw_hist", "setops_k33_raw_a", [], [(["histogram"], [])]),
    ("k33raw_reduce_dump", "setops_k33_raw_a", [], [(["reduce"], ["-ci2"]), (["dump"], [])]),
    ("k33_sort_hist", "setops_k33_a", [], [(["sort"], []), (["histogram"], [])]),
    ("k55_dump", "setops_k55_a", [], [(["dump"], [])]),
    ("k55_reduce", "setops_k55_a", [], [(["reduce"], ["-cx9"])]),
]
LINE_IDS = [ln[0] for ln in LINES]
# not among the goldens: against a live kmc_tools only
LIVE_LINES = [
    ("live_k55_dump_s", "setops_k55_a", [], [(["dump", "-s"], ["-ci2"])]),
    ("live_k33raw_reduce_hist", "setops_k33_raw_a", [], [(["reduce"], ["-ci2", "-cx20", "-cs15"]), (["histogram"], ["-cx40"])]),
    ("live_k27b_set_compact", "setops_k27_b", [], [(["set_counts", "70000"], []), (["compact"], [])]),
]


def is_text(op_tokens):
    return op_tokens[0] in ("histogram", "dump")


def fixture_path(fixture):
    return os.path.join(GOLDEN, fixture)


def out_name(line, i):
    return f"transform_{line[0]}_{i}"


def golden_out(line, i):
    return os.path.join(GOLDEN, out_name(line, i))


def command_line(line, in_path, out_paths):
    _, _, in_opts, outs = line
    argv = ["transform", in_path, *in_opts]
    for (op, opts), path in zip(outs, out_paths):
        argv += [*op, path, *opts]
    return argv


def read_golden_text(line, i) -> bytes:
    with gzip.open(golden_out(line, i) + ".txt.gz", "rb") as f:
        return f.read()


def write_golden_text(line, i, data: bytes):
    with open(golden_out(line, i) + ".txt.gz", "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(data)


# ---- database bodies <-> lists of (k-mer as int, count), in the body's own order
def decode_segmented(k, p, cs, lut, recs):
    """A body under a LUT of n_seg x 4^p global offsets and a closing entry (a KMC2 file): record j's prefix is the index of the last entry <= j, modulo 4^p
    (kmc_tools/kmc2_db_reader.h:1776-1791). With one segment this is S.decode_body."""
    sb = (k - p) // 4
    rb = sb + cs
    r = np.asarray(recs, dtype=np.uint8).reshape(-1, rb)
    lut = [int(x) for x in lut]
    mask = (1 << (2 * p)) - 1
    kmers, counts = [], []
    for j in range(r.shape[0]):
        prefix = (bisect.bisect_right(lut, j) - 1) & mask
        kmers.append((prefix << (2 * (k - p))) | int.from_bytes(bytes(r[j, :sb]), "big"))
        counts.append(int.from_bytes(bytes(r[j, sb:]), "little"))
    return kmers, counts


def encode_segmented(k, p, cs, segments):
    """segments: list of (kmers ascending, counts) -> (lut uint64[n_seg * 4^p + 1], recs): the body and the LUT of a KMC2 file whose bins are the segments"""
    n_pref = 1 << (2 * p)
    lut, parts, base = [], [], 0
    for kmers, counts in segments:
        seg_lut, recs = S.encode_body(k, p, cs, kmers, counts)
        lut += [base + int(x) for x in seg_lut]
        parts.append(recs)
        base += len(kmers)
    assert len(lut) == n_pref * len(segments)
    return np.array(lut + [base], dtype=np.uint64), (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8))


def file_order(db):
    """(kmers, counts) of a database read by dbio in the order `kmc_tools transform dump` without -s walks it"""
    if db.kmc2:
        return decode_segmented(db.kmer_len, db.lut_prefix_len, db.counter_size, db.raw_lut, db.raw_recs)
    return S.decode_body(db.kmer_len, db.lut_prefix_len, db.counter_size, db.lut, db.recs)


# ---- the semantics (kmc_tools.cpp:41-137, kmc1_db_writer.h:375-404, dump_writer.h:111-160, histogram_writer.h:32-48)
def kmer_text(k, x):
    return "".join("ACGT"[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))


def restate_reduce(kmers, counts, in_cut, ci, cx, cs, value=0):
    st = dict(n_cut_in=0, n_below_min=0, n_above_max=0, n_written=0)
    ok, oc = [], []
    for x, c in zip(kmers, counts):
        if not in_cut[0] <= c <= in_cut[1]:
            st["n_cut_in"] += 1
        elif value:
            ok.append(x)
            oc.append(value)
        elif c < ci:
            st["n_below_min"] += 1
        elif c > cx:
            st["n_above_max"] += 1
        else:
            ok.append(x)
            oc.append(min(c, cs))
    st["n_written"] = len(ok)
    return ok, oc, st


def restate_histogram(counts, in_cut, ci, cx):
    st = dict(n_cut_in=0, n_outside=0, n_counted=0)
    hist = [0] * (cx - ci + 1)
    for c in counts:
        if not in_cut[0] <= c <= in_cut[1]:
            st["n_cut_in"] += 1
        elif not ci <= c <= cx:
            st["n_outside"] += 1
        else:
            hist[c - ci] += 1
            st["n_counted"] += 1
    return hist, st


def histogram_text(hist, ci) -> bytes:
    return "".join(f"{ci + i}\t{c}\n" for i, c in enumerate(hist)).encode()


def restate_dump(k, kmers, counts, in_cut, ci, cx, cs):
    ok, oc, st = restate_reduce(kmers, counts, in_cut, ci, cx, cs)
    return "".join(f"{kmer_text(k, x)}\t{c}\n" for x, c in zip(ok, oc)).encode(), st


def resolve_line(line, hdr):
    """The defaults of parameters_parser.cpp:437-450,842-892 for one line. hdr: S.header_of(input) + kmc2 -> (in_cut, need_order, [dict(op, ci, cx, cs, value, sorted)] of
    the outputs that are written: every sort of an ordered input is left out, kmc_tools.cpp:421-433)"""
    _, _, in_opts, outs = line
    in_cut = (S._opt(in_opts, "-ci") or hdr["min_count"], S._opt(in_opts, "-cx") or hdr["max_count"])
    full = (1 << (8 * hdr["counter_size"])) - 1
    res = []
    for i, (op, opts) in enumerate(outs):
        if op[0] == "sort" and not hdr["kmc2"]:
            continue
        r = dict(index=i, op=op[0], sorted="-s" in op, value=int(op[1]) if op[0] == "set_counts" else 0)
        if op[0] == "set_counts":
            r.update(ci=1, cx=U32, cs=U32)
        else:
            r["ci"] = S._opt(opts, "-ci") or in_cut[0]
            r["cx"] = S._opt(opts, "-cx") or (min(hdr["max_count"], 10000, full) if op[0] == "histogram" else in_cut[1])
            r["cs"] = 1 if op[0] == "compact" else (S._opt(opts, "-cs") or full)
        res.append(r)
    need_order = any(r["op"] in DB_OPS or r["sorted"] for r in res)
    return in_cut, need_order, res


def restate_line(line, db):
    """-> [(index of the output, 'text', bytes, tallies) | (index, 'db', dict(kmers, counts, cs_bytes, p, ci, cx), tallies)]"""
    k = db.kmer_len
    hdr = dict(S.header_of(db), kmc2=db.kmc2)
    in_cut, need_order, res = resolve_line(line, hdr)
    kmers, counts = file_order(db)
    if need_order:
        order = sorted(range(len(kmers)), key=kmers.__getitem__)
        kmers, counts = [kmers[i] for i in order], [counts[i] for i in order]
    out = []
    for r in res:
        if r["op"] == "histogram":
            hist, st = restate_histogram(counts, in_cut, r["ci"], r["cx"])
            out.append((r["index"], "text", histogram_text(hist, r["ci"]), st))
        elif r["op"] == "dump":
            text, st = restate_dump(k, kmers, counts, in_cut, r["ci"], r["cx"], r["cs"])
            out.append((r["index"], "text", text, st))
        else:
            ok, oc, st = restate_reduce(kmers, counts, in_cut, r["ci"], r["cx"], r["cs"], r["value"])
            cs_bytes = S.byte_log(r["value"]) if r["value"] else min(S.byte_log(r["cs"]), S.byte_log(r["cx"]))
            out.append((r["index"], "db", dict(kmers=ok, counts=oc, cs_bytes=cs_bytes, p=S.best_p(k, db.total_kmers), ci=r["ci"], cx=r["cx"]), st))
    return out


def database_files(k, want, both_strands, mode, tmp_path):
    """the two files of a restated database output, as bytes (through dbio.write_kmc1: the header layout is covered by the set-operation goldens)"""
    from kmc_amd import dbio

    lut, recs = S.encode_body(k, want["p"], want["cs_bytes"], want["kmers"], want["counts"])
    dbio.write_kmc1(tmp_path, k, want["cs_bytes"], want["p"], want["ci"], want["cx"], both_strands, lut, recs, mode=mode)
    return tuple(open(tmp_path + ext, "rb").read() for ext in (".kmc_pre", ".kmc_suf"))


def golden_database_files(line, i):
    return tuple(open(golden_out(line, i) + ext, "rb").read() for ext in (".kmc_pre", ".kmc_suf"))


# ---- the device calls on bodies
class DeviceBody:
    """a body (p, counter bytes, lut, recs, segments of the LUT) uploaded once; view(in_cut) -> capi.DbView"""

    def __init__(self, ctx, k, p, cb, lut, recs, n_seg=1):
        self.ctx, self.k, self.p, self.cb, self.n_seg = ctx, k, p, cb, n_seg
        self.n = np.asarray(recs).size // ((k - p) // 4 + cb)
        self.allocs = []
        self.d_recs, self.d_lut = self.up(np.asarray(recs, dtype=np.uint8)), self.up(np.asarray(lut, dtype=np.uint64))

    def up(self, arr):
        d = self.ctx.malloc(arr.nbytes + 256)
        self.allocs.append(d)
        if arr.nbytes:
            self.ctx.h2d(d, np.ascontiguousarray(arr))
        return d

    def view(self, in_cut=(1, U32)):
        from kmc_amd import capi

        return capi.DbView(self.d_recs, self.n, self.d_lut, self.p, self.cb, in_cut[0], in_cut[1])

    def free(self):
        for d in self.allocs:
            self.ctx.free(d)
        self.allocs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def run_reduce(ctx, body, in_cut, ci, cx, cs, value, p_out, capacity=None):
    """-> (lut, recs, tallies) of kmc_hip_db_reduce_device"""
    cs_bytes = S.byte_log(value) if value else min(S.byte_log(cs), S.byte_log(cx))
    rb = (body.k - p_out) // 4 + cs_bytes
    cap = body.n * rb if capacity is None else capacity
    d_out, d_lut = ctx.malloc(cap + 256), ctx.malloc(8 << (2 * p_out))
    try:
        n, st = ctx.db_reduce_device(body.k, body.view(in_cut), ci, cx, cs, value, p_out, d_out, cap, d_lut)
        recs, lut = np.zeros(n * rb, dtype=np.uint8), np.zeros(1 << (2 * p_out), dtype=np.uint64)
        if n:
            ctx.d2h(recs, d_out)
        ctx.d2h(lut, d_lut)
        assert n == st["n_written"]
        return lut, recs, st
    finally:
        ctx.free(d_out)
        ctx.free(d_lut)


def run_histogram(ctx, body, in_cut, ci, cx):
    """-> (hist as a list, tallies) of kmc_hip_db_histogram_device"""
    n_bins = cx - ci + 1
    d_hist = ctx.malloc(8 * n_bins + 256)
    try:
        st = ctx.db_histogram_device(body.k, body.view(in_cut), body.n_seg, ci, cx, d_hist)
        hist = np.zeros(n_bins, dtype=np.uint64)
        ctx.d2h(hist, d_hist)
        return hist, st
    finally:
        ctx.free(d_hist)


GUARD = 0xA7


def run_dump(ctx, body, in_cut, ci, cx, cs, first=0, count=None, capacity=None, base_offset=0):
    """-> (text bytes, tallies) of kmc_hip_db_dump_device over records [first, first + count). The text buffer is filled with a guard pattern first: every byte behind
    *n_bytes — and the `base_offset` bytes in front of d_text, which then does not start at an aligned address — must come back intact."""
    count = body.n - first if count is None else count
    cap = count * (body.k + 12) if capacity is None else capacity
    buf = np.full(base_offset + cap + 64, GUARD, dtype=np.uint8)
    d = ctx.malloc(buf.size + 256)
    try:
        ctx.h2d(d, buf)
        n_bytes, st = ctx.db_dump_device(body.k, body.view(in_cut), body.n_seg, first, count, ci, cx, cs, d + base_offset, cap)
        ctx.d2h(buf, d)
        assert n_bytes <= cap
        assert np.all(buf[:base_offset] == GUARD) and np.all(buf[base_offset + n_bytes:] == GUARD), "bytes outside [0, n_bytes) were written"
        return buf[base_offset:base_offset + n_bytes].tobytes(), st
    finally:
        ctx.free(d)


def check_reduce(ctx, body, kmers, counts, in_cut, ci, cx, cs, value, p_out):
    wk, wc, wst = restate_reduce(kmers, counts, in_cut, ci, cx, cs, value)
    cs_bytes = S.byte_log(value) if value else min(S.byte_log(cs), S.byte_log(cx))
    want_lut, want_recs = S.encode_body(body.k, p_out, cs_bytes, wk, wc)
    lut, recs, st = run_reduce(ctx, body, in_cut, ci, cx, cs, value, p_out)
    assert st == wst, (st, wst)
    assert np.array_equal(recs, want_recs), "records differ"
    assert np.array_equal(lut, want_lut), "LUT differs"
    return st


def check_dump(ctx, body, kmers, counts, in_cut, ci, cx, cs, **kw):
    want, wst = restate_dump(body.k, kmers, counts, in_cut, ci, cx, cs)
    got, st = run_dump(ctx, body, in_cut, ci, cx, cs, **kw)
    assert st == wst, (st, wst)
    assert got == want, "text differs"
    return st


def check_histogram(ctx, body, counts, in_cut, ci, cx):
    want, wst = restate_histogram(counts, in_cut, ci, cx)
    got, st = run_histogram(ctx, body, in_cut, ci, cx)
    assert st == wst, (st, wst)
    assert [int(x) for x in got] == want, "histogram differs"
    return st


# ---- planted databases
KS = [(27, 3, 7), (32, 4, 8), (33, 5, 9), (33, 9, 5), (64, 4, 8), (65, 5, 9), (127, 3, 7), (129, 5, 9), (224, 4, 8)]  # (k, p of the input, p of the output); 33: p 5 lies across a 64-bit word boundary, p 9 inside a word
K_IDS = [f"{k}-p{p}" for k, p, _ in KS]
DIGIT_EDGES = [1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000, 999999999, 1000000000, U32]


def planted_cases(k, p, tile, seed=7):
    """-> list of (name, dict(cb, kmers, counts, in_cut, ci, cx, cs, value)): ordered databases of 3 1/3 tiles (`tile`: the larger of the reduce and the dump tile), run
    through reduce, dump and histogram alike. Counts are given as the body holds them (below 2^(8 cb))."""
    rng = np.random.default_rng(seed + k)
    n = 3 * tile + tile // 3 + 7
    kmers = S.random_kmers(rng, k, n)
    base = dict(cb=1, kmers=kmers, in_cut=(1, U32), ci=1, cx=U32, cs=U32, value=0)
    cases = []
    # decimal-length edges in every counter width that holds them
    for cb in (1, 2, 3, 4):
        edges = [e for e in DIGIT_EDGES if e < (1 << (8 * cb))]
        cases.append((f"digits_cb{cb}", dict(base, cb=cb, counts=[edges[i % len(edges)] for i in range(n)])))
    mid = [int(x) for x in rng.integers(10, 100, size=n)]
    seam = lambda f: [(2 if i & 2 else 240) if f(i) else mid[i] for i in range(n)]  # noqa: E731  2: below, 240: above
    whole = lambda i: (i // tile) == 1  # noqa: E731  the second tile writes nothing, between two that write
    for pname, f in (("all", lambda i: True), ("none", lambda i: False), ("even", lambda i: i % 2 == 0), ("odd", lambda i: i % 2 == 1), ("tile", whole)):
        cases.append((f"cut_in_{pname}", dict(base, counts=seam(f), in_cut=(10, 99))))
        cases.append((f"cut_out_{pname}", dict(base, counts=seam(f), ci=10, cx=99)))
    # both at once, and a clamp that changes the digit count (two digits -> one, three -> two)
    cases.append(("cut_both_and_clamp", dict(base, counts=[int(x) for x in rng.integers(1, 256, size=n)], in_cut=(3, 250), ci=12, cx=180, cs=9)))
    cases.append(("clamp_3_to_2_digits", dict(base, cb=2, counts=[int(x) for x in rng.integers(1, 1000, size=n)], cs=50)))
    cases.append(("set_counts", dict(base, counts=mid, in_cut=(20, 80), value=70000)))
    cases.append(("empty", dict(base, kmers=[], counts=[])))
    cases.append(("one_record", dict(base, kmers=kmers[5:6], counts=[42])))
    for name, pref in (("first_prefix", 0), ("last_prefix", (1 << (2 * p)) - 1), ("one_prefix", (1 << (2 * p)) // 3)):
        cases.append((name, dict(base, kmers=S.random_kmers(rng, k, n, lo_prefix=pref, p=p), counts=mid)))
    return cases


def histogram_window(c):
    """the histogram range a planted case is counted over: the output's cutoffs where they are a window already, otherwise the 400 counters below the largest one"""
    hi = max(c["counts"], default=1)
    lo = max(c["ci"], hi - 300) if hi > 1000 else c["ci"]
    return lo, min(c["cx"], lo + 400)


TALLIES = ("n_cut_in", "n_below_min", "n_above_max", "n_written")


def segmented_case(k, p, tile, seed=3):
    """A KMC2-shaped body: 9 segments, empty at the front, in the middle and at the end, prefixes that recur across segments -> (segments, flat kmers, flat counts)"""
    rng = np.random.default_rng(seed + k)
    n = 3 * tile + tile // 3 + 7
    n_pref = 1 << (2 * p)
    chosen = [0, 1, n_pref // 3, n_pref // 2, n_pref - 2, n_pref - 1]  # a few prefixes, the first and the last among them, so that every segment meets most of them
    pool = [x for i, pf in enumerate(chosen) for x in S.random_kmers(rng, k, n // 6 + (n % 6 if i == 0 else 0), lo_prefix=pf, p=p)]
    sizes = [0, n // 4, n // 8, 0, 0, n // 3, 1, n - n // 4 - n // 8 - n // 3 - 1, 0]
    order = rng.permutation(n)
    segments, at = [], 0
    for sz in sizes:
        ks = sorted(pool[i] for i in order[at:at + sz])
        at += sz
        segments.append((ks, [int(x) for x in rng.integers(1, 200, size=sz)]))
    assert at == n
    flat_k = [x for ks, _ in segments for x in ks]
    flat_c = [c for _, cs in segments for c in cs]
    prefixes = [set(x >> (2 * (k - p)) for x in ks) for ks, _ in segments if ks]
    assert any(a & b for i, a in enumerate(prefixes) for b in prefixes[i + 1:]), "no prefix recurs across segments"
    return segments, flat_k, flat_c


class TransformContext(S.LibContext):
    """S.LibContext with the three entry points of this mode: the interface of capi.Context on a library given by path"""

    def __init__(self, path):
        super().__init__(path)
        C, capi, L = self.C, self.capi, self.L
        vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
        L.kmc_hip_db_reduce_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, u64p, u64p]
        L.kmc_hip_db_histogram_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.c_uint32, C.c_uint32, C.c_uint64, vp, u64p]
        L.kmc_hip_db_dump_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, vp, C.c_uint64, u64p, u64p]



def _bind_context_methods():
    """the three methods are capi.Context's own (they use only self.L, self.h, self._chk): the binding under test is the one the product ships"""
    from kmc_amd import capi

    for name in ("db_reduce_device", "db_histogram_device", "db_dump_device", "_need"):
        setattr(TransformContext, name, getattr(capi.Context, name))


_bind_context_methods()
