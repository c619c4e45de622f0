"""Set operations between two k-mer databases (`kmc_tools simple`): the semantics restated on Python ints and dicts — no code shared with the kernels —, the
command lines of the goldens under tests/golden/setops_*, the planted databases, and the helper that runs kmc_hip_db_set_op_device on KMC1 bodies.
TEST INFRASTRUCTURE shared by tests/make_setops_golden.py, tests/test_db_setops_emulated.py and tests/test_gpu_db_setops.py."""
from __future__ import annotations

import bisect
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U32 = 0xFFFFFFFF

OPS = ("intersect", "union", "kmers_subtract", "counters_subtract", "reverse_kmers_subtract", "reverse_counters_subtract")
DEFAULT_OC = {"intersect": "min", "union": "sum"}  # kmc_tools/config.h:96-110; every other operation: diff

# (name, options of input a, options of input b, operation, options of the output): the command lines of the goldens
LINES = [(op, [], [], op, []) for op in OPS] + [
    ("union_ocmax", [], [], "union", ["-ocmax"]),
    ("union_ocleft", [], [], "union", ["-ocleft"]),
    ("intersect_ocsum_cs65535", [], [], "intersect", ["-ocsum", "-cs65535"]),
    ("intersect_ocright", [], [], "intersect", ["-ocright"]),
    ("counters_subtract_ocdiff", [], [], "counters_subtract", ["-ocdiff"]),
    ("reverse_counters_subtract_ocdiff", [], [], "reverse_counters_subtract", ["-ocdiff"]),
    ("union_ci3_cx20_cs10", [], [], "union", ["-ci3", "-cx20", "-cs10"]),
    ("union_a_ci2_b_cx5", ["-ci2"], ["-cx5"], "union", []),
]
PAIRS = (27, 55, 33)
# k = 33: inputs of more than 8 160 k-mers, where kmc_tools itself picks lut_prefix_len 5 — the prefix lies across a 64-bit word boundary of the k-mer
LINES_OF = {27: LINES, 55: LINES, 33: [ln for ln in LINES if ln[0] in ("union", "intersect", "counters_subtract")]}
GOLDEN_CASES = [(k, ln) for k in PAIRS for ln in LINES_OF[k]]
GOLDEN_IDS = [f"{ln[0]}-{k}" for k, ln in GOLDEN_CASES]
RAW_A = {33: "raw_a"}  # the KMC2 database `kmc` wrote for input a (records ordered inside every signature bin), kept next to what `transform sort` made of it


def golden_path(k, name):
    return os.path.join(GOLDEN, f"setops_k{k}_{name}")


def _opt(opts, name, default=0):
    for o in opts:
        if o.startswith(name):
            return int(o[len(name):])
    return default


def byte_log(x):
    return 1 if x < 256 else 2 if x < 65536 else 3 if x < (1 << 24) else 4


def best_p(k, n):
    """kmc1_db_writer.h:432-452"""
    return min((n * (k - p) // 4 + (8 << (2 * p)), p) for p in range(1, 16) if (k - p) % 4 == 0)[1]


# ---- KMC1 bodies <-> lists of (k-mer as int, count)
def decode_body(k, p, cs, lut, recs):
    sb = (k - p) // 4
    rb = sb + cs
    r = np.asarray(recs, dtype=np.uint8).reshape(-1, rb)
    lut = [int(x) for x in lut]
    kmers, counts = [], []
    for j in range(r.shape[0]):
        prefix = bisect.bisect_right(lut, j) - 1
        kmers.append((prefix << (2 * (k - p))) | int.from_bytes(bytes(r[j, :sb]), "big"))
        counts.append(int.from_bytes(bytes(r[j, sb:]), "little"))
    return kmers, counts


def encode_body(k, p, cs, kmers, counts):
    sb = (k - p) // 4
    out = bytearray()
    prefixes = []
    for x, c in zip(kmers, counts):
        out += (x & ((1 << (2 * (k - p))) - 1)).to_bytes(sb, "big") + (c & ((1 << (8 * cs)) - 1)).to_bytes(cs, "little")
        prefixes.append(x >> (2 * (k - p)))
    lut = np.searchsorted(np.array(prefixes, dtype=np.uint64), np.arange(1 << (2 * p), dtype=np.uint64), side="left").astype(np.uint64)  # entry i: records with a prefix below i
    return lut, np.frombuffer(bytes(out), dtype=np.uint8).copy()


# ---- the semantics (operations.h:298-491, bundle.h:257-278, kmc1_db_reader.h:574-618, kmc1_db_writer.h:382-385)
def _present(counts_by_kmer, ci, cx):
    rng = (cx - ci) & 0xFFFFFFFFFFFFFFFF
    return {x: c for x, c in counts_by_kmer.items() if ((c - ci) & U32) <= rng}


def _counter(oc, c1, c2):
    return {"min": min(c1, c2), "max": max(c1, c2), "sum": (c1 + c2) & U32, "diff": c1 - c2 if c1 > c2 else 0, "left": c1, "right": c2}[oc]


def restate(a, b, a_cut, b_cut, op, oc, ci, cx, cs):
    """a, b: (kmers, counts); a_cut, b_cut: (cutoff_min, cutoff_max) of the inputs; -> (kmers, counts, tallies dict)"""
    da, db = _present(dict(zip(*a)), *a_cut), _present(dict(zip(*b)), *b_cut)
    st = dict(n_pairs=0, n_only_a=0, n_only_b=0, n_below_min=0, n_above_max=0, n_written=0)
    kmers, counts = [], []
    for x in sorted(set(da) | set(db)):
        if x in da and x in db:
            st["n_pairs"] += 1
            if op in ("kmers_subtract", "reverse_kmers_subtract"):
                continue
            c = _counter(oc, db[x], da[x]) if op == "reverse_counters_subtract" else _counter(oc, da[x], db[x])
        elif x in da:
            st["n_only_a"] += 1
            if op not in ("union", "kmers_subtract", "counters_subtract"):
                continue
            c = da[x]
        else:
            st["n_only_b"] += 1
            if op not in ("union", "reverse_kmers_subtract", "reverse_counters_subtract"):
                continue
            c = db[x]
        if c < ci:
            st["n_below_min"] += 1
        elif c > cx:
            st["n_above_max"] += 1
        else:
            kmers.append(x)
            counts.append(min(c, cs))
            st["n_written"] += 1
    return kmers, counts, st


def resolve_line(line, hdr_a, hdr_b):
    """The defaults of parameters_parser.cpp:842-866 for one golden line. hdr_*: dict(counter_size, min_count, max_count, total_kmers, kmer_len) ->
    dict(a_cut, b_cut, op, oc, ci, cx, cs, cs_bytes, p_out)"""
    _, oa, ob, op, oo = line
    a_cut = (_opt(oa, "-ci") or hdr_a["min_count"], _opt(oa, "-cx") or hdr_a["max_count"])
    b_cut = (_opt(ob, "-ci") or hdr_b["min_count"], _opt(ob, "-cx") or hdr_b["max_count"])
    ci = _opt(oo, "-ci") or min(a_cut[0], b_cut[0])
    cx = _opt(oo, "-cx") or max(a_cut[1], b_cut[1])
    cs = _opt(oo, "-cs") or (1 << (8 * max(hdr_a["counter_size"], hdr_b["counter_size"]))) - 1
    oc = next((o[3:] for o in oo if o.startswith("-oc")), None) or DEFAULT_OC.get(op, "diff")
    k = hdr_a["kmer_len"]
    return dict(a_cut=a_cut, b_cut=b_cut, op=op, oc=oc, ci=ci, cx=cx, cs=cs, cs_bytes=min(byte_log(cs), byte_log(cx)),
                p_out=max(best_p(k, hdr_a["total_kmers"]), best_p(k, hdr_b["total_kmers"])))


def command_line(line, a, b, out):
    _, oa, ob, op, oo = line
    return ["simple", a, *oa, b, *ob, op, out, *oo]


# ---- the device call on bodies
def run_device(ctx, k, a_body, b_body, a_cut, b_cut, op, oc, ci, cx, cs, p_out, capacity=None):
    """a_body, b_body: (p, counter bytes, lut, recs). -> (lut, recs, tallies) of kmc_hip_db_set_op_device"""
    from kmc_amd import capi

    allocs = []

    def up(arr):
        d = ctx.malloc(arr.nbytes + 256)
        allocs.append(d)
        if arr.nbytes:
            ctx.h2d(d, np.ascontiguousarray(arr))
        return d

    try:
        views, ns = [], []
        for (p, cb, lut, recs), cut in ((a_body, a_cut), (b_body, b_cut)):
            n = recs.size // ((k - p) // 4 + cb)
            ns.append(n)
            views.append(capi.DbView(up(recs), n, up(np.asarray(lut, dtype=np.uint64)), p, cb, cut[0], cut[1]))
        cs_bytes = min(byte_log(cs), byte_log(cx))
        rb = (k - p_out) // 4 + cs_bytes
        bound = {"union": ns[0] + ns[1], "intersect": min(ns), "kmers_subtract": ns[0], "counters_subtract": ns[0]}.get(op, ns[1])
        cap = bound * rb if capacity is None else capacity
        d_out, d_lut = ctx.malloc(cap + 256), ctx.malloc(8 << (2 * p_out))
        allocs.extend([d_out, d_lut])
        n, st = ctx.db_set_op_device(k, views[0], views[1], capi.DbOp(capi.DB_OPS[op], capi.DB_COUNTER_OPS[oc], ci, cs, cx, p_out), d_out, cap, d_lut)
        recs, lut = np.zeros(n * rb, dtype=np.uint8), np.zeros(1 << (2 * p_out), dtype=np.uint64)
        if n:
            ctx.d2h(recs, d_out)
        ctx.d2h(lut, d_lut)
        return lut, recs, st
    finally:
        for d in allocs:
            ctx.free(d)


def check_case(ctx, k, a, b, a_fmt, b_fmt, p_out, op, oc, ci=1, cx=U32, cs=U32, a_cut=(1, U32), b_cut=(1, U32)):
    """a, b: (kmers, counts); *_fmt: (p, counter bytes). The device call on the encoded bodies must equal the restatement: records, LUT and tallies."""
    bodies = [(p, cb, *encode_body(k, p, cb, *x)) for x, (p, cb) in ((a, a_fmt), (b, b_fmt))]
    # what the bodies hold is what the operation sees (a counter of cb bytes keeps the low bytes)
    seen = [(x[0], [c & ((1 << (8 * cb)) - 1) for c in x[1]]) for x, (_, cb) in ((a, a_fmt), (b, b_fmt))]
    wk, wc, wst = restate(seen[0], seen[1], a_cut, b_cut, op, oc, ci, cx, cs)
    want_lut, want_recs = encode_body(k, p_out, min(byte_log(cs), byte_log(cx)), wk, wc)
    lut, recs, st = run_device(ctx, k, bodies[0], bodies[1], a_cut, b_cut, op, oc, ci, cx, cs, p_out)
    assert st == wst, (st, wst)
    assert np.array_equal(recs, want_recs), "records differ"
    assert np.array_equal(lut, want_lut), "LUT differs"
    return st


# ---- planted databases
def random_kmers(rng, k, n, lo_prefix=None, p=None):
    """n distinct ascending k-mers; lo_prefix: all of them inside this p-symbol prefix"""
    bits = 2 * k if lo_prefix is None else 2 * (k - p)
    s = set()
    while len(s) < n:
        s.add(int.from_bytes(rng.bytes((bits + 7) // 8), "big") & ((1 << bits) - 1))
    base = 0 if lo_prefix is None else lo_prefix << bits
    return sorted(base | x for x in s)


def straddles(k, p):
    """the p-symbol prefix of a k-mer lies across a 64-bit word boundary: its lowest bit is bit 2 (k - p)"""
    return (2 * (k - p)) % 64 + 2 * p > 64


def default_prefix_lens(k):
    return [p for p in (1, 2, 3, 4, 5, 6, 7) if (k - p) % 4 == 0][0], [p for p in (5, 6, 7, 4) if (k - p) % 4 == 0][0], [p for p in (3, 4, 1, 2) if (k - p) % 4 == 0][0]


REDUCED = ("mixed_", "equal_", "first_prefix", "last_prefix", "one_prefix")  # the reduced list: the names that start like this

# (k, prefix lengths of A, B and the output or None: default_prefix_lens, reduced list): what test_device_call_on_planted_databases runs. SIZE 1 (k = 27, 32, 33: the
# prefix across the word boundary), 2 (35: likewise; 55), 3 (65, 96), 4 (127), 5 (129), 6 (161), 7 (193, 224: the widest). At every straddling k each of the three
# prefixes straddles in some format
PLANTED = [(27, None, False), (32, None, False), (55, None, False), (127, None, False),
           (33, (5, 9, 5), True), (33, (1, 5, 9), True), (35, (7, 3, 7), True), (35, (3, 7, 3), True), (65, (5, 9, 5), True), (96, (4, 8, 4), True),
           (129, (9, 5, 9), True), (161, (5, 9, 5), True), (193, (9, 5, 9), True), (224, (4, 8, 4), True)]
PLANTED_IDS = [str(k) if pl is None else f"{k}-p{pl[0]}.{pl[1]}.{pl[2]}" for k, pl, _ in PLANTED]
for _k in (33, 35, 65, 129, 161, 193):
    assert all(any(straddles(_k, pl[q]) for k, pl, _ in PLANTED if k == _k) for q in range(3)), _k


def planted_cases(k, tile, seed=5, prefix_lens=None, reduced=False):
    """-> list of (name, a, b, kwargs of check_case). `tile`: records of a merge tile of the library under test; the databases are 3-4 tiles long.
    prefix_lens: lut_prefix_len of A, of B and of the output (default: default_prefix_lens(k)); reduced: only the cases named in REDUCED"""
    rng = np.random.default_rng(seed + k)
    n = 3 * tile + tile // 3 + 7
    p_a, p_b, p_o = prefix_lens or default_prefix_lens(k)
    cnt = lambda m, hi=200: [int(x) for x in rng.integers(1, hi, size=m)]  # noqa: E731
    all_k = random_kmers(rng, k, 2 * n)
    same = all_k[1::2][:n]
    fm = dict(a_fmt=(p_a, 1), b_fmt=(p_b, 2), p_out=p_o)
    cases = []
    eq_a, eq_b = (same, cnt(n)), (same, cnt(n))
    for op, oc in (("intersect", "min"), ("union", "sum"), ("counters_subtract", "diff")):
        cases.append((f"equal_{op}", eq_a, eq_b, dict(fm, op=op, oc=oc)))
        cases.append((f"equal_shifted_{op}", ([0] + same, [7] + eq_a[1]), eq_b, dict(fm, op=op, oc=oc)))  # one smallest A-only record in front: the other parity
    lo, hi = all_k[:n], all_k[n:]
    cases.append(("disjoint_a_below_b", (lo, cnt(n)), (hi, cnt(n)), dict(fm, op="union", oc="sum")))
    cases.append(("disjoint_b_below_a", (hi, cnt(n)), (lo, cnt(n)), dict(fm, op="union", oc="max")))
    cases.append(("disjoint_intersect", (hi, cnt(n)), (lo, cnt(n)), dict(fm, op="intersect", oc="min")))
    some = (all_k[:n], cnt(n))
    for op in ("union", "intersect", "kmers_subtract", "reverse_kmers_subtract"):
        cases.append((f"a_empty_{op}", ([], []), some, dict(fm, op=op, oc="sum")))
        cases.append((f"b_empty_{op}", some, ([], []), dict(fm, op=op, oc="sum")))
        cases.append((f"both_empty_{op}", ([], []), ([], []), dict(fm, op=op, oc="sum")))
    one, other = all_k[5], all_k[9]
    for op, oc in (("union", "sum"), ("intersect", "max"), ("reverse_counters_subtract", "diff"), ("kmers_subtract", "diff")):
        cases.append((f"single_equal_{op}", ([one], [3]), ([one], [9]), dict(fm, op=op, oc=oc)))
        cases.append((f"single_differs_{op}", ([one], [3]), ([other], [9]), dict(fm, op=op, oc=oc)))
    # mixed: half shared, through every operation, p and counter bytes differing between the inputs and the output
    mix_a, mix_b = sorted(all_k[0::3] + all_k[1::3])[:n], sorted(all_k[1::3] + all_k[2::3])[:n]
    for op in OPS:
        cases.append((f"mixed_{op}", (mix_a, cnt(len(mix_a))), (mix_b, cnt(len(mix_b))), dict(a_fmt=(p_a, 2), b_fmt=(p_b, 1), p_out=p_o, op=op, oc=DEFAULT_OC.get(op, "diff"), cs=255)))
    cases.append(("mixed_cut_and_clamp", (mix_a, cnt(len(mix_a), 40)), (mix_b, cnt(len(mix_b), 40)),
                  dict(a_fmt=(p_a, 1), b_fmt=(p_b, 1), p_out=p_o, op="union", oc="sum", ci=5, cx=50, cs=30, a_cut=(3, 35), b_cut=(1, 20))))
    # the LUT's edge entries: everything in one prefix / the first / the last prefix (of the widest LUT in play)
    pw = max(p_a, p_b, p_o)
    for name, pref in (("first_prefix", 0), ("last_prefix", (1 << (2 * pw)) - 1), ("one_prefix", (1 << (2 * pw)) // 3)):
        ks = random_kmers(rng, k, n + n // 2, lo_prefix=pref, p=pw)
        cases.append((name, (ks[:n], cnt(n)), (ks[n // 2:], cnt(len(ks) - n // 2)), dict(fm, op="union", oc="sum")))
    # 32-bit counters at the top: sum wraps, diff reaches 0
    top = [U32, U32 - 1, 1, U32, 2, U32][: min(6, n)]
    tk = all_k[: len(top)]
    f4 = dict(a_fmt=(p_a, 4), b_fmt=(p_b, 4), p_out=p_o)
    cases.append(("wrap_sum", (tk, top), (tk, [1, 2, U32, U32, U32 - 1, 5][: len(top)]), dict(f4, op="union", oc="sum")))
    cases.append(("diff_to_zero", (tk, top), (tk, [U32, U32, 1, 5, 2, U32 - 1][: len(top)]), dict(f4, op="counters_subtract", oc="diff")))
    cases.append(("reverse_diff_to_zero", (tk, top), (tk, [U32, U32, 1, 5, 2, U32 - 1][: len(top)]), dict(f4, op="reverse_counters_subtract", oc="diff")))
    return [c for c in cases if c[0].startswith(REDUCED)] if reduced else cases


SEAM_OPS = (("union", "sum"), ("intersect", "min"), ("counters_subtract", "diff"), ("reverse_kmers_subtract", "diff"))
SEAMS = [(27, None), (55, None), (33, (5, 9, 5))]  # (k, prefix lengths): what test_cut_records_on_every_tile_seam runs
SEAM_IDS = ["27", "55", "33-p5.9.5"]


def seam_cut_cases(k, tile, prefix_lens=None, seed=11):
    """Records cut by their INPUT'S cutoffs on every tile seam. A and B hold the same keys, so the merged sequence is A0 B0 A1 B1 ...: in one parity every seam
    falls between two pairs, in the other (one smallest A-only record in front) inside a pair — A's record the last of a tile, its partner B's the first of the
    next, each seen by the other through the halo. Who is cut is chosen by position: all of A, all of B, A at even and B at odd positions, and the converse —
    so on every seam one side or the other is cut, in the slice or in the halo. A count below its input's cutoff_min (2 against 10) or above its cutoff_max
    (240 against 99) is cut. -> list of (name, a, b, kwargs of check_case)"""
    rng = np.random.default_rng(seed + k)
    n = 3 * tile + tile // 3 + 7
    p_a, p_b, p_o = prefix_lens or default_prefix_lens(k)
    same = random_kmers(rng, k, n + 1)[1:]  # none of them 0
    in_cut, kept = (10, 99), (1, 255)

    def counts(m, is_cut):
        c = [int(x) for x in rng.integers(10, 100, size=m)]
        return [(2 if i & 2 else 240) if is_cut(i) else c[i] for i in range(m)]

    patterns = (("all_a_cut", lambda i: True, lambda i: False), ("all_b_cut", lambda i: False, lambda i: True),
                ("a_even_b_odd_cut", lambda i: i % 2 == 0, lambda i: i % 2 == 1), ("a_odd_b_even_cut", lambda i: i % 2 == 1, lambda i: i % 2 == 0))
    cases = []
    for parity, ka in (("pairs", same), ("shifted", [0] + same)):
        for pname, cut_a, cut_b in patterns:
            a, b = (ka, counts(len(ka), cut_a)), (same, counts(n, cut_b))
            for op, oc in SEAM_OPS:
                cases.append((f"{pname}_{parity}_{op}", a, b, dict(a_fmt=(p_a, 1), b_fmt=(p_b, 1), p_out=p_o, op=op, oc=oc, a_cut=in_cut, b_cut=in_cut, ci=kept[0], cx=kept[1], cs=255)))
    return cases


class LibContext:
    """The few entry points run_device needs, bound on a library given by path (the emulated host library of the CPU tests) — the interface of capi.Context"""

    def __init__(self, path):
        import ctypes as C

        from kmc_amd import capi

        self.C, self.capi = C, capi
        L = self.L = C.CDLL(path)
        vp = C.c_void_p
        L.kmc_hip_init.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
        L.kmc_hip_destroy.argtypes = [vp]
        L.kmc_hip_destroy.restype = None
        L.kmc_hip_last_error.argtypes = [vp]
        L.kmc_hip_last_error.restype = C.c_char_p
        L.kmc_hip_malloc.argtypes = [vp, C.c_int, C.c_uint64, C.POINTER(vp)]
        L.kmc_hip_free.argtypes = [vp, C.c_int, vp]
        L.kmc_hip_memcpy_h2d.argtypes = [vp, C.c_int, vp, vp, C.c_uint64]
        L.kmc_hip_memcpy_d2h.argtypes = [vp, C.c_int, vp, vp, C.c_uint64]
        L.kmc_hip_db_set_op_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.POINTER(capi.DbView), C.POINTER(capi.DbOp), vp, C.c_uint64, vp,
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.kmc_hip_counter_size.argtypes = [C.c_uint64, C.c_uint64]
        L.kmc_hip_out_rec_bytes.argtypes = [C.POINTER(capi.BinParams)]
        L.kmc_hip_out_rec_bytes.restype = C.c_uint32
        L.kmc_hip_order_database_device.argtypes = [vp, C.c_int, C.POINTER(capi.BinParams), C.POINTER(capi.BinDesc), C.c_uint64, C.c_uint32, vp, C.c_uint64, vp, C.POINTER(C.c_uint64)]
        h = vp()
        ids = (C.c_int * 1)(0)
        assert L.kmc_hip_init(ids, 1, C.byref(h)) == 0
        self.h = h

    def close(self):
        if self.h:
            self.L.kmc_hip_destroy(self.h)
            self.h = None

    def _chk(self, rc):
        if rc:
            raise self.capi.KmcHipError(rc, self.L.kmc_hip_last_error(self.h).decode())

    def malloc(self, nbytes):
        p = self.C.c_void_p()
        self._chk(self.L.kmc_hip_malloc(self.h, 0, max(nbytes, 1), self.C.byref(p)))
        return p.value

    def free(self, d):
        self._chk(self.L.kmc_hip_free(self.h, 0, d))

    def h2d(self, d, a):
        self._chk(self.L.kmc_hip_memcpy_h2d(self.h, 0, d, a.ctypes.data, a.nbytes))

    def d2h(self, a, d):
        self._chk(self.L.kmc_hip_memcpy_d2h(self.h, 0, a.ctypes.data, d, a.nbytes))

    def out_rec_bytes(self, p):
        return self.L.kmc_hip_out_rec_bytes(self.C.byref(p))

    def order_database_device(self, p, descs, out_lut_prefix_len, d_out, out_capacity, d_lut_out):
        n = self.C.c_uint64()
        self._chk(self.L.kmc_hip_order_database_device(self.h, 0, self.C.byref(p), descs, len(descs), out_lut_prefix_len, d_out, out_capacity, d_lut_out, self.C.byref(n)))
        return n.value

    def db_set_op_device(self, kmer_len, a, b, op, d_out, out_capacity, d_lut_out):
        C = self.C
        n, st = C.c_uint64(), (C.c_uint64 * 6)()
        self._chk(self.L.kmc_hip_db_set_op_device(self.h, 0, kmer_len, C.byref(a), C.byref(b), C.byref(op), d_out, out_capacity, d_lut_out, C.byref(n), st))
        return n.value, dict(zip(self.capi.DB_STATS, (int(x) for x in st)))


def golden_db(k, name):
    from kmc_amd import dbio

    return dbio.read_database(golden_path(k, name))


def header_of(d):
    return dict(counter_size=d.counter_size, min_count=d.min_count, max_count=d.max_count, total_kmers=d.total_kmers, kmer_len=d.kmer_len)
