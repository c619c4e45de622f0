"""A set expression over several k-mer databases (`kmc_tools complex`): the semantics restated NODE BY NODE on sorted lists of (k-mer as int, count), every node a
two-pointer merge of its children as the reference's bundles are (operations.h:85-256) — no code shared with the kernels, and not their pointwise formulation —, the
definitions of the goldens under tests/golden/complex_*, the planted databases, and the helper that runs kmc_hip_db_expr_device on KMC1 bodies.
TEST INFRASTRUCTURE shared by tests/make_complex_golden.py, tests/test_db_complex_emulated.py and tests/test_gpu_db_complex.py."""
from __future__ import annotations

import os

import numpy as np

import setops_cases as S

ROOT = S.ROOT
GOLDEN = S.GOLDEN
U32 = S.U32
TALLIES = ("n_keys", "n_result", "n_below_min", "n_above_max", "n_written")
MAX_LEAVES = 16
OPS = {"+": "union", "*": "intersect", "-": "kmers_subtract", "~": "counters_subtract"}
DEFAULT_MODE = {"union": "sum", "intersect": "min", "kmers_subtract": "diff", "counters_subtract": "diff"}
EXPR_INPUT = 16


# ---- trees. ("in", i) | (operation, counter mode, left, right); the helpers build them without the command line's parser
def IN(i):
    return ("in", i)


def node(op, left, right, mode=None):
    op = OPS.get(op, op)
    return (op, mode or DEFAULT_MODE[op], left, right)


def leaves(tree):
    return [tree[1]] if tree[0] == "in" else leaves(tree[2]) + leaves(tree[3])


def postfix(tree, slot=None):
    """-> [(kind, arg)] of kmc_hip_db_expr_device; slot: input index -> index among the views passed"""
    from kmc_amd import capi

    if tree[0] == "in":
        return [(EXPR_INPUT, tree[1] if slot is None else slot[tree[1]])]
    return postfix(tree[2], slot) + postfix(tree[3], slot) + [(capi.DB_OPS[tree[0]], capi.DB_COUNTER_OPS[tree[1]])]


def bound(tree, n):
    if tree[0] == "in":
        return n[tree[1]]
    lt, rt = bound(tree[2], n), bound(tree[3], n)
    return lt + rt if tree[0] == "union" else min(lt, rt) if tree[0] == "intersect" else lt


# ---- the semantics, node by node
def _leaf(kmers, counts, ci, cx):
    """kmc1_db_reader.h:574-576,618"""
    rng = (cx - ci) & 0xFFFFFFFFFFFFFFFF
    return [(x, c) for x, c in zip(kmers, counts) if ((c - ci) & U32) <= rng]


def _equal(mode, out, x, c1, c2):
    """C2ArgOper::EqualsToOuputBundle (operations.h:40-68)"""
    if mode == "min":
        out.append((x, min(c1, c2)))
    elif mode == "max":
        out.append((x, max(c1, c2)))
    elif mode == "sum":
        out.append((x, (c1 + c2) & U32))
    elif mode == "diff":
        if c1 > c2:
            out.append((x, c1 - c2))
    elif mode == "left":
        out.append((x, c1))
    elif mode == "right":
        out.append((x, c2))
    else:
        raise ValueError(mode)


def _merge(op, mode, a, b):
    out, i, j = [], 0, 0
    while i < len(a) and j < len(b):
        if a[i][0] == b[j][0]:
            if op != "kmers_subtract":
                _equal(mode, out, a[i][0], a[i][1], b[j][1])
            i, j = i + 1, j + 1
        elif a[i][0] < b[j][0]:
            if op != "intersect":
                out.append(a[i])
            i += 1
        else:
            if op == "union":
                out.append(b[j])
            j += 1
    if op != "intersect":
        out += a[i:]
    if op == "union":
        out += b[j:]
    return out


def evaluate(tree, leaf_lists):
    if tree[0] == "in":
        return leaf_lists[tree[1]]
    return _merge(tree[0], tree[1], evaluate(tree[2], leaf_lists), evaluate(tree[3], leaf_lists))


def restate(tree, inputs, cuts, ci, cx, cs):
    """inputs: [(kmers, counts)] ascending; cuts: [(cutoff_min, cutoff_max)] -> (kmers, counts, tallies). The root: kmc1_db_writer.h:382-385"""
    used = sorted(set(leaves(tree)))
    lists = {i: _leaf(*inputs[i], *cuts[i]) for i in used}
    root = evaluate(tree, lists)
    st = dict.fromkeys(TALLIES, 0)
    st["n_keys"] = len(set().union(*[{x for x, _ in lists[i]} for i in used]))
    st["n_result"] = len(root)
    kmers, counts = [], []
    for x, c in root:
        if c < ci:
            st["n_below_min"] += 1
        elif c > cx:
            st["n_above_max"] += 1
        else:
            kmers.append(x)
            counts.append(min(c, cs))
    st["n_written"] = len(kmers)
    return kmers, counts, st


# ---- the goldens: (name, [(variable, fixture, options)], expression, OUTPUT_PARAMS or None). A fixture is a database already under tests/golden
def _defs(k):
    a, b, c, d, w = (f"setops_k{k}_{n}" for n in ("a", "b", "kmers_subtract", "union_ci3_cx20_cs10", "intersect_ocsum_cs65535"))
    abc = [("a", a, []), ("b", b, []), ("c", c, [])]
    abd = [("a", a, []), ("b", b, []), ("c", d, [])]
    full = [
        ("union_of_product", abd, "a + b * c", None),
        ("product_of_union", abd, "(a + b) * c", None),
        ("minus_minus", abd, "a - b - c", None),
        ("minus_parenthesis", abd, "a - (b - c)", None),
        ("union_diff", abd, "(a + b) ~ c", None),
        ("modes", abd, "a ~ min b + max c", None),
        ("left_right", abd, "a * left b * right c", None),
        ("symmetric_difference", abc, "(a - b) + (b - a)", None),
        ("same_input_twice", abc, "a * b + a", None),
        ("one_input", abc, "a", None),
        ("cutoffs", [("a", a, ["-ci2"]), ("b", b, ["-cx9"]), ("c", d, ["-ci4", "-cx15"])], "(a + b + c) ~ c + a", ["-ci3", "-cx40", "-cs10"]),
        ("unused_wide_input", [("a", a, []), ("wide", w, []), ("b", b, [])], "a + b", None),
        # an inner sum beyond 255 (7 a + 4 w, w = a + b in two counter bytes; 16 leaves) that ~ brings back under it (6 a): a chain of `simple` calls with -cs255 would clamp the sum first
        ("inner_sum_beyond_cs", [("a", a, []), ("w", w, [])], "(a + a + a + a + a + a + a + w + w + w + w) ~ (w + w + w + w + a)", ["-cs255"]),
    ]
    return full


def _defs33():
    a, b, raw, u = (f"setops_k33_{n}" for n in ("a", "b", "raw_a", "union"))
    return [
        ("union_of_product", [("a", a, []), ("b", b, []), ("c", u, [])], "a + b * c", None),
        ("union_diff", [("a", a, []), ("b", b, []), ("c", u, [])], "(c ~ a) - a", None),
        ("kmc2_input", [("raw", raw, []), ("b", b, [])], "b ~ raw + raw * max b", None),
        ("one_input", [("a", a, [])], "a", ["-ci2"]),
    ]


DEFS = {27: _defs(27), 55: _defs(55), 33: _defs33()}
GOLDEN_CASES = [(k, ln) for k in (27, 55, 33) for ln in DEFS[k]]
GOLDEN_IDS = [f"{ln[0]}-{k}" for k, ln in GOLDEN_CASES]


# definitions run against a live kmc_tools where oracle/_ref is built (no golden is kept for them)
LIVE = [("live_mixed", [("a", "setops_k27_a", ["-ci2"]), ("b", "setops_k27_b", []), ("u", "setops_k27_union", ["-cx30"])], "(u ~ a) * max b + (a - b) ~ min u", ["-ci2", "-cs20"]),
        ("live_kmc2", [("raw", "setops_k33_raw_a", ["-cx12"]), ("b", "setops_k33_b", []), ("u", "setops_k33_union", [])], "u - (raw * b) + raw ~ b", None)]


def golden_out(k, name):
    return os.path.join(GOLDEN, f"complex_k{k}_{name}")


def fixture_path(fixture):
    return os.path.join(GOLDEN, fixture)


def definition_text(line, out_path, path_of=fixture_path):
    _, inputs, expression, params = line
    text = "INPUT:\n" + "".join(f"{var} = {path_of(fx)} {' '.join(opts)}\n" for var, fx, opts in inputs) + f"OUTPUT:\n{out_path} = {expression}\n"
    return text + ("OUTPUT_PARAMS:\n" + " ".join(params) + "\n" if params else "")


def resolve_line(line, headers):
    """The defaults of parameters_parser.cpp:842-848,893-916 and kmc1_db_writer.h:425-455 for one golden definition, over every defined input.
    headers: per input dict(counter_size, min_count, max_count, total_kmers, kmer_len) -> dict(cuts, ci, cx, cs, cs_bytes, p_out)"""
    _, inputs, _, params = line
    params = params or []
    cuts = [(S._opt(opts, "-ci") or h["min_count"], S._opt(opts, "-cx") or h["max_count"]) for (_, _, opts), h in zip(inputs, headers)]
    ci = S._opt(params, "-ci") or min(c[0] for c in cuts)
    cx = S._opt(params, "-cx") or max(c[1] for c in cuts)
    cs = S._opt(params, "-cs") or (1 << (8 * max(h["counter_size"] for h in headers))) - 1
    k = headers[0]["kmer_len"]
    return dict(cuts=cuts, ci=ci, cx=cx, cs=cs, cs_bytes=min(S.byte_log(cs), S.byte_log(cx)), p_out=max(S.best_p(k, h["total_kmers"]) for h in headers))


def tree_of(line):
    """the tree of a golden definition, by the command line's own parser (tests pin that parser separately)"""
    from kmc_amd import tools

    return tools.parse_expression(tools.tokenize_expression(line[2]), {var: i for i, (var, _, _) in enumerate(line[1])})


def ordered_lists(db):
    """(kmers, counts) of a database, ascending (a KMC2 database: its bins merged)"""
    if not db.kmc2:
        return S.decode_body(db.kmer_len, db.lut_prefix_len, db.counter_size, db.lut, db.recs)
    import transform_cases as T

    kmers, counts = T.file_order(db)
    order = sorted(range(len(kmers)), key=kmers.__getitem__)
    return [kmers[i] for i in order], [counts[i] for i in order]


# ---- the device call on bodies
class ComplexContext(S.LibContext):
    """S.LibContext + kmc_hip_db_expr_device"""

    def __init__(self, path):
        super().__init__(path)
        C, capi = self.C, self.capi
        vp = C.c_void_p
        self.L.kmc_hip_db_expr_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.c_uint32, C.POINTER(capi.DbExprStep), C.c_uint32, C.POINTER(capi.DbOp), vp, C.c_uint64,
                                                  vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]

    def db_expr_device(self, kmer_len, views, steps, out, d_out, out_capacity, d_lut_out):
        C, capi = self.C, self.capi
        va, sa = (capi.DbView * max(len(views), 1))(*views), (capi.DbExprStep * max(len(steps), 1))(*[capi.DbExprStep(*s) for s in steps])
        n, st = C.c_uint64(), (C.c_uint64 * 5)()
        self._chk(self.L.kmc_hip_db_expr_device(self.h, 0, kmer_len, va, len(views), sa, len(steps), C.byref(out), d_out, out_capacity, d_lut_out, C.byref(n), st))
        return n.value, dict(zip(capi.DBX_STATS, (int(x) for x in st)))


def run_device(ctx, k, bodies, cuts, steps, ci, cx, cs, p_out, cap_records, capacity=None):
    """bodies: [(p, counter bytes, lut, recs)], one view each; steps: the postfix program over them; cap_records: the tree's bound.
    -> (lut, recs, tallies) of kmc_hip_db_expr_device"""
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
        for (p, cb, lut, recs), cut in zip(bodies, cuts):
            n = recs.size // ((k - p) // 4 + cb)
            views.append(capi.DbView(up(recs), n, up(np.asarray(lut, dtype=np.uint64)), p, cb, cut[0], cut[1]))
        rb = (k - p_out) // 4 + min(S.byte_log(cs), S.byte_log(cx))
        cap = cap_records * rb if capacity is None else capacity
        d_out, d_lut = ctx.malloc(cap + 256), ctx.malloc(8 << (2 * p_out))
        allocs.extend([d_out, d_lut])
        n, st = ctx.db_expr_device(k, views, steps, capi.DbOp(0, 0, ci, cs, cx, p_out), d_out, cap, d_lut)
        recs, lut = np.zeros(n * rb, dtype=np.uint8), np.zeros(1 << (2 * p_out), dtype=np.uint64)
        if n:
            ctx.d2h(recs, d_out)
        ctx.d2h(lut, d_lut)
        return lut, recs, st
    finally:
        for d in allocs:
            ctx.free(d)


def check_case(ctx, k, tree, inputs, fmts, p_out, ci=1, cx=U32, cs=U32, cuts=None):
    """inputs: [(kmers, counts)]; fmts: [(p, counter bytes)]. The device call on the encoded bodies must equal the restatement: records, LUT and tallies."""
    cuts = cuts or [(1, U32)] * len(inputs)
    bodies = [(p, cb, *S.encode_body(k, p, cb, *x)) for x, (p, cb) in zip(inputs, fmts)]
    seen = [(x[0], [c & ((1 << (8 * cb)) - 1) for c in x[1]]) for x, (_, cb) in zip(inputs, fmts)]  # a counter of cb bytes keeps the low bytes
    wk, wc, wst = restate(tree, seen, cuts, ci, cx, cs)
    want_lut, want_recs = S.encode_body(k, p_out, min(S.byte_log(cs), S.byte_log(cx)), wk, wc)
    lut, recs, st = run_device(ctx, k, bodies, cuts, postfix(tree), ci, cx, cs, p_out, bound(tree, [len(x[0]) for x in inputs]))
    assert st == wst, (st, wst)
    assert np.array_equal(recs, want_recs), "records differ"
    assert np.array_equal(lut, want_lut), "LUT differs"
    return st


# ---- planted databases
def left_deep(op, n, mode=None):
    t = IN(0)
    for i in range(1, n):
        t = node(op, t, IN(i), mode)
    return t


def balanced(op, lo, hi, mode=None):
    if hi - lo == 1:
        return IN(lo)
    mid = (lo + hi) // 2
    return node(op, balanced(op, lo, mid, mode), balanced(op, mid, hi, mode), mode)


REDUCED = ("identical_", "round_robin", "seam_", "wide_")


def planted_cases(k, tile, prefix_lens=None, reduced=False, seed=7):
    """-> [(name, tree, inputs, kwargs of check_case)]. `tile`: records of a tile of the library under test; the larger cases hold 3-4 tiles of records.
    prefix_lens: (p of even inputs, p of odd inputs, p of the output), default S.default_prefix_lens(k); reduced: only the cases whose names start as in REDUCED"""
    rng = np.random.default_rng(seed + k)
    n = 3 * tile + tile // 3 + 7
    p_a, p_b, p_o = prefix_lens or S.default_prefix_lens(k)
    cnt = lambda m, hi=200: [int(x) for x in rng.integers(1, hi, size=m)]  # noqa: E731
    fm = lambda m, cb=1: [((p_a, p_b)[i % 2], cb) for i in range(m)]  # noqa: E731
    all_k = S.random_kmers(rng, k, 2 * n)
    cases = []
    # every input the same keys: every key an L-way tie, the partition bound's worst case
    for L in (2, 5, MAX_LEAVES):
        m = max(n // L, 40)
        same = all_k[:m]
        cases.append((f"identical_{L}_union", left_deep("+", L), [(same, cnt(m, 9)) for _ in range(L)], dict(fmts=fm(L), p_out=p_o)))
        cases.append((f"identical_{L}_intersect_balanced", balanced("*", 0, L, "max"), [(same, cnt(m)) for _ in range(L)], dict(fmts=fm(L), p_out=p_o)))
    # disjoint keys dealt round-robin
    for L in (3, MAX_LEAVES):
        cases.append((f"round_robin_{L}", balanced("+", 0, L), [(all_k[i:n:L], cnt(len(all_k[i:n:L]))) for i in range(L)], dict(fmts=fm(L), p_out=p_o)))
    # one long leaf against leaves of 0, 1 and 2 records
    big = (all_k[:n], cnt(n))
    small = [([], []), ([all_k[n // 2]], [5]), ([all_k[3], all_k[n + 5]], [7, 9])]
    for name, tree in (("long_union_tiny", node("+", node("+", node("+", IN(0), IN(1)), IN(2)), IN(3))), ("tiny_minus_long", node("-", node("+", IN(2), IN(3)), IN(0))),
                       ("long_intersect_tiny", node("*", IN(0), node("+", IN(3), node("+", IN(1), IN(2))), "right")), ("long_diff_tiny", node("~", IN(0), node("+", IN(2), IN(3))))):
        cases.append((name, tree, [big] + small, dict(fmts=fm(4), p_out=p_o)))
    cases.append(("all_empty", left_deep("+", 3), [([], [])] * 3, dict(fmts=fm(3), p_out=p_o)))
    cases.append(("all_empty_one_leaf", IN(0), [([], [])], dict(fmts=fm(1), p_out=p_o)))
    # the same input in two leaves
    half = (all_k[1:n:2], cnt(len(all_k[1:n:2])))
    cases.append(("twice_a_minus_a", node("-", IN(0), IN(0)), [big], dict(fmts=fm(1), p_out=p_o)))
    cases.append(("twice_a_diff_a", node("~", IN(0), IN(0)), [big], dict(fmts=fm(1), p_out=p_o)))
    cases.append(("twice_a_b_a", node("+", node("*", IN(0), IN(1)), IN(0)), [big, half], dict(fmts=fm(2), p_out=p_o)))
    # diff dropping inside: a <= b everywhere, so (a ~ b) is empty, and c alone gives nothing through * left
    ca = cnt(n, 50)
    cases.append(("diff_drops_inside", node("*", node("~", IN(0), IN(1)), IN(2), "left"), [(all_k[:n], ca), (all_k[:n], [c + int(x) for c, x in zip(ca, rng.integers(0, 3, size=n))]), big],
                  dict(fmts=fm(3), p_out=p_o)))
    cases.append(("diff_keeps_some", node("*", node("~", IN(0), IN(1)), IN(2), "left"), [big, (all_k[:n], cnt(n)), half], dict(fmts=fm(3), p_out=p_o)))
    # an inner sum beyond -cs that a later ~ brings back under it; cut and clamped at the root only
    c200 = (all_k[:n], [200] * n)
    c100 = (all_k[:n], [100 + (i % 3) for i in range(n)])
    cases.append(("wide_inner_sum_reduced", node("~", node("+", IN(0), IN(1)), IN(2)), [c200, c100, c100], dict(fmts=fm(3), p_out=p_o, cs=255, cx=255)))
    cases.append(("wide_root_cut_and_clamp", node("+", node("+", IN(0), IN(1)), IN(2)), [big, half, (all_k[n // 2:n + n // 2], cnt(n, 40))],
                  dict(fmts=fm(3), p_out=p_o, ci=30, cx=200, cs=120, cuts=[(3, 150), (1, 180), (2, 30)])))
    # an inner sum that wraps 2^32 (four counter bytes) and is not cut inside
    top = [U32, U32 - 1, 7, U32, 2, U32][: min(6, n)]
    tk = all_k[: len(top)]
    cases.append(("wrap_inner_sum", node("~", node("+", IN(0), IN(1)), IN(2)), [(tk, top), (tk, [1, 2, U32, U32, U32 - 1, 5][: len(top)]), (tk, [1, 1, 3, 5, 1, 2][: len(top)])],
                  dict(fmts=fm(3, 4), p_out=p_o)))
    # a left-deep and a balanced tree at the limit, mixed operations
    mix = [(sorted(set(all_k[i::7] + all_k[(i * 3) % 5::5]))[: n // 4], None) for i in range(MAX_LEAVES)]
    mix = [(ks, cnt(len(ks))) for ks, _ in mix]
    deep = IN(0)
    for i in range(1, MAX_LEAVES):
        deep = node("+*~-"[i % 4] if i % 4 else "+", deep, IN(i))
    cases.append(("limit_left_deep", deep, mix, dict(fmts=fm(MAX_LEAVES, 2), p_out=p_o, cs=255)))
    right = IN(MAX_LEAVES - 1)
    for i in range(MAX_LEAVES - 2, -1, -1):  # right-deep: the deepest value stack
        right = node("+" if i % 3 else "~", IN(i), right)
    cases.append(("limit_right_deep", right, mix, dict(fmts=fm(MAX_LEAVES, 2), p_out=p_o)))
    cases.append(("limit_balanced", balanced("+", 0, MAX_LEAVES, "max"), mix, dict(fmts=fm(MAX_LEAVES), p_out=p_o)))
    return [c for c in cases if c[0].startswith(REDUCED)] if reduced else cases


def seam_cases(k, tile, prefix_lens=None, seed=13):
    """Records cut by their INPUT'S cutoffs at every position around a tile seam: three inputs hold the same keys, so every key is a run of three records in the merged
    order and the seams fall at every offset inside runs; who is cut goes by position with periods 2, 3 and 5 — among them the first leaf's record cut while a later
    leaf holds the key (the head of the run is then absent). A count of 2 or 240 is outside the inputs' cutoffs (10, 99)."""
    rng = np.random.default_rng(seed + k)
    n = tile + tile // 3 + 7
    p_a, p_b, p_o = prefix_lens or S.default_prefix_lens(k)
    same = S.random_kmers(rng, k, n)
    cut = (10, 99)

    def counts(period, phase):
        c = [int(x) for x in rng.integers(10, 100, size=n)]
        return [(2 if i & 4 else 240) if i % period == phase else c[i] for i in range(n)]

    cases = []
    for name, tree in (("seam_union", left_deep("+", 3)), ("seam_intersect", left_deep("*", 3, "sum")), ("seam_mixed", node("~", node("+", IN(0), IN(1)), IN(2))),
                       ("seam_minus", node("-", IN(2), node("*", IN(0), IN(1))))):
        for phase in (0, 1):
            inputs = [(same, counts(2, phase)), (same[1:], counts(3, phase)[1:]), (same, counts(5, phase))]
            cases.append((f"{name}_{phase}", tree, inputs, dict(fmts=[(p_a, 1), (p_b, 1), (p_a, 1)], p_out=p_o, cuts=[cut] * 3, cs=255)))
    return cases
