"""CPU: a set expression over several k-mer databases (`kmc_tools complex`) — kmc_hip_db_expr_device in the PRODUCT'S host library compiled over the emulated HIP runtime
(tests/emu.py build_hostlib, small geometry; $KMC_HIP_EXPR_TILE = 128: tiles of the key space of at most 128 records, so databases of a few hundred records cross many
tiles), and `python -m kmc_amd.tools complex` over it.

The oracle is the node-by-node restatement of tests/complex_cases.py. It is held to what `kmc_tools complex` itself wrote (tests/golden/complex_*, made by
tests/make_complex_golden.py), byte for byte, so it is pinned to the reference and not to the code under test. The -m gpu file runs the same cases on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import complex_cases as X
import emu
import setops_cases as S
from kmc_amd import capi, dbio, tools

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ECORRUPT, ECAPACITY = -1, -4, -5
TILE = 128


@pytest.fixture(scope="module")
def lib():
    os.environ["KMC_HIP_EXPR_TILE"] = str(TILE)
    c = X.ComplexContext(emu.build_hostlib("small"))
    yield c
    c.close()
    del os.environ["KMC_HIP_EXPR_TILE"]


@pytest.fixture(scope="module")
def inputs():
    """the golden inputs, read once: fixture -> (database, its (kmers, counts) ascending)"""
    out = {}
    for fixture in sorted({fx for _, ln in X.GOLDEN_CASES for _, fx, _ in ln[1]}):
        db = dbio.read_database(X.fixture_path(fixture))
        out[fixture] = (db, X.ordered_lists(db))
    return out


def _resolved(inputs, line):
    dbs = [inputs[fx][0] for _, fx, _ in line[1]]
    return dbs, X.resolve_line(line, [S.header_of(d) for d in dbs]), X.tree_of(line)


@pytest.fixture(scope="module")
def restated(inputs):
    out = {}
    for k, line in X.GOLDEN_CASES:
        _, r, tree = _resolved(inputs, line)
        out[(k, line[0])] = X.restate(tree, [inputs[fx][1] for _, fx, _ in line[1]], r["cuts"], r["ci"], r["cx"], r["cs"])
    return out


def _files(path):
    return tuple(open(path + e, "rb").read() for e in (".kmc_pre", ".kmc_suf"))


# ---- 1: the restatement is the reference
@pytest.mark.parametrize("k,line", X.GOLDEN_CASES, ids=X.GOLDEN_IDS)
def test_the_restatement_writes_what_kmc_tools_writes(inputs, restated, k, line, tmp_path):
    dbs, r, _ = _resolved(inputs, line)
    kmers, counts, st = restated[(k, line[0])]
    assert st["n_written"] > 0
    lut, recs = S.encode_body(k, r["p_out"], r["cs_bytes"], kmers, counts)
    dbio.write_kmc1(str(tmp_path / "db"), k, r["cs_bytes"], r["p_out"], r["ci"], r["cx"], all(d.both_strands for d in dbs), lut, recs, mode=dbs[0].mode)
    assert _files(str(tmp_path / "db")) == _files(X.golden_out(k, line[0]))


def test_the_goldens_hold_what_the_cases_are_about(restated):
    for k in (27, 55):
        assert restated[(k, "cutoffs")][2]["n_below_min"] > 0 and restated[(k, "cutoffs")][2]["n_above_max"] > 0 and max(restated[(k, "cutoffs")][1]) == 10
        assert dbio.read_database(X.golden_out(k, "unused_wide_input")).counter_size == 2 and dbio.read_database(X.golden_out(k, "union_of_product")).counter_size == 1
        assert restated[(k, "union_diff")][2]["n_result"] < restated[(k, "union_diff")][2]["n_keys"]  # diff dropped records inside


def test_a_chain_of_simple_calls_is_not_equivalent(inputs, restated):
    """(7 a + 4 w) ~ (4 w + a) = 6 a: the left side exceeds 255 for some k-mers; clamped there first — what every `simple` call does with -cs255 — the result differs"""
    _, line = next(c for c in X.GOLDEN_CASES if c[0] == 27 and c[1][0] == "inner_sum_beyond_cs")
    dbs, r, tree = _resolved(inputs, line)
    lists = {i: X._leaf(*inputs[fx][1], *r["cuts"][i]) for i, (_, fx, _) in enumerate(line[1])}
    left, right = X.evaluate(tree[2], lists), X.evaluate(tree[3], lists)
    assert sum(c > 255 for _, c in left) > 10
    chained = X._merge("counters_subtract", "diff", [(x, min(c, 255)) for x, c in left], right)
    ours = list(zip(*restated[(27, "inner_sum_beyond_cs")][:2]))
    assert chained != ours and len(chained) == len(ours)


# ---- 2: the device call on the golden inputs
def _golden_on_device(lib, inputs, k, line):
    dbs, r, tree = _resolved(inputs, line)
    used = sorted(set(X.leaves(tree)))
    slot = {i: q for q, i in enumerate(used)}
    assert not any(dbs[i].kmc2 for i in used) or line[0] == "kmc2_input"
    bodies = []
    for i in used:
        d = dbs[i] if not dbs[i].kmc2 else inputs["setops_k33_a"][0]  # the ordered twin of the KMC2 fixture; the command line orders the KMC2 body itself
        bodies.append((d.lut_prefix_len, d.counter_size, d.lut, d.recs))
    return X.run_device(lib, k, bodies, [r["cuts"][i] for i in used], X.postfix(tree, slot), r["ci"], r["cx"], r["cs"], r["p_out"], X.bound(tree, [d.total_kmers for d in dbs]))


@pytest.mark.parametrize("k,line", X.GOLDEN_CASES, ids=X.GOLDEN_IDS)
def test_device_call_on_the_golden_inputs(lib, inputs, restated, k, line):
    lut, recs, st = _golden_on_device(lib, inputs, k, line)
    g = dbio.read_database(X.golden_out(k, line[0]))
    assert np.array_equal(recs, g.recs) and np.array_equal(lut, g.lut)
    assert st == restated[(k, line[0])][2]


# ---- 3: two leaves are `simple`
@pytest.mark.parametrize("op", ["intersect", "union", "kmers_subtract", "counters_subtract"])
def test_two_leaves_against_simple(lib, inputs, op):
    k = 27
    a, b = inputs["setops_k27_a"][0], inputs["setops_k27_b"][0]
    bodies = [(d.lut_prefix_len, d.counter_size, d.lut, d.recs) for d in (a, b)]
    for oc in capi.DB_COUNTER_OPS:
        for ci, cx, cs in ((1, 255, 255), (3, 20, 10)) if oc == "sum" else ((1, 255, 255),):
            want_lut, want_recs, wst = S.run_device(lib, k, bodies[0], bodies[1], (1, 255), (2, 9), op, oc, ci, cx, cs, 3)
            tree = X.node(op, X.IN(0), X.IN(1), oc)
            lut, recs, st = X.run_device(lib, k, bodies, [(1, 255), (2, 9)], X.postfix(tree), ci, cx, cs, 3, X.bound(tree, [a.total_kmers, b.total_kmers]))
            assert np.array_equal(recs, want_recs) and np.array_equal(lut, want_lut), (op, oc, ci)
            assert st["n_written"] == wst["n_written"] and st["n_keys"] == wst["n_pairs"] + wst["n_only_a"] + wst["n_only_b"] and st["n_above_max"] == wst["n_above_max"]


# ---- 4: planted databases
def _run_cases(lib, k, cases):
    seen = dict.fromkeys(X.TALLIES, 0)
    for name, tree, ins, kw in cases:
        try:
            st = X.check_case(lib, k, tree, ins, **kw)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")
        for key in seen:
            seen[key] += st[key]
    return seen


@pytest.mark.parametrize("k,prefix_lens,reduced", [(k, pl, k != 27) for k, pl, _ in S.PLANTED], ids=S.PLANTED_IDS)
def test_device_call_on_planted_databases(lib, k, prefix_lens, reduced):
    """every record width (SIZE 1 .. 7), the inputs' and the output's prefixes inside and across a 64-bit word: the full list at k = 27, the reduced one elsewhere"""
    cases = X.planted_cases(k, TILE, prefix_lens=prefix_lens, reduced=reduced)
    assert len(cases) >= (8 if reduced else 25)
    seen = _run_cases(lib, k, cases)
    assert all(v > 0 for v in seen.values()), seen  # every tally was exercised


@pytest.mark.parametrize("k,prefix_lens", S.SEAMS, ids=S.SEAM_IDS)
def test_cut_records_on_every_tile_seam(lib, k, prefix_lens):
    cases = X.seam_cases(k, TILE, prefix_lens=prefix_lens)
    # the first leaf's record is cut while a later leaf holds the key, somewhere in the set
    name, tree, ins, kw = cases[0]
    lo, hi = kw["cuts"][0]
    later = set(ins[1][0])
    assert any(not (lo <= c <= hi) and x in later for x, c in zip(*ins[0]))
    _run_cases(lib, k, cases)


# ---- 5: refusals
def test_refusals(lib, inputs):
    k = 27
    a, b = inputs["setops_k27_a"][0], inputs["setops_k27_b"][0]
    good = [(d.lut_prefix_len, d.counter_size, d.lut, d.recs) for d in (a, b)]
    n = [a.total_kmers, b.total_kmers]
    union = X.node("+", X.IN(0), X.IN(1))

    def code(steps, bodies=good, cap_records=n[0] + n[1], ci=1, cs=255, p_out=3, capacity=None):
        with pytest.raises(capi.KmcHipError) as e:
            X.run_device(lib, k, bodies, [(1, 255)] * len(bodies), steps, ci, 255, cs, p_out, cap_records, capacity=capacity)
        assert "kmc_hip_db_expr_device" in str(e.value), str(e.value)
        return e.value.code, str(e.value)

    IN, U = X.EXPR_INPUT, capi.DB_OPS["union"]
    assert code([])[0] == EINVAL
    c, msg = code([(IN, 0), (U, 2)])
    assert c == EINVAL and "underflow" in msg
    c, msg = code([(IN, 0), (IN, 1)])
    assert c == EINVAL and "values left" in msg
    c, msg = code([(IN, 2)])
    assert c == EINVAL and "out of range" in msg
    assert code([(IN, 0), (IN, 1), (7, 0)])[0] == EINVAL  # an unknown operation (the reverse operations of `simple` are not nodes)
    assert code([(IN, 0), (IN, 1), (4, 0)])[0] == EINVAL
    assert code([(IN, 0), (IN, 1), (U, 6)])[0] == EINVAL  # an unknown counter mode
    too_many = X.postfix(X.left_deep("+", X.MAX_LEAVES + 1))
    c, msg = code([(kind, 0 if kind == IN else arg) for kind, arg in too_many], cap_records=17 * n[0])
    assert c == EINVAL and "MAX_LEAVES" in msg
    at_limit = [(kind, 0 if kind == IN else arg) for kind, arg in X.postfix(X.left_deep("*", X.MAX_LEAVES))]
    assert X.run_device(lib, k, good, [(1, 255)] * 2, at_limit, 1, 255, 255, 3, n[0])[2]["n_written"] == n[0]  # the limit itself is legal
    assert code(X.postfix(union), ci=0)[0] == EINVAL
    assert code(X.postfix(union), cs=0)[0] == EINVAL
    assert code(X.postfix(union), p_out=4)[0] == EINVAL  # (27 - 4) % 4 != 0
    assert code(X.postfix(union), bodies=[good[0], (3, 0, b.lut, b.recs)])[0] == EINVAL  # counter size 0
    assert code(X.postfix(union), bodies=[good[0], (3, 5, b.lut, b.recs[:0])])[0] == EINVAL
    bad = b.lut.copy()
    bad[-1] = n[1] + 1
    c, msg = code(X.postfix(union), bodies=[good[0], (3, 1, bad, b.recs)])
    assert c == ECORRUPT and "LUT" in msg
    assert code([(IN, 0)], bodies=[good[0], (3, 1, bad, b.recs)])[0] == ECORRUPT  # a view the expression does not name is checked too
    # capacity: the tree's own bound, to the byte
    rb = (k - 3) // 4 + 1
    for tree, bound in ((union, n[0] + n[1]), (X.node("*", X.IN(0), X.IN(1)), min(n)), (X.node("-", X.IN(1), X.IN(0)), n[1]), (X.node("~", X.IN(0), X.node("+", X.IN(1), X.IN(1))), n[0])):
        assert X.bound(tree, n) == bound
        assert code(X.postfix(tree), capacity=bound * rb - 1)[0] == ECAPACITY
        X.run_device(lib, k, good, [(1, 255)] * 2, X.postfix(tree), 1, 255, 255, 3, bound, capacity=bound * rb)
    # NULL arguments
    L, C = lib.L, lib.C
    d = lib.malloc(4096)
    try:
        lib.h2d(d, np.zeros(4096, dtype=np.uint8))  # a LUT of zeros
        v = (capi.DbView * 1)(capi.DbView(d, 0, d, 3, 1, 1, 255))
        steps = (capi.DbExprStep * 1)(capi.DbExprStep(IN, 0))
        out = capi.DbOp(0, 0, 1, 255, 255, 3)
        n_out, st = C.c_uint64(), (C.c_uint64 * 5)()
        args = [lib.h, 0, k, v, 1, steps, 1, C.byref(out), d, 1024, d, C.byref(n_out), st]
        assert L.kmc_hip_db_expr_device(*args) == 0 and n_out.value == 0  # an empty input is legal
        for i in (3, 5, 7, 8, 10, 11, 12):
            assert L.kmc_hip_db_expr_device(*[None if j == i else x for j, x in enumerate(args)]) == EINVAL
            assert b"kmc_hip_db_expr_device: NULL" in L.kmc_hip_last_error(lib.h)
        no_lut = (capi.DbView * 1)(capi.DbView(d, 0, 0, 3, 1, 1, 255))
        assert L.kmc_hip_db_expr_device(*[no_lut if j == 3 else x for j, x in enumerate(args)]) == EINVAL and b"NULL" in L.kmc_hip_last_error(lib.h)
        v225 = (capi.DbView * 1)(capi.DbView(d, 0, d, 1, 1, 1, 255))
        assert L.kmc_hip_db_expr_device(lib.h, 0, 225, v225, 1, steps, 1, C.byref(capi.DbOp(0, 0, 1, 255, 255, 1)), d, 1024, d, C.byref(n_out), st) == EINVAL  # kmer_len > 224
    finally:
        lib.free(d)


def test_inputs_that_are_not_ordered_sets_are_reported_not_overrun(lib):
    """every leaf the same key throughout: no splitter separates them, so a tile holds more than its LDS — the guard reports it and writes nothing"""
    k, n = 27, 4 * TILE
    lut, recs = S.encode_body(k, 3, 1, [12345] * n, [1] * n)
    with pytest.raises(capi.KmcHipError) as e:
        X.run_device(lib, k, [(3, 1, lut, recs)] * 2, [(1, 255)] * 2, X.postfix(X.node("+", X.IN(0), X.IN(1))), 1, 255, 255, 3, 2 * n)
    assert e.value.code == ECORRUPT and "kmc_hip_db_expr_device" in str(e.value)


# ---- 6: the binding
def test_the_binding_knows_the_entry_point():
    assert "kmc_hip_db_expr_device" in capi.SYMBOLS and hasattr(capi.Context, "db_expr_device")
    assert capi.DBX_STATS == X.TALLIES and capi.DB_EXPR_INPUT == X.EXPR_INPUT and capi.DB_EXPR_MAX_LEAVES == X.MAX_LEAVES
    with open(os.path.join(ROOT, "include", "kmc_hip.h")) as f:
        header = f.read()
    assert "int kmc_hip_db_expr_device(" in header and "#define KMC_HIP_DB_EXPR_INPUT 16u" in header and "#define KMC_HIP_DB_EXPR_MAX_LEAVES 16" in header


# ---- 7: the command line's parser, without a device
NAMES = {"a": 0, "b": 1, "c": 2, "x": 3, "minimum": 4}


def _tree(expression):
    return tools.parse_expression(tools.tokenize_expression(expression), NAMES)


def test_precedence_associativity_and_modifiers():
    a, b, c = X.IN(0), X.IN(1), X.IN(2)
    assert _tree("a + b * c") == X.node("+", a, X.node("*", b, c))
    assert _tree("a * b + c") == X.node("+", X.node("*", a, b), c)
    assert _tree("(a + b) * c") == X.node("*", X.node("+", a, b), c)
    assert _tree("a - b - c") == X.node("-", X.node("-", a, b), c)
    assert _tree("a - (b - c)") == X.node("-", a, X.node("-", b, c))
    assert _tree("a ~ b + c - a") == X.node("-", X.node("+", X.node("~", a, b), c), a)
    assert _tree("a * b * c") == X.node("*", X.node("*", a, b), c)
    assert _tree("a ~ min b + max c") == X.node("+", X.node("~", a, b, "min"), c, "max")
    assert _tree("a * left b * right c") == X.node("*", X.node("*", a, b, "left"), c, "right")
    assert _tree("a +sum(b ~diff c)") == X.node("+", a, X.node("~", b, c, "diff"), "sum")
    assert _tree("a+b") == _tree("  a\t+ b ") == X.node("+", a, b)
    # the defaults: union sum, intersect min, ~ diff
    assert [_tree(f"a {o} b")[1] for o in "+*~-"] == ["sum", "min", "diff", "diff"]
    assert X.postfix(_tree("a + b * c")) == [(16, 0), (16, 1), (16, 2), (capi.DB_OPS["intersect"], capi.DB_COUNTER_OPS["min"]), (capi.DB_OPS["union"], capi.DB_COUNTER_OPS["sum"])]
    assert tools.expr_steps(_tree("(a ~ b) * max c")) == X.postfix(_tree("(a ~ b) * max c"))


def test_keywords_match_as_prefixes():
    assert tools.tokenize_expression("a * minx") == [("a", "var"), ("*", "*"), ("min", "min"), ("x", "var")]
    assert _tree("a * minx") == X.node("*", X.IN(0), X.IN(3), "min")
    # so a name that starts with a keyword cannot be used where a modifier may stand, or anywhere else
    with pytest.raises(tools.UsageError, match="imum"):
        _tree("a + minimum")
    with pytest.raises(tools.UsageError):
        _tree("minimum + a")


@pytest.mark.parametrize("expression,word", [("a + min", "expected"), ("a * max", "expected"), ("a - min b", "min"), ("min", "expected"), ("a + * b", "expected"), ("a +", "expected"),
                                             ("", "empty"), ("   ", "empty"), ("a $ b", "near"), ("a + b.c", "near"), ("a + d", "not defined"), ("a b", "wrong symbol"),
                                             ("(a + b", "parenthesis"), ("a + b)", "wrong symbol"), ("()", "expected")])
def test_expressions_that_are_refused(expression, word):
    with pytest.raises(tools.UsageError, match=word):
        _tree(expression)


def _definition(inputs="a = /p/a\nb = /p/b -ci3 -cx9\n", output="/p/out = a + b\n", params=None):
    return "INPUT:\n" + inputs + "OUTPUT:\n" + output + ("OUTPUT_PARAMS:\n" + params if params is not None else "")


def test_the_definition_file_is_split_as_the_reference_splits_it():
    o = tools.parse_complex(_definition(params="-ci2 -cx40 -cs10 -okmc\n"))
    assert o["inputs"] == [("a", "/p/a", 0, 0), ("b", "/p/b", 3, 9)] and o["path"] == "/p/out" and (o["ci"], o["cx"], o["cs"]) == (2, 40, 10)
    assert o["tree"] == X.node("+", X.IN(0), X.IN(1))
    # the section names anywhere in a line, blank lines skipped, lines between the output and OUTPUT_PARAMS: ignored, the parameters on the next non-blank line
    text = "# a comment\n\n  here INPUT: starts\n\n a=/p/a\n\n\tb = /p/b\t-cx7 \nthe OUTPUT: \n\n /p/o ut  = b-a \n whatever = a\n\nnow OUTPUT_PARAMS: -ci9\n\n -cs3\n-ci5\n"
    o = tools.parse_complex(text)
    assert o["inputs"] == [("a", "/p/a", 0, 0), ("b", "/p/b", 0, 7)] and o["path"] == "/p/o ut" and o["tree"] == X.node("-", X.IN(1), X.IN(0)) and (o["ci"], o["cx"], o["cs"]) == (0, 0, 3)
    # the output pattern is greedy: the path reaches to the LAST '='
    assert tools.parse_complex(_definition(output="/p/x=y = a\n"))["path"] == "/p/x=y"
    assert tools.parse_complex(_definition(params=""))["cs"] == 0  # OUTPUT_PARAMS: without parameters is a warning in the reference
    assert [i[0] for i in tools.parse_complex(_definition(inputs="a-1 = /p/a\nb = /p/b\n", output="/p/o = b\n"))["inputs"]] == ["a-1", "b"]  # the input pattern takes + and - in a name


@pytest.mark.parametrize("text,word", [
    ("OUTPUT:\n/p/o = a\n", "'INPUT:' missing"), ("INPUT:\nOUTPUT:\n/p/o = a\n", "None input"), ("INPUT:\na = /p/a\n", "'OUTPUT:' missing"),
    ("INPUT:\na = /p/a\nOUTPUT:\n", "None output"), ("INPUT:\na = /p/a\nOUTPUT:\nOUTPUT_PARAMS:\n-ci2\n", "None output"),
    (_definition(inputs="a = /p/a\na = /p/b\n"), "redefinition"), (_definition(inputs="a = /p/a\nmin = /p/b\n"), "not valid name"), (_definition(inputs="a = /p/a\nleft = /p/b\n"), "not valid name"),
    (_definition(inputs="a = /p/a\nb =\n"), "not specified"), (_definition(inputs="a = /p/a\nb /p/b\n"), "wrong line format"), (_definition(inputs="a = /p/a -cs9\nb = /p/b\n"), "Unknow parameter"),
    (_definition(inputs="a = /p/a -cix\nb = /p/b\n"), "bad value"), (_definition(output=" = a + b\n"), "not specified"), (_definition(output="/p/o a + b\n"), "wrong line format"),
    (_definition(output="/p/o = a + c\n"), "not defined"), (_definition(output="/p/o =\n"), "empty"), (_definition(params="-okff\n"), "KFF"), (_definition(params="-oxyz\n"), "Unknown output type"),
    (_definition(params="-ci2 -q\n"), "Unknow parameter"), (_definition(params="-cs1x\n"), "bad value")])
def test_definition_files_that_are_refused(text, word):
    with pytest.raises(tools.UsageError, match=word):
        tools.parse_complex(text)


def test_the_defaults_count_every_defined_input(inputs):
    """parameters_parser.cpp:842-848,893-916: -ci / -cx / -cs and the LUT prefix come from ALL inputs of the file, the unused two-byte one too"""
    k, line = next(c for c in X.GOLDEN_CASES if c[0] == 27 and c[1][0] == "unused_wide_input")
    o = tools.parse_complex(X.definition_text(line, "/p/out"))
    dbs = [inputs[fx][0] for _, fx, _ in line[1]]
    r = tools.resolve_complex(o, dbs)
    want = X.resolve_line(line, [S.header_of(d) for d in dbs])
    assert {key: r[key] for key in want} == want and (r["cs"], r["cs_bytes"]) == (65535, 2) and r["cx"] == max(d.max_count for d in dbs) and r["canonical"]
    assert tools.resolve_complex(tools.parse_complex(X.definition_text(("x", line[1][:1] + line[1][2:], "a + b", None), "/p/out")), [dbs[0], dbs[2]])["cs"] == 255
    k55 = inputs["setops_k55_a"][0]
    with pytest.raises(tools.UsageError, match="different k-mer lengths"):
        tools.resolve_complex(o, [dbs[0], dbs[1], k55])
    header = tools._read_header(X.fixture_path("setops_k33_raw_a"))
    raw = inputs["setops_k33_raw_a"][0]
    assert S.header_of(header) == S.header_of(raw) and header.kmc2 and header.both_strands == raw.both_strands and header.recs is None


# ---- 8: the command line end to end
CLI_CASES = [c for c in X.GOLDEN_CASES if (c[0], c[1][0]) in ((27, "cutoffs"), (27, "unused_wide_input"), (27, "inner_sum_beyond_cs"), (55, "modes"), (33, "kmc2_input"), (33, "one_input"))]


@pytest.mark.parametrize("k,line", CLI_CASES, ids=[f"{ln[0]}-{k}" for k, ln in CLI_CASES])
def test_the_command_line_writes_the_golden_files(lib, restated, k, line, tmp_path):
    definition = tmp_path / "def.txt"
    definition.write_text(X.definition_text(line, str(tmp_path / "out")))
    st = tools.complex([str(definition)], ctx=lib)
    assert _files(str(tmp_path / "out")) == _files(X.golden_out(k, line[0]))
    assert st == restated[(k, line[0])][2]


def test_the_command_line_names_what_it_refuses(tmp_path):
    with pytest.raises(tools.UsageError, match="usage"):
        tools.complex([])
    with pytest.raises(tools.UsageError, match="cannot open"):
        tools.complex([str(tmp_path / "missing.txt")])
    a = X.fixture_path("setops_k27_a")
    f = tmp_path / "d.txt"
    f.write_text(f"INPUT:\na = {a}\nOUTPUT:\n{tmp_path / 'o'} = " + " + ".join(["a"] * 17) + "\n")
    with pytest.raises(tools.UsageError, match="at most 16"):
        tools.complex([str(f)])
    f.write_text(f"INPUT:\na = {a}\nb = {tmp_path / 'nothing'}\nOUTPUT:\n{tmp_path / 'o'} = a\n")
    with pytest.raises(tools.UsageError):
        tools.complex([str(f)])  # an input that is not used must exist all the same: its header is read
    assert sorted(os.listdir(tmp_path)) == ["d.txt"]


def test_python_m_kmc_amd_tools_complex(tmp_path):
    """the process as a user starts it"""
    k, line = next(c for c in X.GOLDEN_CASES if c[0] == 27 and c[1][0] == "union_diff")
    definition = tmp_path / "def.txt"
    definition.write_text(X.definition_text(line, str(tmp_path / "out")))
    r = subprocess.run([sys.executable, "-m", "kmc_amd.tools", "complex", str(definition)], cwd=ROOT, capture_output=True, text=True, timeout=1200,
                       env=dict(os.environ, KMC_HIP_LIB=emu.build_hostlib("small"), KMC_HIP_EXPR_TILE=str(TILE)))
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    assert _files(str(tmp_path / "out")) == _files(X.golden_out(k, line[0]))
    assert "complex ->" in r.stdout and "n_written 2894" in r.stdout and "n_keys 5804" in r.stdout


# ---- 9: against a live kmc_tools
@pytest.mark.parametrize("line", X.LIVE, ids=[ln[0] for ln in X.LIVE])
def test_the_command_line_against_a_live_kmc_tools(lib, ref_bins, line, tmp_path):
    if ref_bins is None:
        pytest.skip("oracle/_ref is not built")
    ours, theirs = tmp_path / "ours.txt", tmp_path / "theirs.txt"
    ours.write_text(X.definition_text(line, str(tmp_path / "ours")))
    theirs.write_text(X.definition_text(line, str(tmp_path / "theirs")))
    subprocess.run([ref_bins["kmc_tools"], "-t1", "-hp", "complex", str(theirs)], check=True, capture_output=True, timeout=600)
    st = tools.complex([str(ours)], ctx=lib)
    assert st["n_written"] > 0 and _files(str(tmp_path / "ours")) == _files(str(tmp_path / "theirs"))
