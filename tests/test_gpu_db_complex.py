"""GPU: a set expression over several ordered k-mer databases (kmc_hip_db_expr_device, `python -m kmc_amd.tools complex`) at the product tile geometry — the golden and
planted cases of tests/test_db_complex_emulated.py, two leaves against kmc_hip_db_set_op_device, one expression over 4 x 1 M k-mers for the count / scan / write passes
across thousands of tiles, and the command line against a live `kmc_tools complex` where oracle/_ref is present. Reads tests/golden and oracle/_ref only."""
import os
import subprocess

import numpy as np
import pytest

import complex_cases as X
import setops_cases as S
from kmc_amd import capi, dbio, tools

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def product_tile(k):
    """records of a tile of the key space: 32 KiB / ((words + 2) x 8) (cx_default_tile, kmc_amd/csrc/order_db.hip.h)"""
    return 32 * 1024 // (((k + 31) // 32 + 2) * 8)


@pytest.fixture(scope="module")
def inputs():
    out = {}
    for fixture in sorted({fx for _, ln in X.GOLDEN_CASES for _, fx, _ in ln[1]}):
        db = dbio.read_database(X.fixture_path(fixture))
        out[fixture] = (db, X.ordered_lists(db))
    return out


def _files(path):
    return tuple(open(path + e, "rb").read() for e in (".kmc_pre", ".kmc_suf"))


@pytest.mark.parametrize("k", sorted(X.DEFS))
def test_device_call_on_the_golden_inputs(ctx, inputs, k):
    for line in X.DEFS[k]:
        dbs = [inputs[fx][0] for _, fx, _ in line[1]]
        r, tree = X.resolve_line(line, [S.header_of(d) for d in dbs]), X.tree_of(line)
        used = sorted(set(X.leaves(tree)))
        slot = {i: q for q, i in enumerate(used)}
        bodies = []
        for i in used:
            d = dbs[i] if not dbs[i].kmc2 else inputs["setops_k33_a"][0]  # the ordered twin of the KMC2 fixture
            bodies.append((d.lut_prefix_len, d.counter_size, d.lut, d.recs))
        lut, recs, st = X.run_device(ctx, k, bodies, [r["cuts"][i] for i in used], X.postfix(tree, slot), r["ci"], r["cx"], r["cs"], r["p_out"], X.bound(tree, [d.total_kmers for d in dbs]))
        g = dbio.read_database(X.golden_out(k, line[0]))
        assert np.array_equal(recs, g.recs) and np.array_equal(lut, g.lut), line[0]
        _, _, wst = X.restate(tree, [inputs[fx][1] for _, fx, _ in line[1]], r["cuts"], r["ci"], r["cx"], r["cs"])
        assert st == wst, line[0]


def _run_cases(ctx, k, cases):
    seen = dict.fromkeys(X.TALLIES, 0)
    for name, tree, ins, kw in cases:
        try:
            st = X.check_case(ctx, k, tree, ins, **kw)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")
        for key in seen:
            seen[key] += st[key]
    return seen


@pytest.mark.parametrize("k,prefix_lens,reduced", [(k, pl, k != 27) for k, pl, _ in S.PLANTED], ids=S.PLANTED_IDS)
def test_device_call_on_planted_databases(ctx, k, prefix_lens, reduced):
    """3-4 product tiles of records; every record width (SIZE 1..7), the prefixes inside and across a 64-bit word: the full list at k = 27, the reduced one elsewhere"""
    seen = _run_cases(ctx, k, X.planted_cases(k, product_tile(k), prefix_lens=prefix_lens, reduced=reduced))
    assert all(v > 0 for v in seen.values()), seen  # every tally was exercised


@pytest.mark.parametrize("k,prefix_lens", S.SEAMS, ids=S.SEAM_IDS)
def test_cut_records_on_every_tile_seam(ctx, k, prefix_lens):
    _run_cases(ctx, k, X.seam_cases(k, product_tile(k), prefix_lens=prefix_lens))


def test_two_leaves_against_set_op(ctx, inputs):
    k = 27
    a, b = inputs["setops_k27_a"][0], inputs["setops_k27_b"][0]
    bodies = [(d.lut_prefix_len, d.counter_size, d.lut, d.recs) for d in (a, b)]
    for op in ("intersect", "union", "kmers_subtract", "counters_subtract"):
        for oc in capi.DB_COUNTER_OPS:
            for ci, cx, cs in ((1, 255, 255), (3, 20, 10)):
                want_lut, want_recs, wst = S.run_device(ctx, k, bodies[0], bodies[1], (1, 255), (2, 9), op, oc, ci, cx, cs, 3)
                tree = X.node(op, X.IN(0), X.IN(1), oc)
                lut, recs, st = X.run_device(ctx, k, bodies, [(1, 255), (2, 9)], X.postfix(tree), ci, cx, cs, 3, X.bound(tree, [a.total_kmers, b.total_kmers]))
                assert np.array_equal(recs, want_recs) and np.array_equal(lut, want_lut), (op, oc, ci)
                assert st["n_written"] == wst["n_written"] and st["n_keys"] == wst["n_pairs"] + wst["n_only_a"] + wst["n_only_b"] and st["n_above_max"] == wst["n_above_max"]


# ---- 4 x 1 M k-mers: (a + b) * c - d against numpy
def _encode27(kmers, counts, p, cb):
    """S.encode_body for k = 27 on arrays: a k-mer is 54 bits of a uint64"""
    sb = (27 - p) // 4
    sbits = np.uint64(2 * (27 - p))
    suffix = (kmers & ((np.uint64(1) << sbits) - np.uint64(1))).astype(">u8").view(np.uint8).reshape(-1, 8)[:, 8 - sb:]
    cnt = counts.astype("<u4").view(np.uint8).reshape(-1, 4)[:, :cb]
    lut = np.searchsorted(kmers >> sbits, np.arange(1 << (2 * p), dtype=np.uint64), side="left").astype(np.uint64)
    return lut, np.ascontiguousarray(np.concatenate([suffix, cnt], axis=1)).reshape(-1)


def test_four_inputs_of_a_million_kmers_against_numpy(ctx):
    k, n_pool = 27, 2_200_000
    rng = np.random.default_rng(27)
    pool = np.unique(rng.integers(0, 1 << 54, size=n_pool, dtype=np.uint64))
    member = rng.random((4, pool.size)) < 0.46  # about 1 M each; every pair shares about a fifth of the pool
    ins = [(pool[m], rng.integers(1, 201, size=int(m.sum())).astype(np.uint32)) for m in member]
    assert all(900_000 < x[0].size < 1_100_000 for x in ins)
    fmts = [(3, 1), (7, 1), (3, 2), (7, 1)]
    (ka, ca), (kb, cb), (kc, cc), (kd, cd) = ins
    # the restatement on arrays: union sum, intersect min, kmers_subtract
    ku = np.union1d(ka, kb)
    cu = np.zeros(ku.size, dtype=np.uint32)
    cu[np.searchsorted(ku, ka)] += ca
    cu[np.searchsorted(ku, kb)] += cb
    ki, iu, ic = np.intersect1d(ku, kc, assume_unique=True, return_indices=True)
    ci_ = np.minimum(cu[iu], cc[ic])
    keep = ~np.isin(ki, kd, assume_unique=True)
    wk, wc = ki[keep], ci_[keep]
    lo, hi, clamp = 20, 180, 150
    written = (wc >= lo) & (wc <= hi)
    wst = dict(n_keys=int(np.union1d(np.union1d(ku, kc), kd).size), n_result=int(wk.size), n_below_min=int((wc < lo).sum()), n_above_max=int((wc > hi).sum()), n_written=int(written.sum()))
    assert min(wst.values()) > 1000
    want_lut, want_recs = _encode27(wk[written], np.minimum(wc[written], clamp), 7, 1)
    tree = X.node("-", X.node("*", X.node("+", X.IN(0), X.IN(1)), X.IN(2)), X.IN(3))
    bodies = [(p, cbytes, *_encode27(x[0], x[1], p, cbytes)) for x, (p, cbytes) in zip(ins, fmts)]
    lut, recs, st = X.run_device(ctx, k, bodies, [(1, S.U32)] * 4, X.postfix(tree), lo, hi, clamp, 7, X.bound(tree, [x[0].size for x in ins]))
    assert st == wst
    assert np.array_equal(recs, want_recs) and np.array_equal(lut, want_lut)


# ---- the command line
def test_the_command_line_with_a_kmc2_input(ctx, tmp_path):
    k, line = next(c for c in X.GOLDEN_CASES if c[0] == 33 and c[1][0] == "kmc2_input")
    definition = tmp_path / "def.txt"
    definition.write_text(X.definition_text(line, str(tmp_path / "out")))
    st = tools.complex([str(definition)], ctx=ctx)
    assert _files(str(tmp_path / "out")) == _files(X.golden_out(k, line[0])) and st["n_written"] == 9410


@pytest.mark.parametrize("line", X.LIVE, ids=[ln[0] for ln in X.LIVE])
def test_the_command_line_against_a_live_kmc_tools(ctx, ref_bins, line, tmp_path):
    if ref_bins is None:
        pytest.skip("oracle/_ref is not built")
    ours, theirs = tmp_path / "ours.txt", tmp_path / "theirs.txt"
    ours.write_text(X.definition_text(line, str(tmp_path / "ours")))
    theirs.write_text(X.definition_text(line, str(tmp_path / "theirs")))
    subprocess.run([ref_bins["kmc_tools"], "-t1", "-hp", "complex", str(theirs)], check=True, capture_output=True, timeout=600)
    st = tools.complex([str(ours)], ctx=ctx)
    assert st["n_written"] > 0 and _files(str(tmp_path / "ours")) == _files(str(tmp_path / "theirs"))
