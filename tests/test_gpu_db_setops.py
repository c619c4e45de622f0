"""GPU: set operations between two ordered k-mer databases (kmc_hip_db_set_op_device, `python -m kmc_amd.tools simple`) at the product tile geometry — the
golden and planted cases of tests/test_db_setops_emulated.py, one case of 2 M + 2 M k-mers for the scan across thousands of tiles, and the command line against a
live `kmc_tools simple` where oracle/_ref is present. Reads tests/golden and oracle/_ref only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import setops_cases as S
from kmc_amd import dbio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def product_tile(k):
    """records of a merge tile: SO_THREADS x max(1, SO_IPT_WORDS / (words + 1)) (kmc_amd/csrc/order_db.hip.h)"""
    return 256 * max(1, 8 // ((k + 31) // 32 + 1))


@pytest.fixture(scope="module")
def goldens():
    out = {}
    for k in S.PAIRS:
        dbs = [S.golden_db(k, n) for n in "ab"]
        out[k] = (dbs, [S.decode_body(k, d.lut_prefix_len, d.counter_size, d.lut, d.recs) for d in dbs])
    return out


@pytest.mark.parametrize("k", S.PAIRS)
def test_device_call_on_the_golden_inputs(ctx, goldens, k):
    (a, b), decoded = goldens[k]
    for line in S.LINES_OF[k]:
        r = S.resolve_line(line, S.header_of(a), S.header_of(b))
        lut, recs, st = S.run_device(ctx, k, (a.lut_prefix_len, a.counter_size, a.lut, a.recs), (b.lut_prefix_len, b.counter_size, b.lut, b.recs), r["a_cut"], r["b_cut"],
                                     r["op"], r["oc"], r["ci"], r["cx"], r["cs"], r["p_out"])
        want = S.golden_db(k, line[0])
        assert np.array_equal(recs, want.recs) and np.array_equal(lut, want.lut), line[0]
        _, _, wst = S.restate(*decoded, r["a_cut"], r["b_cut"], r["op"], r["oc"], r["ci"], r["cx"], r["cs"])
        assert st == wst, line[0]


@pytest.mark.parametrize("k,prefix_lens,reduced", S.PLANTED, ids=S.PLANTED_IDS)
def test_device_call_on_planted_databases(ctx, k, prefix_lens, reduced):
    """3-4 product tiles; A == B in both parities (equal_*, equal_shifted_*); every record width (SIZE 1..7) and the LUT prefix of A, of B and of the output across a
    64-bit word boundary (setops_cases.PLANTED)"""
    seen = dict(n_pairs=0, n_only_a=0, n_only_b=0, n_below_min=0, n_above_max=0, n_written=0)
    for name, a, b, kw in S.planted_cases(k, product_tile(k), prefix_lens=prefix_lens, reduced=reduced):
        try:
            st = S.check_case(ctx, k, a, b, **kw)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")
        for key in seen:
            seen[key] += st[key]
    assert all(v > 0 for v in seen.values()), seen  # every tally was exercised


@pytest.mark.parametrize("k,prefix_lens", S.SEAMS, ids=S.SEAM_IDS)
def test_cut_records_on_every_tile_seam(ctx, k, prefix_lens):
    """equal key sets in both parities, one side or the other cut by its INPUT'S cutoffs at every position, at the product tile (setops_cases.seam_cut_cases)"""
    for name, a, b, kw in S.seam_cut_cases(k, product_tile(k), prefix_lens):
        try:
            S.check_case(ctx, k, a, b, **kw)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")


@pytest.mark.parametrize("k", sorted(S.RAW_A))
def test_the_command_line_orders_a_kmc2_fixture_first(k, tmp_path):
    """the database as `kmc` wrote it (KMC2) as first input: ordered on the device, then united with b == the `union` golden"""
    r = subprocess.run([sys.executable, "-m", "kmc_amd.tools", "simple", S.golden_path(k, S.RAW_A[k]), S.golden_path(k, "b"), "union", str(tmp_path / "u")], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    for ext in (".kmc_pre", ".kmc_suf"):
        assert open(str(tmp_path / "u") + ext, "rb").read() == open(S.golden_path(k, "union") + ext, "rb").read(), ext


def _body27(kmers, counts):
    """vectorised encode_body for k = 27, p = 3, one counter byte"""
    suf = (kmers & np.uint64((1 << 48) - 1)).astype(">u8").view(np.uint8).reshape(-1, 8)[:, 2:]
    recs = np.concatenate([suf, counts.astype(np.uint8)[:, None]], axis=1).reshape(-1)
    lut = np.searchsorted(kmers >> np.uint64(48), np.arange(64, dtype=np.uint64), side="left").astype(np.uint64)
    return lut, np.ascontiguousarray(recs)


def test_two_million_and_two_million(ctx):
    """2 M + 2 M random 27-mers, half of them shared: thousands of tiles through the count / scan / write launches"""
    rng = np.random.default_rng(9)
    pool = np.unique(rng.integers(0, 1 << 54, size=3_200_000, dtype=np.uint64))[:3_000_000]
    pool = pool[rng.permutation(pool.size)]
    ka, kb = np.sort(pool[:2_000_000]), np.sort(pool[1_000_000:])
    ca, cb = rng.integers(1, 200, size=ka.size).astype(np.uint64), rng.integers(1, 200, size=kb.size).astype(np.uint64)
    bodies = [(3, 1, *_body27(ka, ca)), (3, 1, *_body27(kb, cb))]
    both, ia, ib = np.intersect1d(ka, kb, assume_unique=True, return_indices=True)
    assert both.size == 1_000_000
    # intersect, -ocmin
    lut, recs, st = S.run_device(ctx, 27, *bodies, (1, 255), (1, 255), "intersect", "min", 1, 255, 255, 3)
    w_lut, w_recs = _body27(both, np.minimum(ca[ia], cb[ib]))
    assert st == dict(n_pairs=1_000_000, n_only_a=1_000_000, n_only_b=1_000_000, n_below_min=0, n_above_max=0, n_written=1_000_000)
    assert np.array_equal(lut, w_lut) and np.array_equal(recs, w_recs)
    # union, -ocsum, clamped at 255
    uni = np.union1d(ka, kb)
    cnt = np.zeros(uni.size, dtype=np.uint64)
    cnt[np.searchsorted(uni, ka)] += ca
    cnt[np.searchsorted(uni, kb)] += cb
    lut, recs, st = S.run_device(ctx, 27, *bodies, (1, 255), (1, 255), "union", "sum", 1, 10**9, 255, 3)
    w_lut, w_recs = _body27(uni, np.minimum(cnt, 255))
    assert st["n_written"] == 3_000_000 and np.array_equal(lut, w_lut) and np.array_equal(recs, w_recs)


def test_the_command_line_against_a_live_kmc_tools(ref_bins, tmp_path):
    if ref_bins is None:
        pytest.skip("oracle/_ref not shipped")
    a, b = S.golden_path(27, "a"), S.golden_path(27, "b")
    tail = lambda d: ["union", str(tmp_path / (d + "_u")), "-ocmax", "-cs20", "intersect", str(tmp_path / (d + "_i")), "reverse_counters_subtract", str(tmp_path / (d + "_r")), "-ci2"]  # noqa: E731
    subprocess.run([ref_bins["kmc_tools"], "simple", a, "-ci2", b, "-cx30", *tail("ref")], check=True, capture_output=True)
    r = subprocess.run([sys.executable, "-m", "kmc_amd.tools", "simple", a, "-ci2", b, "-cx30", *tail("got")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    for o in "uir":
        for ext in (".kmc_pre", ".kmc_suf"):
            assert open(str(tmp_path / f"got_{o}") + ext, "rb").read() == open(str(tmp_path / f"ref_{o}") + ext, "rb").read(), (o, ext)
        assert dbio.read_database(str(tmp_path / f"got_{o}")).total_kmers > 100
