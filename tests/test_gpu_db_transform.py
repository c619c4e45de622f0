"""GPU: one k-mer database transformed (kmc_hip_db_reduce_device, kmc_hip_db_histogram_device, kmc_hip_db_dump_device, `python -m kmc_amd.tools transform`) at the
product tile geometry — the golden and planted cases of tests/test_db_transform_emulated.py, histograms of 2 M records in LDS and in HBM, one database of 2 M k-mers
against numpy, and the command line against a live `kmc_tools transform` where oracle/_ref is present. Reads tests/golden and oracle/_ref only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import setops_cases as S
import transform_cases as T
from kmc_amd import dbio, tools

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = S.U32


def product_tile(k):
    """the larger of the dump tile (32 KiB of text) and the reduce tile (256 records)"""
    return max(T.default_dump_tile(k), T.REDUCE_TILE)


@pytest.fixture(scope="module")
def inputs():
    out = {}
    for fixture in sorted({ln[1] for ln in T.LINES + T.LIVE_LINES}):
        out[fixture] = dbio.read_database(T.fixture_path(fixture))
    return out


# ---- planted databases, every record width
@pytest.mark.parametrize("k,p,p_out", T.KS, ids=T.K_IDS)
def test_planted_databases(ctx, k, p, p_out):
    """3 1/3 product tiles; counters of 1..4 bytes at the decimal-length edges, records cut by the input's and by the output's cutoffs on every tile seam, whole tiles
    cut, clamps that change the digit count, everything cut, an empty database, one record, one prefix; reduce, dump and histogram on every case"""
    seen = dict.fromkeys(T.TALLIES, 0)
    for name, c in T.planted_cases(k, p, product_tile(k)):
        lut, recs = S.encode_body(k, p, c["cb"], c["kmers"], c["counts"])
        try:
            with T.DeviceBody(ctx, k, p, c["cb"], lut, recs) as body:
                st = T.check_reduce(ctx, body, c["kmers"], c["counts"], c["in_cut"], c["ci"], c["cx"], c["cs"], c["value"], p_out)
                if not c["value"]:
                    assert T.check_dump(ctx, body, c["kmers"], c["counts"], c["in_cut"], c["ci"], c["cx"], c["cs"]) == st
                T.check_histogram(ctx, body, c["counts"], c["in_cut"], *T.histogram_window(c))
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")
        for key in seen:
            seen[key] += st[key]
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("k,p", [(27, 3), (33, 5), (65, 9)])
def test_dump_and_histogram_of_a_segmented_body(ctx, k, p):
    """a KMC2-shaped LUT (empty segments at the front, in the middle and at the end, recurring prefixes), whole and in record ranges that start and end inside tiles"""
    tile = product_tile(k)
    segments, kmers, counts = T.segmented_case(k, p, tile)
    lut, recs = T.encode_segmented(k, p, 1, segments)
    with T.DeviceBody(ctx, k, p, 1, lut, recs, n_seg=len(segments)) as body:
        T.check_dump(ctx, body, kmers, counts, (1, U32), 1, U32, U32)
        T.check_histogram(ctx, body, counts, (5, 150), 20, 120)
        whole, _ = T.restate_dump(k, kmers, counts, (5, 150), 20, 120, 99)
        cuts = [0, 1, tile - 1, tile + 77, 2 * tile + 77, 2 * tile + 78, len(kmers) - 3, len(kmers)]
        parts = []
        for a, b in zip(cuts, cuts[1:]):
            want, wst = T.restate_dump(k, kmers[a:b], counts[a:b], (5, 150), 20, 120, 99)
            text, st = T.run_dump(ctx, body, (5, 150), 20, 120, 99, first=a, count=b - a, base_offset=len(parts) % 16)
            assert (text, st) == (want, wst), (a, b)
            parts.append(text)
        assert b"".join(parts) == whole


def test_the_text_starts_at_every_byte_offset(ctx):
    """a capacity of exactly count x (k + 12), d_text at each residue of an address modulo 16, the guard in front of it and behind *n_bytes intact"""
    k, p = 27, 3
    rng = np.random.default_rng(1)
    n = 2 * T.default_dump_tile(k) + 31
    kmers = S.random_kmers(rng, k, n)
    counts = [T.DIGIT_EDGES[i % 12] for i in range(n)]
    lut, recs = S.encode_body(k, p, 3, kmers, counts)
    with T.DeviceBody(ctx, k, p, 3, lut, recs) as body:
        for off in range(16):
            T.check_dump(ctx, body, kmers, counts, (1, U32), 1, U32, U32, base_offset=off, capacity=n * (k + 12))
        for count in (1, 2, 3):
            T.check_dump(ctx, body, kmers[:count], counts[:count], (1, U32), 1, U32, U32, base_offset=7, count=count)


# ---- histograms
@pytest.fixture(scope="module")
def large():
    """k = 27, p 7, 2 M distinct k-mers, two counter bytes, a k-mer-spectrum-like draw: about 70 % ones and a geometric tail. Made once, shared, not changed."""
    k, p, n = 27, 7, 2_000_000
    rng = np.random.default_rng(27)
    kmers = np.unique(rng.integers(0, 1 << (2 * k), size=n + n // 50, dtype=np.uint64))[:n]
    assert kmers.size == n
    counts = np.where(rng.random(n) < 0.7, 1, 1 + rng.geometric(0.02, size=n)).astype(np.uint32)
    sb = (k - p) // 4
    be = kmers.astype(">u8").view(np.uint8).reshape(n, 8)
    recs = np.ascontiguousarray(np.concatenate([be[:, 8 - sb:], counts.astype("<u2").view(np.uint8).reshape(n, 2)], axis=1))
    lut = np.searchsorted(kmers >> np.uint64(2 * (k - p)), np.arange(1 << (2 * p), dtype=np.uint64), side="left").astype(np.uint64)
    return dict(k=k, p=p, n=n, kmers=kmers, counts=counts, lut=lut, recs=recs.reshape(-1))


def test_histogram_of_one_counter(ctx, large):
    """all 2 M records hold counter 1: one bin, the worst contention, a total above 2^20"""
    n, sb = large["n"], (large["k"] - large["p"]) // 4
    recs = large["recs"].reshape(n, sb + 2).copy()
    recs[:, sb:] = (1, 0)
    with T.DeviceBody(ctx, large["k"], large["p"], 2, large["lut"], recs.reshape(-1)) as body:
        for lo, hi in ((1, 1), (1, 255), (1, T.HIST_LDS_BINS + 1)):
            hist, st = T.run_histogram(ctx, body, (1, U32), lo, hi)
            assert int(hist[0]) == n > 1 << 20 and not hist[1:].any() and st == dict(n_cut_in=0, n_outside=0, n_counted=n)


def test_histogram_in_lds_and_in_hbm_agree(ctx, large):
    n, counts = large["n"], large["counts"]
    full = np.bincount(counts, minlength=T.HIST_LDS_BINS + 2)
    with T.DeviceBody(ctx, large["k"], large["p"], 2, large["lut"], large["recs"]) as body:
        a, sa = T.run_histogram(ctx, body, (1, U32), 1, T.HIST_LDS_BINS)  # the widest range in LDS
        b, sb_ = T.run_histogram(ctx, body, (1, U32), 1, T.HIST_LDS_BINS + 1)  # one more: 64-bit atomics in HBM
        assert np.array_equal(a, b[:-1]) and np.array_equal(b, full[1:T.HIST_LDS_BINS + 2]) and sa == sb_ == dict(n_cut_in=0, n_outside=0, n_counted=n)
        c, sc = T.run_histogram(ctx, body, (2, 300), 5, 200)  # bin 0 is counter 5, not counter 0
        assert np.array_equal(c, full[5:201])
        assert sc == dict(n_cut_in=int(((counts < 2) | (counts > 300)).sum()), n_outside=int((((counts >= 2) & (counts < 5)) | ((counts > 200) & (counts <= 300))).sum()), n_counted=int(full[5:201].sum()))


def test_histogram_of_counters_near_the_top(ctx):
    k, p = 27, 3
    rng = np.random.default_rng(3)
    n = 5000
    kmers = S.random_kmers(rng, k, n)
    counts = [U32 - int(x) for x in rng.integers(0, 6, size=n)]
    lut, recs = S.encode_body(k, p, 4, kmers, counts)
    with T.DeviceBody(ctx, k, p, 4, lut, recs) as body:
        T.check_histogram(ctx, body, counts, (1, U32), U32 - 3, U32)
        T.check_histogram(ctx, body, counts, (1, U32 - 1), U32 - 4, U32 - 2)


# ---- one large database against numpy
def _numpy_dump(k, kmers, counts):
    n = kmers.size
    rows = np.zeros((n, k + 12), dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(k):
        rows[:, i] = acgt[((kmers >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)).astype(np.intp)]
    rows[:, k] = 9
    c = counts.astype(np.uint64)
    nd = np.ones(n, dtype=np.intp)
    for d in range(1, 10):
        nd += c >= 10 ** d
    for j in range(10):
        has = j < nd
        rows[has, k + 1 + j] = 48 + ((c[has] // (10 ** (nd[has] - 1 - j)).astype(np.uint64)) % np.uint64(10))
    rows[np.arange(n), k + 1 + nd] = 10
    return rows[np.arange(k + 12)[None, :] < (k + 2 + nd)[:, None]].tobytes()


def test_two_million_kmers_against_numpy(ctx, large):
    k, p, n, kmers, counts = (large[x] for x in ("k", "p", "n", "kmers", "counts"))
    in_cut, ci, cx, cs = (1, 400), 2, 150, 99
    present = (counts >= in_cut[0]) & (counts <= in_cut[1])
    keep = present & (counts >= ci) & (counts <= cx)
    want_st = dict(n_cut_in=int((~present).sum()), n_below_min=int((present & (counts < ci)).sum()), n_above_max=int((present & (counts > cx)).sum()), n_written=int(keep.sum()))
    assert all(v > 0 for v in want_st.values())
    out_counts = np.minimum(counts[keep], cs)
    with T.DeviceBody(ctx, k, p, 2, large["lut"], large["recs"]) as body:
        text, st = T.run_dump(ctx, body, in_cut, ci, cx, cs)
        assert st == want_st
        assert text == _numpy_dump(k, kmers[keep], out_counts)
        lut, recs, st = T.run_reduce(ctx, body, in_cut, ci, cx, cs, 0, p)
        assert st == want_st
        sb = (k - p) // 4
        assert np.array_equal(recs.reshape(-1, sb + 1)[:, :sb], large["recs"].reshape(n, sb + 2)[keep][:, :sb]) and np.array_equal(recs.reshape(-1, sb + 1)[:, sb], out_counts.astype(np.uint8))
        assert np.array_equal(lut, np.searchsorted(kmers[keep] >> np.uint64(2 * (k - p)), np.arange(1 << (2 * p), dtype=np.uint64), side="left").astype(np.uint64))
        hist, sth = T.run_histogram(ctx, body, in_cut, ci, cx)
        assert np.array_equal(hist, np.bincount(counts[keep], minlength=cx + 1)[ci:cx + 1]) and sth["n_counted"] == want_st["n_written"]


# ---- the command line
def _check_outputs(line, paths):
    for i, (op, _) in enumerate(line[3]):
        if T.is_text(op):
            assert open(paths[i], "rb").read() == T.read_golden_text(line, i), (line[0], i)
        elif os.path.exists(T.golden_out(line, i) + ".kmc_pre"):
            assert tuple(open(paths[i] + e, "rb").read() for e in (".kmc_pre", ".kmc_suf")) == T.golden_database_files(line, i), (line[0], i)
        else:
            assert not os.path.exists(paths[i] + ".kmc_pre")


@pytest.mark.parametrize("line", T.LINES, ids=T.LINE_IDS)
def test_the_command_line_writes_the_golden_files(ctx, line, tmp_path):
    paths = [str(tmp_path / T.out_name(line, i)) for i in range(len(line[3]))]
    tools.transform(T.command_line(line, T.fixture_path(line[1]), paths)[1:], ctx=ctx)
    _check_outputs(line, paths)


def test_the_command_line_in_a_process_of_its_own(tmp_path):
    """the KMC2 input ordered for a reduce, the plain dump next to it streamed in parts of 50 KB of text"""
    line = next(ln for ln in T.LINES if ln[0] == "k33raw_reduce_dump")
    paths = [str(tmp_path / T.out_name(line, i)) for i in range(len(line[3]))]
    r = subprocess.run([sys.executable, "-m", "kmc_amd.tools", *T.command_line(line, T.fixture_path(line[1]), paths)], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, KMC_HIP_DUMP_PART_MB="0.05"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    _check_outputs(line, paths)


@pytest.mark.parametrize("line", T.LIVE_LINES, ids=[ln[0] for ln in T.LIVE_LINES])
def test_the_command_line_against_a_live_kmc_tools(ctx, ref_bins, line, tmp_path):
    if ref_bins is None:
        pytest.skip("no reference binaries (oracle/_ref)")
    ours = [str(tmp_path / f"ours_{i}") for i in range(len(line[3]))]
    theirs = [str(tmp_path / f"theirs_{i}") for i in range(len(line[3]))]
    subprocess.run([ref_bins["kmc_tools"], "-t1", "-hp", *T.command_line(line, T.fixture_path(line[1]), theirs)], check=True, capture_output=True, timeout=600)
    tools.transform(T.command_line(line, T.fixture_path(line[1]), ours)[1:], ctx=ctx)
    for i, (op, _) in enumerate(line[3]):
        for ext in ([""] if T.is_text(op) else [".kmc_pre", ".kmc_suf"]):
            want = open(theirs[i] + ext, "rb").read()
            assert len(want) > 8 and open(ours[i] + ext, "rb").read() == want, (line[0], i, ext)
