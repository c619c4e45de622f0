"""GPU: the reads of a file against an ordered k-mer database (kmc_hip_db_query_reads_device, `python -m kmc_amd.tools filter`) at the product tile geometry — the
planted cases of tests/query_cases.py for every record width, an invalid symbol at every offset around a tile seam, the golden command lines, one case of 2 M database
records and 4 M positions against numpy.searchsorted, and the command line against a live `kmc_tools filter` where oracle/_ref is present. Reads tests/golden and
oracle/_ref only."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import query_cases as Q
import setops_cases as S
from kmc_amd import tools

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEN = dict.fromkeys(Q.STATS, 0)  # the tallies over the whole planted list


@pytest.fixture()
def runner(ctx):
    r = Q.Runner(ctx)
    yield r
    r.close()


@pytest.mark.parametrize("k,p", Q.PLANTED, ids=Q.PLANTED_IDS)
def test_device_call_on_planted_cases(runner, k, p):
    """SIZE 1 (k = 27, 32), 2 (33, 64), 3 (65), 4 (127), 5 (129), 7 (224); at k = 33 and 65 a LUT prefix across a 64-bit word of the k-mer and one inside a word"""
    cases = Q.planted_cases(k, p, Q.product_tile(k))
    assert len(cases) == (9 if k % 2 == 0 else 8)
    for case in cases:
        st = Q.check_case(runner, case)
        for key in SEEN:
            SEEN[key] += st[key]


def test_the_planted_list_exercised_every_tally():
    assert all(v > 0 for v in SEEN.values()), SEEN


@pytest.mark.parametrize("k,p", Q.PLANTED, ids=Q.PLANTED_IDS)
def test_an_invalid_symbol_at_every_offset_around_a_seam(runner, k, p):
    tile = Q.product_tile(k)
    case, shifted = Q.shifted_invalid(k, p, tile)
    runner.set_db(k, p, case["cb"], case["db"], case["cut"])
    base, st0 = Q.restate_counters(case["seq"], k, True, case["db"], *case["cut"])
    assert st0["n_invalid_windows"] == k + 1 and np.count_nonzero(base) == base.size - 2 * k
    for d in range(2 * k + 1):
        seq, off = shifted(d)
        got, n_valid, _, _, st = runner.run(k, True, seq, off, 1, want=("counters", "n_valid"))
        want = np.concatenate([np.zeros(d, dtype=np.uint32), base])
        assert np.array_equal(got, want), (d, np.flatnonzero(got != want)[:8])
        assert st == dict(st0, n_invalid_windows=st0["n_invalid_windows"] + d) and n_valid[-1] == np.count_nonzero(base)


@pytest.mark.parametrize("line", Q.LINES, ids=Q.LINE_IDS)
def test_the_golden_command_lines(ctx, line, tmp_path):
    out = str(tmp_path / "out")
    st = tools.filter_reads(Q.command_line(line, out)[1:], ctx=ctx)
    assert open(out, "rb").read() == Q.golden_out(line[0])
    assert st["n_reads"] == 200 and st["n_found"] > 0


def test_the_command_line_in_a_process_of_its_own(tmp_path):
    line = next(ln for ln in Q.LINES if ln[0] == "k33_mask_raw")  # the KMC2 database: ordered on the device first
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, "-m", "kmc_amd.tools", *Q.command_line(line, out)], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, KMC_HIP_FILTER_PART_MB="0.02"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    assert open(out, "rb").read() == Q.golden_out(line[0])


def _rev2(x):
    """the 32 two-bit symbols of every uint64 in reverse order"""
    for sh, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        x = ((x >> np.uint64(sh)) & np.uint64(m)) | ((x & np.uint64(m)) << np.uint64(sh))
    return (x >> np.uint64(32)) | (x << np.uint64(32))


def test_two_million_records_and_four_million_positions(runner):
    """k = 27, lut_prefix_len 7: 26 667 reads of 150 symbols against 2 M canonical k-mers, about half of the windows found; counters, tallies, n_valid and trim_len
    against numpy.searchsorted"""
    k, p, read_len = 27, 7, 150
    rng = np.random.default_rng(17)
    n_reads = 4_000_000 // (read_len + 1) + 1
    text = Q.BASES[rng.integers(0, 4, size=(n_reads, read_len + 1))]
    text[:, -1] = ord("\n")
    text[rng.integers(0, n_reads, size=300), rng.integers(0, read_len, size=300)] = ord("N")
    seq = text.reshape(-1)
    off = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len + 1)
    codes = Q.CODE[seq]
    n_win = seq.size - k + 1
    fw = np.zeros(n_win, dtype=np.uint64)
    for j in range(k):
        fw |= (codes[j:j + n_win] & 3).astype(np.uint64) << np.uint64(2 * (k - 1 - j))
    rc = _rev2(~fw) >> np.uint64(64 - 2 * k)
    q = np.minimum(fw, rc)
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    valid = (bad[k:] - bad[:-k]) == 0
    pool = np.unique(q[valid])
    dbk = np.unique(np.concatenate([pool[rng.permutation(pool.size)[:pool.size // 2]], rng.integers(0, 1 << 54, size=1_200_000, dtype=np.uint64)]))[:2_000_000]
    assert dbk.size == 2_000_000
    cnt = rng.integers(1, 256, size=dbk.size).astype(np.uint8)
    sbits = 2 * (k - p)
    suf = (dbk & np.uint64((1 << sbits) - 1)).astype(">u8").view(np.uint8).reshape(-1, 8)[:, 8 - sbits // 8:]
    recs = np.ascontiguousarray(np.concatenate([suf, cnt[:, None]], axis=1).reshape(-1))
    lut = np.searchsorted(dbk >> np.uint64(sbits), np.arange(1 << (2 * p), dtype=np.uint64), side="left").astype(np.uint64)
    ci, cx = 3, 250
    at = np.minimum(np.searchsorted(dbk, q), dbk.size - 1)
    hit = valid & (dbk[at] == q)
    c = cnt[at].astype(np.uint32)
    inside = hit & (c >= ci) & (c <= cx)
    want = np.zeros(seq.size, dtype=np.uint32)
    want[:n_win][inside] = c[inside]
    from kmc_amd import capi

    allocs = [runner.ctx.malloc(recs.nbytes + 256), runner.ctx.malloc(lut.nbytes)]
    try:
        runner.ctx.h2d(allocs[0], recs)
        runner.ctx.h2d(allocs[1], lut)
        runner.view = capi.DbView(allocs[0], dbk.size, allocs[1], p, 1, ci, cx)
        got, n_valid, trim, _, st = runner.run(k, True, seq, off, 40, want=("counters", "n_valid", "trim_len"))
    finally:
        for d in allocs:
            runner.ctx.free(d)
    assert st == dict(n_valid_windows=int(valid.sum()), n_found=int(inside.sum()), n_cut=int((hit & ~inside).sum()), n_invalid_windows=int((~valid).sum()))
    assert 0.3 < st["n_found"] / st["n_valid_windows"] < 0.6 and st["n_cut"] > 10_000
    assert np.array_equal(got, want)
    per_read = want.reshape(n_reads, read_len + 1)[:, :read_len - k + 1]
    assert np.array_equal(n_valid, np.count_nonzero(per_read, axis=1))
    low = per_read < 40
    later = np.where(low[:, 1:].any(axis=1), low[:, 1:].argmax(axis=1) + 1, read_len - k + 1)
    assert np.array_equal(trim, np.where(low[:, 0], 0, k - 1 + later))
    assert np.count_nonzero(trim) > 1000


def test_the_command_line_against_a_live_kmc_tools(ctx, ref_bins, tmp_path):
    if ref_bins is None:
        pytest.skip("oracle/_ref not shipped")
    a, fq = S.golden_path(27, "a"), str(tmp_path / "reads.fq")
    with open(fq, "wb") as f:
        f.write(gzip.open(os.path.join(Q.GOLDEN, Q.FQ_LONG), "rb").read())
    for i, args in enumerate((["-hm", a, "-ci2", "-cx9", fq, "-ci4"], [a, fq, "-ci0.25", "-cx0.75"], ["-t", a, fq, "-ci2"])):
        ref, got = str(tmp_path / f"ref{i}"), str(tmp_path / f"got{i}")
        subprocess.run([ref_bins["kmc_tools"], "-t1", "-hp", "filter", *args, ref, "-fa"], check=True, capture_output=True)
        tools.filter_reads([*args, got, "-fa"], ctx=ctx)
        data = open(got, "rb").read()
        assert data == open(ref, "rb").read() and len(data) > 1000, i
