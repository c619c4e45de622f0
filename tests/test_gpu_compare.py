"""GPU: `kmc_tools compare`, `check` and `info` at the product tile geometry — the planted pairs of tests/test_compare_emulated.py (tiles of 2048 words, forwards and with
the tiles taken last to first), one pair of 2 M records at k = 27 against numpy, the recorded command lines in-process, and two of them against a live `kmc_tools`
where oracle/_ref is present. Reads tests/golden and oracle/_ref only."""
import contextlib
import io
import subprocess

import numpy as np
import pytest

import compare_cases as CC
import setops_cases as S
from kmc_amd import tools

pytestmark = pytest.mark.gpu
STEPS = 8  # the product's tile: 256 threads x 8 words


@pytest.mark.parametrize("k,p", CC.WIDTHS, ids=CC.WIDTH_IDS)
def test_planted_pairs(ctx, k, p):
    """three tiles and a third of 2048 words: 3 400 records of two words to 850 of eight; every case asserts all eight result words"""
    for name, a, b, kw in CC.planted_cases(k, p, STEPS, reduced=k not in (27, 65)):
        try:
            CC.check_case(ctx, k, a, b, **kw)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")


@pytest.mark.parametrize("k,p", [(33, 5), (127, 3)], ids=["33-p5", "127-p3"])
def test_the_smaller_of_two_differences_wins_with_the_tiles_reversed(ctx, monkeypatch, k, p):
    monkeypatch.setenv("KMC_HIP_COMPARE_REVERSED", "1")
    ran = 0
    for name, a, b, kw in CC.planted_cases(k, p, STEPS, reduced=True):
        if name.startswith(("two_", "both_", "a_short_and", "counter_at_seam", "cut_and_a", "uncut_differs")):
            try:
                CC.check_case(ctx, k, a, b, **kw)
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}")
            ran += 1
    assert ran > 10


def test_two_million_records_against_numpy(ctx):
    """k = 27, lut_prefix_len 3: equal bodies, one counter changed at a seeded record, and the same under cutoffs that remove every record counted once from both"""
    k, p, n = 27, 3, 2_000_000
    rng = np.random.default_rng(17)
    x = np.unique(rng.integers(0, 1 << 54, size=n + n // 8, dtype=np.uint64))[:n]
    assert x.size == n
    counts = rng.integers(1, 200, size=n).astype(np.uint8)
    recs = np.empty((n, 7), dtype=np.uint8)
    for q in range(6):
        recs[:, q] = (x >> np.uint64(8 * (5 - q))) & np.uint64(0xFF)
    recs[:, 6] = counts
    lut = np.searchsorted(x >> np.uint64(48), np.arange(64, dtype=np.uint64), side="left").astype(np.uint64)
    pos = int(rng.integers(n // 2, n))
    other = recs.copy()
    other[pos, 6] = counts[pos] % 199 + 1
    assert int(np.flatnonzero((recs != other).any(axis=1))[0]) == pos
    bodies = [(p, 1, lut, r.reshape(-1)) for r in (recs, other)]
    zero = dict.fromkeys(CC.RESULT, 0)
    assert CC.run_device(ctx, k, bodies[0], bodies[0]) == dict(zero, n_a=n, n_b=n)
    assert CC.run_device(ctx, k, bodies[0], bodies[1]) == dict(kind=1, ordinal=pos, n_a=n, n_b=n, counter_a=int(counts[pos]), counter_b=int(other[pos, 6]), record_a=pos, record_b=pos)
    # counters of 2 and more on both sides: the ordinal counts the present records in front, the record numbers stay
    kept = counts >= 2
    if not kept[pos] or other[pos, 6] < 2:
        pytest.fail("the seeded record is cut: choose another seed")
    m = int(kept.sum())
    assert CC.run_device(ctx, k, bodies[0], bodies[1], (2, 255), (2, 255)) == dict(kind=1, ordinal=int(kept[:pos].sum()), n_a=m, n_b=m, counter_a=int(counts[pos]),
                                                                                 counter_b=int(other[pos, 6]), record_a=pos, record_b=pos)
    assert CC.run_device(ctx, k, bodies[0], bodies[0], (2, 255), (2, 255)) == dict(zero, n_a=m, n_b=m)


def _in_process(argv, ctx):
    out, err = io.StringIO(), io.StringIO()
    status = 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            if argv[0] == "compare":
                res = tools.compare(argv[1:], ctx=ctx)
                out.write(tools.compare_report(res))
                status = 0 if res["kind"] == "equal" else 1
            elif argv[0] == "check":
                out.write(tools.check(argv[1:], ctx=ctx))
            else:
                o, e = tools.info(argv[1:])
                out.write(o)
                err.write(e)
        except SystemExit as e:
            err.write(f"{e.code}\n")
            status = 1
    return dict(stdout=out.getvalue(), stderr=err.getvalue(), status=status)


@pytest.mark.parametrize("line", CC.LINES, ids=CC.LINE_IDS)
def test_the_command_line_prints_the_recorded_lines(ctx, line):
    assert _in_process(CC.argv_of(line), ctx) == CC.read_golden(line)


def test_check_kmers(ctx):
    a = S.golden_path(27, "a")
    got = tools.check_kmers(a, ["AAAAAAGGGATCCTCGCAGGTCGCAAA", "AAAAAAGGGATCCTCGCAGGTCGCAAC", "AAAAAACCTGACTCGCGTTTCTCTGCG", "TTTCGTACGAACAATCTTGACGGCAAA", CC.RC_ONLY_27,
                                "aaaaaaGGGATCCTCGCAGGTcgcaaa"], ctx=ctx)
    assert got.dtype == np.uint32 and got.tolist() == [4, 0, 3, 11, 0, 4]
    assert tools.check_kmers(a, ["AAAAAAGGGATCCTCGCAGGTCGCAAA"], cx=4, ctx=ctx).tolist() == [0]  # equal to cutoff_max


@pytest.mark.parametrize("name", CC.LIVE_LINES)
def test_the_command_line_against_a_live_kmc_tools(ctx, ref_bins, name):
    if ref_bins is None:
        pytest.skip("no reference binaries (oracle/_ref)")
    argv = CC.argv_of({ln[0]: ln for ln in CC.LINES}[name])
    r = subprocess.run([ref_bins["kmc_tools"], "-t1", "-hp", *argv], capture_output=True, text=True, timeout=600)
    assert _in_process(argv, ctx) == dict(stdout=r.stdout, stderr=r.stderr, status=r.returncode)
