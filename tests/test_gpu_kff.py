"""GPU: KFF files read as database bodies (kmc_hip_kff_import_device, the KFF inputs of `python -m kmc_amd.tools`) at the product tile geometry — the planted and the
corruption cases of tests/test_kff_emulated.py, the recorded command lines, one body of 2 M k-mers against numpy as one section and as 512, a round trip of a KMC body
through the restatement's KFF records, and the command line against a live `kmc_tools` where oracle/_ref is present. Reads tests/golden and oracle/_ref only."""
import os
import subprocess

import numpy as np
import pytest

import kff_cases as K
import setops_cases as S
import transform_cases as T
from kmc_amd import capi, dbio, tools

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"simple": tools.simple, "transform": tools.transform, "complex": tools.complex, "filter": tools.filter_reads}


@pytest.mark.parametrize("k,p", K.WIDTHS, ids=K.WIDTH_IDS)
def test_planted_sections(ctx, k, p):
    """3 1/3 product tiles of data_size 1 (the seam cases sit on its tile seams exactly); every case with ordered = 0 and ordered = 1"""
    for name, cs, sections in K.planted_cases(k, p, K.tile_records(k, p, 1)):
        for ordered in (False, True):
            try:
                K.check_import(ctx, k, cs, p, sections, ordered)
            except AssertionError as e:
                raise AssertionError(f"{name}, ordered {ordered}: {e}")


def test_every_address_residue(ctx):
    k, p, cs = 27, 3, 1
    tile = K.tile_records(k, p, cs)
    kmers = S.random_kmers(np.random.default_rng(4), k, 2 * tile + 37)
    sections = K.split(kmers, K.edge_counts(cs, len(kmers)), [tile + 3])
    data = b"".join(K.encode_records(k, cs, ks, cc) for ks, cc in sections)
    want = K.restate_import(k, cs, p, sections, False)
    for off in range(16):
        lut, recs = K.run_import(ctx, k, cs, p, data, [len(ks) for ks, _ in sections], False, in_off=off, out_off=(5 * off + 3) % 16)
        assert np.array_equal(lut, want[0]) and np.array_equal(recs, want[1]), off


@pytest.mark.parametrize("k,p", [(27, 3), (33, 5), (64, 4), (129, 5)])
def test_corrupt_sections_are_named(ctx, k, p):
    rb = (k + 3) // 4 + 1
    for name, secs, bad0, bad1, where in K.corruption_cases(k, p, K.tile_records(k, p, 1)):
        sec_n = [len(s) // rb for s in secs]
        for ordered, bad in ((False, bad0), (True, bad1)):
            if not bad:
                K.run_import(ctx, k, 1, p, b"".join(secs), sec_n, ordered)
                continue
            with pytest.raises(capi.KmcHipError) as e:
                K.run_import(ctx, k, 1, p, b"".join(secs), sec_n, ordered)
            assert e.value.code == K.ECORRUPT and "KFF" in str(e.value), (name, ordered, str(e.value))
            if where is not None:
                sec = 0 if where < sec_n[0] else 1
                assert f"KFF record {where} (record {where - sec * sec_n[0]} of section {sec})" in str(e.value), (name, ordered, str(e.value))
    K.check_import(ctx, k, 1, p, [([1, 2, 3], [4, 5, 6])], True)


def test_the_unordered_body_through_dump_and_histogram(ctx):
    k, p = 33, 5
    segments, kmers, counts = T.segmented_case(k, p, K.tile_records(k, p, 1))
    data = b"".join(K.encode_records(k, 1, ks, cc) for ks, cc in segments)
    lut, recs, body = K.run_import(ctx, k, 1, p, data, [len(ks) for ks, _ in segments], False, keep=True)
    try:
        T.check_dump(ctx, body, kmers, counts, (5, 150), 20, 120, 99)
        T.check_histogram(ctx, body, counts, (5, 150), 20, 120)
    finally:
        body.free()


@pytest.mark.parametrize("line", K.LINES, ids=K.LINE_IDS)
def test_the_command_line_writes_the_recorded_files(ctx, line, tmp_path):
    argv, outs = K.command_line(line, str(tmp_path))
    MODES[argv[0]](argv[1:], ctx=ctx)
    for i, (path, kind) in enumerate(zip(outs, line[3])):
        assert K.output_bytes(path, kind) == K.read_golden(line, i, kind), (line[0], i)


@pytest.fixture(scope="module")
def big():
    """2 M distinct k-mers at k = 27 with two counter bytes, ascending, and what their body is for the prefix length of that size — numpy only, computed once"""
    k, cs, n = 27, 2, 2_000_000
    rng = np.random.default_rng(27)
    keys = np.unique(rng.integers(0, 1 << 54, size=n + n // 50, dtype=np.uint64))[:n]
    assert keys.size == n
    counts = rng.integers(1, 1 << 16, size=n, dtype=np.uint64).astype(np.uint16)
    key_be = keys.astype(">u8").view(np.uint8).reshape(n, 8)
    kff = np.concatenate([key_be[:, 1:], counts.astype(">u2").view(np.uint8).reshape(n, 2)], axis=1)  # 7 k-mer bytes, 2 counter bytes, most significant first

    def body(order, p):
        sb = (k - p) // 4
        recs = np.concatenate([key_be[order, 8 - sb:], counts[order].astype("<u2").view(np.uint8).reshape(n, 2)], axis=1)
        return recs.reshape(-1), (keys[order] >> np.uint64(2 * (k - p)))

    return dict(k=k, cs=cs, n=n, keys=keys, kff=kff, body=body)


def _import(ctx, big, data, sec_n, ordered, p):
    k, cs, n = big["k"], big["cs"], big["n"]
    rb = (k - p) // 4 + cs
    lut_n = (1 << (2 * p)) if ordered else (len(sec_n) << (2 * p)) + 1
    d = [ctx.malloc(data.size + 256), ctx.malloc(n * rb + 256), ctx.malloc(8 * lut_n)]
    try:
        ctx.h2d(d[0], np.ascontiguousarray(data))
        assert ctx.kff_import_device(k, cs, d[0], sec_n, ordered, p, d[1], n * rb, d[2]) == n
        recs, lut = np.zeros(n * rb, dtype=np.uint8), np.zeros(lut_n, dtype=np.uint64)
        ctx.d2h(recs, d[1])
        ctx.d2h(lut, d[2])
        return lut, recs
    finally:
        for x in d:
            ctx.free(x)


def test_two_million_kmers_as_one_section_and_as_512(ctx, big):
    k, n = big["k"], big["n"]
    p = dbio.best_lut_prefix_len(k, n)
    ident = np.arange(n)
    want_recs, prefixes = big["body"](ident, p)
    want_lut = np.searchsorted(prefixes, np.arange(1 << (2 * p), dtype=np.uint64), side="left").astype(np.uint64)
    lut, recs = _import(ctx, big, big["kff"].reshape(-1), [n], True, p)
    assert np.array_equal(recs, want_recs) and np.array_equal(lut, want_lut)
    # dealt into 512 sections at random, each ascending; sections 100 and 511 empty
    sec = np.random.default_rng(5).integers(0, 510, size=n)
    sec[sec >= 100] += 1
    order = np.argsort(sec, kind="stable")
    sec_n = np.bincount(sec, minlength=512).tolist()
    assert sec_n[100] == 0 and sec_n[511] == 0 and len(sec_n) == 512
    data = big["kff"][order].reshape(-1)
    lut, recs = _import(ctx, big, data, sec_n, True, p)
    assert np.array_equal(recs, want_recs) and np.array_equal(lut, want_lut)
    # the file's order under the segmented LUT, smallest valid prefix length
    p0 = K.smallest_p(k)
    want_recs0, prefixes0 = big["body"](order, p0)
    starts = np.concatenate([[0], np.cumsum(sec_n)]).astype(np.int64)
    want_lut0 = np.concatenate([starts[s] + np.searchsorted(prefixes0[starts[s]:starts[s + 1]], np.arange(1 << (2 * p0), dtype=np.uint64), side="left") for s in range(512)] + [[n]]).astype(np.uint64)
    lut, recs = _import(ctx, big, data, sec_n, False, p0)
    assert np.array_equal(recs, want_recs0) and np.array_equal(lut, want_lut0)


def test_a_kmc_body_through_kff_records_and_back(ctx):
    """the round trip: a KMC1 body decoded, encoded as KFF records by the restatement and imported must be the original bytes"""
    for k in (27, 33, 55):
        db = dbio.read_database(S.golden_path(k, "a"))
        kmers, counts = S.decode_body(k, db.lut_prefix_len, db.counter_size, db.lut, db.recs)
        lut, recs = K.run_import(ctx, k, db.counter_size, db.lut_prefix_len, K.encode_records(k, db.counter_size, kmers, counts), [len(kmers)], True)
        assert np.array_equal(recs, db.recs) and np.array_equal(lut, db.lut)
        raw = dbio.read_kff(K.kff_file(f"kff_k{k}_a"))  # and the reference's own KFF twin of that database
        lut, recs = K.run_import(ctx, k, raw.counter_size, db.lut_prefix_len, raw.records().tobytes(), [n for _, n in raw.sections], True)
        assert np.array_equal(recs, db.recs) and np.array_equal(lut, db.lut)


@pytest.mark.parametrize("name", K.LIVE_LINES)
def test_the_command_line_against_a_live_kmc_tools(ctx, ref_bins, name, tmp_path):
    if ref_bins is None:
        pytest.skip("no reference binaries (oracle/_ref)")
    line = {ln[0]: ln for ln in K.LINES}[name]
    (tmp_path / "ours").mkdir()
    (tmp_path / "theirs").mkdir()
    argv, theirs = K.command_line(line, str(tmp_path / "theirs"))
    subprocess.run([ref_bins["kmc_tools"], "-t1", "-hp", *argv], check=True, capture_output=True, timeout=600)
    argv, ours = K.command_line(line, str(tmp_path / "ours"))
    MODES[argv[0]](argv[1:], ctx=ctx)
    for a, b, kind in zip(ours, theirs, line[3]):
        assert K.output_bytes(a, kind) == K.output_bytes(b, kind), name
