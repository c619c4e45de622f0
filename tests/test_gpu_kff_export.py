"""GPU: KFF output (kmc_hip_db_kff_export_device, `python -m kmc_amd.tools export`, `count` with output_format="kff") at the product tile geometry and at tiles of 256
records — the planted bodies and round trips of tests/test_kff_export_emulated.py, the recorded reference files through `export` in-process, 2 M random k-mers at k = 27
and k = 127 against the record restated in numpy, as one segment and as 512, and `export` against a live `kmc_tools` where oracle/_ref is present. Reads tests/golden and
oracle/_ref only."""
import os
import subprocess

import numpy as np
import pytest

import kff_cases as K
import kffout_cases as X
import setops_cases as S
from kmc_amd import capi, dbio, tools

pytestmark = pytest.mark.gpu


def golden(name):
    with open(X.kff_file(name), "rb") as f:
        return f.read()


@pytest.mark.parametrize("ipt", [None, 1], ids=["default_tile", "ipt1"])
@pytest.mark.parametrize("k,p", X.WIDTHS, ids=X.WIDTH_IDS)
def test_planted_bodies_and_round_trips(ctx, monkeypatch, k, p, ipt):
    """3 1/3 tiles of data_size 1 (the seam cases sit on its tile seams exactly); every case as one ascending body and as a segmented body, with both round trips"""
    if ipt:
        monkeypatch.setenv("KMC_HIP_KFF_IPT", str(ipt))
    for name, cs, sections in X.planted_cases(k, p, X.tile_records(k, p, 1, ipt=ipt)):
        try:
            X.round_trips(ctx, k, p, cs, sections)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")


def test_five_records_under_the_widest_lut(ctx):
    k, p = X.WIDEST
    ks = S.random_kmers(np.random.default_rng(9), k, 5)
    lut, recs, kmers, counts = X.ordered_body(k, p, 3, [(ks, [1, 1 << 16, 65535, 65536, (1 << 24) - 1])])
    X.check_export(ctx, k, p, 3, lut, recs, kmers, counts)
    X.check_export(ctx, k, p, 3, lut, recs, kmers, counts, first=1, count=3)


def test_every_data_size_range_and_address_residue(ctx):
    k, p = 27, 3
    for cs in (1, 2, 3, 4):
        tile = X.tile_records(k, p, cs)
        kmers = S.random_kmers(np.random.default_rng(cs), k, 2 * tile + 37)
        lut, recs, kmers, counts = X.ordered_body(k, p, cs, [(kmers, K.edge_counts(cs, len(kmers)))])
        for ds in range(cs, 5):
            X.check_export(ctx, k, p, cs, lut, recs, kmers, counts, ds=ds)
        cuts = [0, tile + 17, 2 * tile - 200, len(kmers)]
        assert b"".join(X.check_export(ctx, k, p, cs, lut, recs, kmers, counts, first=a, count=b - a) for a, b in zip(cuts, cuts[1:])) == X.run_export(ctx, k, p, cs, lut, recs)
    for off in range(16):  # cs = 4 still: 10 bytes in, 11 out
        X.check_export(ctx, k, p, 4, lut, recs, kmers, counts, in_off=off, out_off=(5 * off + 3) % 16, first=off, count=len(kmers) - 2 * off)


def test_errors(ctx):
    k, p = 27, 3
    lut, recs, kmers, counts = X.ordered_body(k, p, 1, [([1, 2, 1 << 50], [1, 2, 3])])
    for kw, code in ((dict(ds=5), X.EINVAL), (dict(first=2, count=2), X.EINVAL), (dict(n_seg=0), X.EINVAL), (dict(capacity=23), X.ECAPACITY)):
        with pytest.raises(capi.KmcHipError) as e:
            X.run_export(ctx, k, p, 1, lut, recs, **kw)
        assert e.value.code == code and "kmc_hip_db_kff_export_device" in str(e.value)
    X.check_export(ctx, k, p, 1, lut, recs, kmers, counts)


@pytest.mark.parametrize("name", list(X.OLD_FILES) + list(X.FILES))
def test_export_writes_the_recorded_files(ctx, name, tmp_path):
    out = str(tmp_path / "o")
    tools.export(X.export_argv(name, out), ctx=ctx)
    assert open(out + ".kff", "rb").read() == golden(name)


def test_export_sections_reads_back_as_the_recorded_kmc2_line(ctx, tmp_path):
    src, out, again = os.path.join(X.GOLDEN, "setops_k33_raw_a"), str(tmp_path / "s"), str(tmp_path / "again")
    db = dbio.read_database(src)
    st = tools.export([src, out, "--sections"], ctx=ctx)
    f = dbio.read_kff(out + ".kff")
    assert [n for _, n in f.sections] == [recs.size // db.rec_bytes for recs, _ in db.bins if recs.size] and st["n_sections"] == len(f.sections) > 1
    tools.export([out + ".kff", again], ctx=ctx)
    assert open(again + ".kff", "rb").read() == golden("kffout_k33_raw")


def test_count_writes_the_recorded_file(ctx, tmp_path):
    fq = os.path.join(X.GOLDEN, "count_k27_fq.fq")
    as_kff, as_kmc, again = str(tmp_path / "kff"), str(tmp_path / "kmc"), str(tmp_path / "again")
    tools.count(X.COUNT_ARGV + [fq, as_kff], ctx=ctx, output_format="kff")
    assert open(as_kff + ".kff", "rb").read() == golden("kffout_k27_multi") and os.listdir(tmp_path) == ["kff.kff"]
    tools.count(X.COUNT_ARGV + [fq, as_kmc], ctx=ctx)
    tools.export([as_kmc, again], ctx=ctx)
    assert open(again + ".kff", "rb").read() == golden("kffout_k27_multi")


# ---- 2 M random k-mers against numpy
def _big(k, n=2_000_000, cs=2, seed=27):
    """n distinct ascending k-mers as big-endian bytes [n, ceil(k/4)] (the padding bits zero) and counters of cs bytes; numpy only"""
    rng = np.random.default_rng(seed + k)
    kb = (k + 3) // 4
    tb = min(kb, 8)  # the leading bytes are distinct and ascending, so the rows are; what follows them is random
    top = np.unique(rng.integers(0, 1 << (2 * k - 8 * (kb - tb)), size=n + n // 50, dtype=np.uint64))[:n]
    assert top.size == n and 2 * k - 8 * (kb - tb) < 64
    key = np.concatenate([top.astype(">u8").view(np.uint8).reshape(n, 8)[:, 8 - tb:], rng.integers(0, 256, size=(n, kb - tb), dtype=np.uint8)], axis=1)
    counts = rng.integers(1, 1 << (8 * cs), size=n, dtype=np.uint64)
    be = counts.astype(">u8").view(np.uint8).reshape(n, 8)[:, 8 - cs:]
    return key, be


def _prefixes(key, k, p):
    """the p-symbol prefix of every row: with (k - p) % 4 == 0 the value of its first ceil(p / 4) bytes"""
    kb = key.shape[1]
    pb = kb - (k - p) // 4
    x = np.zeros(key.shape[0], dtype=np.uint64)
    for q in range(pb):
        x = (x << np.uint64(8)) | key[:, q].astype(np.uint64)
    return x


def _check_big(ctx, k, n):
    cs = 2
    key, be = _big(k, n, cs)
    p = dbio.best_lut_prefix_len(k, n)
    sb = (k - p) // 4
    want = np.concatenate([key, be], axis=1)  # kff_cases.encode_records, vectorised: the k-mer bytes, the counter most significant byte first

    def body(order, q):
        return np.concatenate([key[order, key.shape[1] - (k - q) // 4:], be[order, ::-1]], axis=1).reshape(-1), _prefixes(key[order], k, q)

    recs, prefixes = body(np.arange(n), p)
    assert recs.size == n * (sb + cs)
    lut = np.searchsorted(prefixes, np.arange(1 << (2 * p), dtype=np.uint64), side="left").astype(np.uint64)
    got = X.run_export(ctx, k, p, cs, lut, recs)
    assert got == want.tobytes()
    assert X.run_export(ctx, k, p, cs, lut, recs, first=n // 3 + 1, count=n // 2, ds=4, in_off=5, out_off=9) == np.concatenate(
        [key, np.zeros((n, 2), dtype=np.uint8), be], axis=1)[n // 3 + 1:n // 3 + 1 + n // 2].tobytes()
    # dealt into 512 segments at random, each ascending; segments 100 and 511 empty; the smallest valid prefix length, as a KMC2 body has it
    sec = np.random.default_rng(5).integers(0, 510, size=n)
    sec[sec >= 100] += 1
    order = np.argsort(sec, kind="stable")
    sec_n = np.bincount(sec, minlength=512)
    assert sec_n[100] == 0 and sec_n[511] == 0 and sec_n.size == 512
    p0 = K.smallest_p(k)
    recs0, prefixes0 = body(order, p0)
    starts = np.concatenate([[0], np.cumsum(sec_n)]).astype(np.int64)
    lut0 = np.concatenate([starts[s] + np.searchsorted(prefixes0[starts[s]:starts[s + 1]], np.arange(1 << (2 * p0), dtype=np.uint64), side="left") for s in range(512)] + [[n]]).astype(np.uint64)
    assert X.run_export(ctx, k, p0, cs, lut0, recs0, n_seg=512) == want[order].tobytes()


@pytest.mark.parametrize("k", [27, 127])
def test_two_million_kmers_as_one_segment_and_as_512(ctx, k):
    _check_big(ctx, k, 2_000_000)


def test_export_against_a_live_kmc_tools(ctx, ref_bins, tmp_path):
    if ref_bins is None:
        pytest.skip("no reference binaries (oracle/_ref)")
    theirs, ours = str(tmp_path / "theirs"), str(tmp_path / "ours")
    src = os.path.join(X.GOLDEN, "setops_k33_raw_a")
    subprocess.run([ref_bins["kmc_tools"], "-t1", "-hp", "transform", src, "-ci2", "reduce", theirs, "-cx40", "-cs300", "-okff"], check=True, capture_output=True, timeout=600)
    tools.export([src, "-ci2", ours, "-cx40", "-cs300"], ctx=ctx)
    assert open(ours + ".kff", "rb").read() == open(theirs + ".kff", "rb").read()
