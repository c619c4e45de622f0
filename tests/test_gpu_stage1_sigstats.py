"""-m gpu: stage 0 on the device. The per-part cases of tests/test_stage1_sigstats_emulated.py on libkmc_hip.so (k_s1_sig_stats on gfx950, in the product's
geometry: the cases are sized from the product's tile), two 8 MB parts, the planted-balance count, then kmc_hip_s1 against the reference's kmc: the .kmc_pre of a
KMC2 database holds the signature map, so byte-identical files hold the device's statistics to the reference's through the reference's own CSignatureMapper::Init."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import count_cases as CC
import oracle_s1 as S1
import sigstats_cases as SC
from kmc_amd import build as B
from kmc_amd import capi, synth, tools
from sigstats_cases import EINVAL, KM, KM_IDS, UNCOVERED, SigStatsLib, check_part
from test_stage1_hc_emulated import _rnd, getseq_returns
from test_stage1_multiline_emulated import _wrap

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE_CAP = 1 << 17
REPORT = r"\[kmc_hip stage 0\] worker: signature statistics on the device: (\d+) parts, (\d+) k-mers"


@pytest.fixture(scope="module")
def T():
    return SC.tile_constants("product")["tile"]


@pytest.fixture(scope="module")
def lib():
    L = SigStatsLib(os.environ.get("KMC_HIP_LIB") or B.LIB_HIP)
    yield L
    L.close()


def test_the_library_says_it_computes_the_statistics_and_keeps_its_contract(lib):
    L = lib.L
    assert L.kmc_hip_abi_version() == 4
    assert L.kmc_hip_split_covers(capi.SPLIT_COVERS_SIGSTATS) == 1 and [L.kmc_hip_split_covers(t) for t in (0x106, 0x108)] == [0, 0]
    assert lib.close_table() == 0 and lib.close_table() == 0
    text = b">t\nACGTACGTTGCATGCATTGACCAGTAGGATCCAGT\n"
    assert lib.part(text, 27, 9, 0, LINE_CAP)[0] == EINVAL  # none open
    for k, m in ((27, 4), (27, 12), (8, 9), (257, 9)):
        assert lib.open(k, m) == EINVAL
    assert lib.open(27, 9) == 0 and lib.open(27, 9) == 0 and lib.open(27, 7) == EINVAL and lib.open(28, 9) == EINVAL
    for bad in (dict(flags=4), dict(flags=2), dict(file_type=3), dict(k=28), dict(m=7), dict(line_cap=100)):
        kw = dict(dict(k=27, m=9, file_type=0, line_cap=LINE_CAP, flags=0), **bad)
        assert lib.part(text, kw["k"], kw["m"], kw["file_type"], kw["line_cap"], 0, kw["flags"])[0] == EINVAL, bad
    assert lib.part(b">a\nACGTACG\n\n>b\nACGTACGT\n", 27, 9, 0, LINE_CAP)[0] == UNCOVERED
    assert not lib.read_all(9).any()
    assert lib.L.kmc_hip_sigstats_read(lib.h, 0, 4**9, 2, None) == EINVAL
    lib.close_table()


@pytest.mark.parametrize("k,m", KM, ids=KM_IDS)
def test_part_sizes_around_k_and_around_the_tile(lib, T, k, m):
    for name, text, ft in SC.size_cases(T, k):
        want, _ = check_part(lib, text, ft, k, m, LINE_CAP)
        if name.startswith("pos_"):
            assert int(want.sum()) == {"pos_T-1": T - 1, "pos_T": T, "pos_T+1": T + 1, "pos_3T+5": 3 * T + 5}[name]


def test_an_invalid_code_at_every_offset_around_a_tile_seam(lib, T):
    k, m = 27, 9
    for d in range(-k, k + 1):
        want, returns = check_part(lib, SC.seam_n_text(T, k, d), 0, k, m, LINE_CAP)
        assert int(want.sum()) == (T + 2 * k + 5) - k + 1 - k and returns[0][T + d] < 0, d


@pytest.mark.parametrize("k,m", [(27, 9), (12, 11), (28, 7), (255, 5)], ids=["k27-m9", "k12-m11", "k28-m7", "k255-m5"])
def test_homopolymers_satellites_and_both_table_placements(lib, T, k, m, monkeypatch):
    for name, text, ft in SC.repeat_cases(T, k):
        want, _ = check_part(lib, text, ft, k, m, LINE_CAP)
        if name == "poly_A":
            assert int(want[4**m]) >= max(3 * T, 2 * k) - k + 1
        for env in (dict(KMC_HIP_S1_SIGSTATS_LDS_M="7"), dict(KMC_HIP_S1_SIGSTATS_LDS_M="7", KMC_HIP_S1_SIGSTATS_WGS="2"), dict(KMC_HIP_S1_SIGSTATS_LDS_M="0", KMC_HIP_S1_SIGSTATS_WGS="1")):
            for var in ("KMC_HIP_S1_SIGSTATS_LDS_M", "KMC_HIP_S1_SIGSTATS_WGS"):
                monkeypatch.delenv(var, raising=False)
            for var, v in env.items():
                monkeypatch.setenv(var, v)
            check_part(lib, text, ft, k, m, LINE_CAP, want=want)
        for var in ("KMC_HIP_S1_SIGSTATS_LDS_M", "KMC_HIP_S1_SIGSTATS_WGS"):
            monkeypatch.delenv(var, raising=False)


@pytest.mark.parametrize("k,m", [(27, 9), (55, 9), (12, 11)], ids=["k27-m9", "k55-m9", "k12-m11"])
def test_formats_part_kinds_and_homopolymer_compression(lib, T, k, m):
    names = []
    for name, text, ft, line_cap, long_read, returns in SC.format_cases(T, k):
        for hc in (False, True):
            check_part(lib, text, ft, k, m, line_cap, long_read, hc, returns)
        names.append(name)
    assert {"fastq", "fastq_crlf", "fasta_crlf_no_final_eol", "pieces", "long_titled", "long_untitled", "multiline_0", "multiline_1", "bam"} <= set(names)


def test_the_statistics_of_a_bins_signatures_are_the_bins_kmers(lib):
    from test_stage1_emulated import _records_text, _sig_map

    k, m, n_bins = 27, 9, 37
    rng = np.random.default_rng(21)
    text = _records_text("fq", b"\n", [_rnd(rng, int(n), b"ACGTacgtN" if i % 5 == 0 else b"ACGT") for i, n in enumerate(rng.integers(20, 400, size=600))] + [b"A" * 3000, b"AC" * 2000])
    smap = _sig_map(m, n_bins, 5)
    for flags in (0, capi.SPLIT_HOMOPOLYMER):
        rc, got = lib.split(text, k, m, n_bins, smap, LINE_CAP, 1, flags=flags)
        assert rc == 0, got
        lib.reopen(k, m)
        rc, n_reads, n_kmers = lib.part(text, k, m, 1, LINE_CAP, flags=flags)
        assert rc == 0 and n_reads == got["n_reads"] and n_kmers == int(got["kmers"].sum())
        stats = lib.read_all(m)
        per_bin = np.zeros(n_bins, dtype=np.uint64)
        np.add.at(per_bin, smap[stats > 0].astype(np.int64), stats[stats > 0].astype(np.uint64))
        assert np.array_equal(per_bin, got["kmers"])
    lib.close_table()


@pytest.mark.parametrize("poly_a", [False, True], ids=["random", "poly_A_1Mbp"])
def test_large_part_on_the_device(lib, poly_a):
    """one 8 MB part (more tiles than persistent workgroups): random reads; and the same with a 1 Mbp record of A inside (every window on the special entry)"""
    k, m = 27, 9
    rng = np.random.default_rng(17)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    recs = [acgt[rng.integers(0, 4, size=int(n))].tobytes() for n in rng.integers(1000, 150_000, size=100)]
    if poly_a:
        recs[40:60] = [b"A" * 1_000_000]
    text = b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(recs))
    assert 6_000_000 < len(text) < 10_000_000
    returns, n_reads = getseq_returns(text, 0, k, 1 << 20)
    want = SC.stats_from_superkmers(returns, k, m)
    lib.reopen(k, m)
    rc, got_reads, got_kmers = lib.part(text, k, m, 0, 1 << 20)
    assert rc == 0, lib.L.kmc_hip_last_error(lib.h)
    got = lib.read_all(m)
    lib.close_table()
    assert (got_reads, got_kmers) == (n_reads, int(want.sum(dtype=np.uint64))) and np.array_equal(got, want)
    if poly_a:
        assert int(want[4**m]) >= 1_000_000 - k + 1


def test_count_with_the_map_from_the_statistics_balances_the_planted_input(tmp_path):
    k, m, n_bins = 27, 5, 64
    text, (s1, s2) = SC.planted_input(k, m, n_bins)
    path = str(tmp_path / "planted.fa")
    with open(path, "wb") as f:
        f.write(text)
    stats = SC.oracle_stats(getseq_returns(text, 0, k, capi.SPLIT_LINE_CAP)[0], k, m)
    L = S1.lib()
    allowed = np.array([bool(L.oracle_s1_is_allowed(x, m)) for x in range(4**m)] + [False])
    fixed, balanced = tools.count_signature_map(m, n_bins), tools.balanced_signature_map(stats, m, n_bins, allowed)
    want = dict(fixed=SC.balance_of(stats, fixed, n_bins), stats=SC.balance_of(stats, balanced, n_bins))
    assert fixed[s1] == fixed[s2] and want["stats"] < want["fixed"]
    ctx = capi.Context((0,))
    try:
        res, body = {}, {}
        for which in ("fixed", "stats"):
            out = str(tmp_path / which)
            res[which] = tools.count([f"-k{k}", "-ci1", "-fa", f"-p{m}", f"-n{n_bins}", path, out], ctx=ctx, part_bytes=1 << 20, signature_map=which)
            body[which] = CC.database_bytes(out)
            assert res[which]["map"] == which and res[which]["n_parts"] == 1 and res[which]["balance"] == want[which], (which, res[which]["balance"], want[which])
        assert body["fixed"] == body["stats"] and res["stats"]["balance"] < res["fixed"]["balance"]
        few = tools.count([f"-k{k}", "-ci1", "-fa", "-n8", path, str(tmp_path / "few")], ctx=ctx, part_bytes=1 << 20, signature_map="stats")
        assert few["map"] == "fixed" and CC.database_bytes(str(tmp_path / "few")) == body["fixed"]
    finally:
        ctx.close()


# ---- kmc_hip_s1 against kmc
def _exe(name):
    return os.path.join(ROOT, "kmc_amd", "bin", name) if name.startswith("kmc_hip") else os.path.join(ROOT, "oracle", "_ref", name)


def _require_binaries():
    missing = [n for n in ("kmc", "kmc_hip_s1") if not os.path.exists(_exe(n))]
    if missing:
        pytest.skip("needs the reference pipeline binaries (%s not built: the reference source tree was absent at build time)" % ", ".join(missing))


_state = {"broken": False}  # one failed or hung run is enough: the other parameter sets do not spend GPU time on the same problem
_IN = {}


def _input(tmp_path_factory, fmt):
    if fmt not in _IN:
        p = str(tmp_path_factory.mktemp("sigstats") / ("reads." + fmt))
        if fmt == "ml":
            synth.make_multiline_fasta(p, seed=7, contig_lens=[600_000, 0, 250_000, 900, 400_000], line_width=60, lower_frac=0.2)
        else:
            synth.make_fastq(p, seed=31, genome_len=2_000_000, n_reads=300_000, read_len=150)  # the input of tests/test_gpu_stage1_e2e.py
        _IN[fmt] = p
    return _IN[fmt]


def _run(exe, flags, inp, tmp_path, tag, env=None):
    t = tmp_path / ("tmp_" + tag)
    t.mkdir(exist_ok=True)
    db = str(tmp_path / ("db_" + tag))
    e = dict(os.environ, KMC_HIP_LIB=os.environ.get("KMC_HIP_LIB") or B.LIB_HIP, **(env or {}))
    try:
        r = subprocess.run([_exe(exe), *flags, inp, db, str(t)], capture_output=True, text=True, env=e, timeout=120)
    except subprocess.TimeoutExpired:
        _state["broken"] = True
        raise
    if r.returncode != 0:
        _state["broken"] = True
    assert r.returncode == 0, (exe, flags, (r.stdout + r.stderr)[-1500:])
    files = [db + x for x in (".kmc_pre", ".kmc_suf") if os.path.exists(db + x)]
    md5 = tuple(hashlib.md5(open(f, "rb").read()).hexdigest() for f in files)
    stats = [ln.split(":")[1].strip() for ln in r.stdout.splitlines() if "No. of" in ln or "Total no." in ln]
    return md5, stats, r.stdout + r.stderr


@pytest.mark.parametrize("flags,fmt", [(["-k27", "-ci1"], "fq"), (["-k27", "-hc"], "fq"), (["-k55", "-p7"], "fq"), (["-k27", "-fm"], "ml")], ids=["k27", "k27hc", "k55p7", "k27fm"])
def test_kmc_hip_s1_with_stage_0_on_the_device_writes_the_reference_database(flags, fmt, tmp_path, tmp_path_factory):
    _require_binaries()
    if _state["broken"]:
        pytest.fail("an earlier run of kmc_hip_s1 failed or hung")
    inp = _input(tmp_path_factory, fmt)
    want = _run("kmc", flags + ["-m4", "-sf1", "-sp1", "-sr1"], inp, tmp_path, "ref")
    got = _run("kmc_hip_s1", flags + ["-m4", "-sf2", "-sp4", "-sr4"], inp, tmp_path, "hip", env={"KMC_HIP_VERBOSE": "1"})
    assert len(want[0]) == 2 and got[:2] == want[:2]  # .kmc_pre (with the signature map) and .kmc_suf, byte for byte; the statistics lines
    rep = re.findall(REPORT, got[2])
    assert rep and sum(int(p) for p, _ in rep) > 0 and sum(int(n) for _, n in rep) > 0, got[2][-2000:]


def test_small_k_builds_no_map_and_never_constructs_the_stage_0_worker(tmp_path, tmp_path_factory):
    _require_binaries()
    if _state["broken"]:
        pytest.fail("an earlier run of kmc_hip_s1 failed or hung")
    got = _run("kmc_hip_s1", ["-k9", "-fm", "-m4", "-sf1", "-sp2", "-sr2"], _input(tmp_path_factory, "ml"), tmp_path, "k9", env={"KMC_HIP_VERBOSE": "1"})
    assert "small k on the device" in got[2] and not re.findall(REPORT, got[2]) and "stage 0" not in got[2]
