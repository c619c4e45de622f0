"""CPU: stage 0 on the device — kmc_hip_sigstats_open / _part / _read / _close (k_s1_sig_stats behind the front half of kmc_amd/csrc/stage1_chain.h) in the
PRODUCT'S host library compiled over the emulated HIP runtime (tests/emu.py build_hostlib, small geometry), the map tools.balanced_signature_map builds from
the statistics, and `python -m kmc_amd.tools count` with it.

The oracles are in tests/sigstats_cases.py: the existing stage-1 oracle's super-k-mers summed per signature, and the reference's CalcStats loop restated; both are
asked, and must agree, before the device is. Tables are compared exactly. The -m gpu file runs the same cases on the device in the product's geometry."""
import os
import threading

import numpy as np
import pytest

import count_cases as CC
import emu
import oracle_s1 as S1
import sigstats_cases as SC
from kmc_amd import capi, tools
from sigstats_cases import EINVAL, KM, KM_IDS, UNCOVERED, SigStatsLib, check_part
from test_stage1_emulated import _records_text, _sig_map
from test_stage1_hc_emulated import _rnd, getseq_returns

G = SC.tile_constants("small")
T = G["tile"]
LINE_CAP = 1 << 17


@pytest.fixture(scope="module")
def hostlib():
    lib = SigStatsLib(emu.build_hostlib("small"))
    yield lib
    lib.close()


def oracle_allowed(m):
    L = S1.lib()
    return np.array([bool(L.oracle_s1_is_allowed(x, m)) for x in range(4**m)] + [False])


# ---- 0: the oracles
def test_the_two_oracles_agree_and_count_every_window():
    rng = np.random.default_rng(1)
    for k, m in KM:
        reads = [np.frombuffer(_rnd(rng, int(n), b"ACGTN" if i % 2 else b"ACGT"), dtype=np.uint8) for i, n in enumerate(rng.integers(max(k - 2, 1), 3 * k + 60, size=12))]
        returns = [S1._CODES[r] for r in reads] + [S1._CODES[np.frombuffer(b"A" * (2 * k) + b"AC" * k + b"C" * (2 * k), dtype=np.uint8)]]
        a = SC.stats_from_superkmers(returns, k, m)
        assert np.array_equal(a, SC.stats_calcstats(returns, k, m)), (k, m)
        windows = sum(int((np.convolve((q < 0).astype(np.int64), np.ones(k, dtype=np.int64), "valid") == 0).sum()) for q in returns if q.size >= k)
        assert int(a.sum()) == windows and int(a[4**m]) > 0  # the A run: no allowed m-mer
        assert np.array_equal(SC.stats_from_superkmers(returns, k, m, True), SC.stats_calcstats(returns, k, m, True))
    assert T == 256 * G["per"] and G["per"] % 2 == 1  # the strip is odd (LDS banks), the tile is the strips of one workgroup


def test_the_kernel_alone_on_a_code_stream():
    """k_s1_sig_stats launched by tests/hipemu/emu_sigstats.cpp on a bare code stream: one workgroup per tile and two persistent ones, both table placements"""
    L = SC.kernel_lib("small")
    assert G["lds_m"] == 7 and G["wg_tile"] >= T // 2
    rng = np.random.default_rng(1)
    for k, m in ((27, 9), (5, 5), (28, 7), (256, 11)):
        n = 3 * T + 5 + k - 1
        codes = rng.integers(0, 4, size=n).astype(np.int8)
        codes[rng.integers(0, n, size=6)] = -1
        codes[T:T + T // 2] = 0
        codes[5] |= 0x40  # a piece mark is a valid code
        want = SC.stats_from_superkmers([codes], k, m)
        for grid, lds in ((0, 0), (2, 0), (0, 1), (3, 1)):
            got = np.zeros(4**m + 1, dtype=np.uint32)
            total = L.emu_s1_sig_stats(codes.ctypes.data, n, k, m, got.ctypes.data, grid, lds)
            assert total == int(want.sum()) and np.array_equal(got, want), (k, m, grid, lds)
        assert L.emu_s1_sig_stats(codes.ctypes.data, k - 1, k, m, got.ctypes.data, 0, 0) == 0


def test_the_kernels_allowed_signatures_are_the_references(hostlib):
    for m in (5, 7, 9):
        assert np.array_equal(capi.allowed_signatures(m, hostlib.L), oracle_allowed(m)), m
    buf = np.zeros(8, dtype=np.uint8)
    assert hostlib.L.kmc_hip_sigstats_allowed(4, buf.ctypes.data) == EINVAL and hostlib.L.kmc_hip_sigstats_allowed(12, buf.ctypes.data) == EINVAL
    assert hostlib.L.kmc_hip_sigstats_allowed(5, None) == EINVAL


# ---- 1: the contract of the four entries
def test_the_library_says_it_computes_the_statistics_and_keeps_its_contract(hostlib):
    L, lib = hostlib.L, hostlib
    assert L.kmc_hip_abi_version() == 4
    assert L.kmc_hip_split_covers(capi.SPLIT_COVERS_SIGSTATS) == 1 and capi.SPLIT_COVERS_SIGSTATS == 0x107
    assert [L.kmc_hip_split_covers(t) for t in (0x106, 0x108, 0x200)] == [0, 0, 0]
    for sym in capi.SYMBOLS:
        assert hasattr(L, sym), sym
    assert {"kmc_hip_sigstats_open", "kmc_hip_sigstats_part", "kmc_hip_sigstats_read", "kmc_hip_sigstats_close"} <= set(capi.SYMBOLS)
    assert lib.close_table() == 0 and lib.close_table() == 0  # closing twice is fine
    text = b">t\nACGTACGTTGCATGCATTGACCAGTAGGATCCAGT\n"
    rc, _, _ = lib.part(text, 27, 9, 0, LINE_CAP)
    assert rc == EINVAL and b"sigstats_open" in L.kmc_hip_last_error(lib.h)  # no table open
    assert L.kmc_hip_sigstats_read(lib.h, 0, 0, 1, np.zeros(1, dtype=np.uint32).ctypes.data) == EINVAL
    for k, m in ((27, 4), (27, 12), (8, 9), (257, 9), (0, 5)):
        assert lib.open(k, m) == EINVAL, (k, m)
    assert lib.open(27, 9) == 0 and lib.open(27, 9) == 0
    assert lib.open(27, 7) == EINVAL and lib.open(28, 9) == EINVAL
    for k, m in ((28, 9), (27, 7)):  # a table opened with another (k, m)
        assert lib.part(text, k, m, 0, LINE_CAP)[0] == EINVAL
    for k, m in ((27, 4), (27, 12), (8, 9)):
        assert lib.part(text, k, m, 0, LINE_CAP)[0] == EINVAL
    n = 4**9 + 1
    assert L.kmc_hip_sigstats_read(lib.h, 0, 1, n, None) == EINVAL and L.kmc_hip_sigstats_read(lib.h, 0, n + 1, 0, None) == EINVAL
    assert lib.read(n, 0).size == 0 and lib.read(n - 1, 1).size == 1
    assert lib.close_table() == 0


def test_calls_that_add_nothing_leave_the_table_as_it_was(hostlib):
    lib, k, m = hostlib, 27, 9
    rng = np.random.default_rng(12)
    text = _records_text("fa", b"\n", [_rnd(rng, 300) for _ in range(10)])
    lib.reopen(k, m)
    assert lib.part(text, k, m, 0, LINE_CAP)[0] == 0
    want = SC.oracle_stats(getseq_returns(text, 0, k, LINE_CAP)[0], k, m)
    assert want.any() and np.array_equal(lib.read_all(m), want)
    blank = b">a\n" + _rnd(rng, 200) + b"\n\n>b\n" + _rnd(rng, 200) + b"\n"
    assert lib.part(blank, k, m, 0, LINE_CAP)[0] == UNCOVERED  # malformed text
    assert np.array_equal(lib.read_all(m), want)
    for bad in (dict(line_cap=100), dict(file_type=3), dict(flags=2), dict(flags=0x100), dict(flags=capi.SPLIT_ESTIMATE), dict(flags=capi.SPLIT_ESTIMATE | 1), dict(part_kind=2)):
        kw = dict(dict(file_type=0, line_cap=LINE_CAP, part_kind=0, flags=0), **bad)
        assert lib.part(text, k, m, kw["file_type"], kw["line_cap"], kw["part_kind"], kw["flags"])[0] == EINVAL, bad
        assert np.array_equal(lib.read_all(m), want), bad
    # n_bins, max_x and both_strands decide nothing: values the bin path refuses
    assert lib.part(text, k, m, 0, LINE_CAP, n_bins=5000, max_x=7, both=False)[0] == 0
    assert np.array_equal(lib.read_all(m), 2 * want)
    lib.close_table()


# ---- 2: sizes and seams
@pytest.mark.parametrize("k,m", KM, ids=KM_IDS)
def test_part_sizes_around_k_and_around_the_tile(hostlib, k, m):
    names = []
    for name, text, ft in SC.size_cases(T, k):
        want, returns = check_part(hostlib, text, ft, k, m, LINE_CAP)
        names.append(name)
        total = int(want.sum())
        if name.startswith("sym_"):
            assert total == max(0, int(name[4:]) + 1)
        elif name.startswith("pos_"):
            assert total == {"pos_T-1": T - 1, "pos_T": T, "pos_T+1": T + 1, "pos_3T+5": 3 * T + 5}[name] and len(returns) == 1
        elif name == "read_ends_at_tile_end":
            assert returns[0].size == T + k - 1  # its last window starts at T - 1
        else:
            assert returns[0].size == T - 2  # the next read's first code is position T - 1
    assert len(names) == 9


def test_an_invalid_code_at_every_offset_around_a_tile_seam(hostlib):
    k, m = 27, 9
    for d in range(-k, k + 1):
        want, returns = check_part(hostlib, SC.seam_n_text(T, k, d), 0, k, m, LINE_CAP)
        assert int(want.sum()) == (T + 2 * k + 5) - k + 1 - k and returns[0][T + d] < 0, d


@pytest.mark.parametrize("k,m", [(27, 9), (12, 11), (28, 7), (255, 5)], ids=["k27-m9", "k12-m11", "k28-m7", "k255-m5"])
def test_homopolymers_and_satellites(hostlib, k, m):
    for name, text, ft in SC.repeat_cases(T, k):
        want, _ = check_part(hostlib, text, ft, k, m, LINE_CAP)
        n = max(3 * T, 2 * k)
        if name == "poly_A":
            assert int(want[4**m]) >= n - k + 1  # every window of the run on the special entry
        else:
            assert int(want.max()) >= (n - k + 1) // 3 and np.count_nonzero(want >= (n - k + 1) // 3) <= 2  # one or two entries take the run


# ---- 3: formats, part kinds, -hc
@pytest.mark.parametrize("hc", [False, True], ids=["plain", "hc"])
@pytest.mark.parametrize("k,m", [(27, 9), (55, 9), (12, 11)], ids=["k27-m9", "k55-m9", "k12-m11"])
def test_formats_part_kinds_and_homopolymer_compression(hostlib, k, m, hc):
    names = []
    for name, text, ft, line_cap, long_read, returns in SC.format_cases(T, k):
        _, got = check_part(hostlib, text, ft, k, m, line_cap, long_read, hc, returns)
        names.append(name)
        if name == "pieces":
            assert len(got) >= 6 + 4  # the lines beyond line_cap came in pieces
    assert {"fastq", "fastq_crlf", "fasta_crlf_no_final_eol", "pieces", "long_titled", "long_untitled", "multiline_0", "multiline_1", "bam"} <= set(names)


# ---- 4: the switches do not show in the result
@pytest.mark.parametrize("k,m", [(27, 5), (28, 7), (27, 9)], ids=["k27-m5", "k28-m7", "k27-m9"])
def test_the_result_depends_neither_on_the_table_placement_nor_on_the_grid(hostlib, k, m, monkeypatch):
    """m <= 7 can keep the table in LDS; with two workgroups each walks several tiles before it flushes; with one, 3T + windows of one signature pass one LDS entry"""
    rng = np.random.default_rng(4)
    text = b">poly\n" + b"A" * (3 * T) + b"\n>other\n" + _rnd(rng, 2 * T) + b"\n>again\n" + b"AC" * T + b"\n"
    want, _ = check_part(hostlib, text, 0, k, m, LINE_CAP)
    assert int(want[4**m]) >= 3 * T - k + 1
    for env in (dict(KMC_HIP_S1_SIGSTATS_LDS_M="7"), dict(KMC_HIP_S1_SIGSTATS_LDS_M="7", KMC_HIP_S1_SIGSTATS_WGS="2"), dict(KMC_HIP_S1_SIGSTATS_LDS_M="0", KMC_HIP_S1_SIGSTATS_WGS="2"),
                dict(KMC_HIP_S1_SIGSTATS_LDS_M="7", KMC_HIP_S1_SIGSTATS_WGS="1"), dict(KMC_HIP_S1_SIGSTATS_LDS_M="0", KMC_HIP_S1_SIGSTATS_WGS="1")):
        for name in ("KMC_HIP_S1_SIGSTATS_LDS_M", "KMC_HIP_S1_SIGSTATS_WGS"):
            monkeypatch.delenv(name, raising=False)
        for name, v in env.items():
            monkeypatch.setenv(name, v)
        check_part(hostlib, text, 0, k, m, LINE_CAP, want=want)


# ---- 5: accumulation
def test_parts_accumulate_over_calls_slots_and_threads(hostlib):
    k, m, lib = 27, 9, hostlib
    rng = np.random.default_rng(11)
    texts = [_records_text("fq", b"\n", [_rnd(rng, int(n)) for n in rng.integers(20, 300, size=40)] + [b"A" * 400]) for _ in range(7)]
    each = [SC.oracle_stats(getseq_returns(t, 1, k, LINE_CAP)[0], k, m) for t in texts]
    lib.reopen(k, m)
    kmers = 0
    for t in texts[:2]:  # two parts, one after the other on one slot
        rc, _, n = lib.part(t, k, m, 1, LINE_CAP)
        assert rc == 0
        kmers += n
    want = each[0] + each[1]
    assert np.array_equal(lib.read_all(m), want) and kmers == int(want.sum())
    for t in texts[2:5]:  # five in all
        assert lib.part(t, k, m, 1, LINE_CAP)[0] == 0
    want = want + each[2] + each[3] + each[4]
    assert np.array_equal(lib.read_all(m), want)
    rcs = {}

    def work(slot, t):
        rcs[slot] = lib.part(t, k, m, 1, LINE_CAP, slot=slot)[0]

    th = [threading.Thread(target=work, args=(1 + i, texts[5 + i])) for i in range(2)]  # two slots from two host threads at once
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert rcs == {1: 0, 2: 0}
    want = want + each[5] + each[6]
    assert np.array_equal(lib.read_all(m), want) and np.array_equal(lib.read_all(m), want)  # reading does not clear
    assert np.array_equal(np.concatenate([lib.read(f, min(50_000, want.size - f)) for f in range(0, want.size, 50_000)]), want)  # reads at chunk offsets
    lib.close_table()


# ---- 6: the histogram is the cut's: per bin, the statistics of its signatures are the k-mers the bin path puts there
@pytest.mark.parametrize("hc", [False, True], ids=["plain", "hc"])
def test_the_statistics_of_a_bins_signatures_are_the_bins_kmers(hostlib, hc):
    k, m, n_bins = 27, 9, 37
    rng = np.random.default_rng(21)
    text = _records_text("fq", b"\n", [_rnd(rng, int(n), b"ACGTacgtN" if i % 5 == 0 else b"ACGT") for i, n in enumerate(rng.integers(20, 400, size=60))] + [b"A" * 300, b"AC" * 200])
    for seed in (5, 6):
        smap = _sig_map(m, n_bins, seed)
        rc, got = hostlib.split(text, k, m, n_bins, smap, LINE_CAP, 1, flags=capi.SPLIT_HOMOPOLYMER if hc else 0)
        assert rc == 0, got
        hostlib.reopen(k, m)
        rc, n_reads, n_kmers = hostlib.part(text, k, m, 1, LINE_CAP, flags=capi.SPLIT_HOMOPOLYMER if hc else 0)
        assert rc == 0 and n_reads == got["n_reads"] and n_kmers == int(got["kmers"].sum())
        stats = hostlib.read_all(m)
        per_bin = np.zeros(n_bins, dtype=np.uint64)
        np.add.at(per_bin, smap[stats > 0].astype(np.int64), stats[stats > 0].astype(np.uint64))
        assert np.array_equal(per_bin, got["kmers"])
    hostlib.close_table()


# ---- 7: the balanced map
def _check_map(smap, stats, m, n_bins, allowed):
    special = 4**m
    assert smap.dtype == np.int32 and smap.size == special + 1
    assert np.all(smap[:special][~allowed[:special]] == -1)
    on = np.append(allowed[:special], True)
    assert smap[on].min() >= 0 and smap[on].max() < n_bins
    assert np.count_nonzero(smap == smap[special]) == 1  # the special signature's bin holds nothing else
    # what Init must do with the leading signatures, worked out without its groups: in descending order (ties: ascending signature) each one above the running
    # mean = (weight left) / (bins left) gets the next bin alone
    sig = np.flatnonzero(allowed[:special])
    w = stats[sig].astype(np.float64) + 1000.0
    order = np.argsort(-w, kind="stable")
    sig, w = sig[order], w[order]
    left, bin_no, alone = float(w.sum()), 0, 0
    mean = left / n_bins
    members = np.bincount(smap[smap >= 0], minlength=n_bins)
    while alone < sig.size and sig.size - alone > n_bins - 1 - bin_no and w[alone] > mean:
        assert smap[sig[alone]] == bin_no and members[bin_no] == 1, (alone, int(sig[alone]))
        left -= float(w[alone])
        bin_no += 1
        alone += 1
        if n_bins - 1 - bin_no <= 0:
            break
        mean = left / (n_bins - 1 - bin_no)
    return alone


@pytest.mark.parametrize("n_bins", [64, 65, 512, 2000])
def test_the_balanced_map_keeps_inits_invariants(hostlib, n_bins):
    m = 7
    allowed = oracle_allowed(m)
    rng = np.random.default_rng(n_bins)
    zero = np.zeros(4**m + 1, dtype=np.uint32)
    assert _check_map(tools.balanced_signature_map(zero, m, n_bins, allowed), zero, m, n_bins, allowed) == 0
    one = zero.copy()
    one[int(np.flatnonzero(allowed)[100])] = 3_000_000_000  # one signature holds everything
    assert _check_map(tools.balanced_signature_map(one, m, n_bins, allowed), one, m, n_bins, allowed) >= 1
    one[4**m] = 123_456  # the special signature's own count decides nothing
    assert np.array_equal(tools.balanced_signature_map(one, m, n_bins, allowed), tools.balanced_signature_map(one, m, n_bins, allowed))
    skew = (rng.pareto(0.7, size=4**m + 1) * 50).astype(np.uint32)  # a heavy tail: several signatures above the mean
    skew[~np.append(allowed[:4**m], True)] = 0
    smap = tools.balanced_signature_map(skew, m, n_bins, allowed)
    assert _check_map(smap, skew, m, n_bins, allowed) >= (3 if n_bins < 2000 else 0)
    assert np.array_equal(smap, tools.balanced_signature_map(skew, m, n_bins, capi.allowed_signatures(m, hostlib.L)))  # the library's own allowedness
    if n_bins <= 512:  # more signatures than bins: some bins are groups
        assert np.bincount(smap[smap >= 0], minlength=n_bins).max() > 1


def test_the_balanced_map_refuses_what_init_cannot_do():
    with pytest.raises(ValueError):
        tools.balanced_signature_map(np.zeros(4**5 + 1, dtype=np.uint32), 5, 63, np.ones(4**5 + 1, dtype=bool))
    with pytest.raises(ValueError):
        tools.balanced_signature_map(np.zeros(4**5, dtype=np.uint32), 5, 64, np.ones(4**5 + 1, dtype=bool))


# ---- 8: the front end
@pytest.fixture(scope="module")
def count_lib():
    c = CC.CountContext(emu.build_hostlib("small"))
    yield c
    c.close()


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    k, m, n_bins = 27, 5, 64
    text, (s1, s2) = SC.planted_input(k, m, n_bins)
    d = tmp_path_factory.mktemp("planted")
    path = str(d / "planted.fa")
    with open(path, "wb") as f:
        f.write(text)
    stats = SC.oracle_stats(getseq_returns(text, 0, k, capi.SPLIT_LINE_CAP)[0], k, m)
    fixed = tools.count_signature_map(m, n_bins)
    assert fixed[s1] == fixed[s2] and s1 != s2 and min(int(stats[s1]), int(stats[s2])) * 5 > int(stats.sum())  # each carries more than a fifth
    balanced = tools.balanced_signature_map(stats, m, n_bins, oracle_allowed(m))
    want = dict(fixed=SC.balance_of(stats, fixed, n_bins), stats=SC.balance_of(stats, balanced, n_bins))
    assert want["stats"] < want["fixed"] and balanced[s1] != balanced[s2]  # the oracle alone shows it
    return path, want, k, m, n_bins


def test_count_with_the_map_from_the_statistics_balances_the_planted_input(count_lib, planted, tmp_path):
    path, want, k, m, n_bins = planted
    res, body = {}, {}
    for which in ("fixed", "stats"):
        out = str(tmp_path / which)
        res[which] = tools.count([f"-k{k}", "-ci1", "-fa", f"-p{m}", f"-n{n_bins}", path, out], ctx=count_lib, part_bytes=1 << 20, signature_map=which)
        body[which] = CC.database_bytes(out)
        assert res[which]["n_parts"] == 1 and res[which]["map"] == which
        assert res[which]["balance"] == want[which], (which, res[which]["balance"], want[which])
        assert ("the map from stage-0 statistics" if which == "stats" else "the fixed signature map") in tools.count_report(res[which])
    assert body["fixed"] == body["stats"] and res["fixed"]["stats"] == res["stats"]["stats"]
    assert res["stats"]["balance"] < res["fixed"]["balance"]
    few = tools.count([f"-k{k}", "-ci1", "-fa", "-n8", path, str(tmp_path / "few")], ctx=count_lib, part_bytes=1 << 20, signature_map="stats")
    assert few["map"] == "fixed" and CC.database_bytes(str(tmp_path / "few")) == body["fixed"]  # below the reference's 64 bins the fixed map stays
    with pytest.raises(ValueError):
        tools.count([f"-k{k}", "-fa", path, str(tmp_path / "x")], ctx=count_lib, signature_map="balanced")


def test_the_environment_selects_the_map_for_the_command_line(planted, tmp_path, monkeypatch, capsys):
    path, want, k, m, n_bins = planted
    monkeypatch.setenv("KMC_HIP_LIB", emu.build_hostlib("small"))
    monkeypatch.setattr(capi, "_LIB", None)
    argv = ["count", f"-k{k}", "-ci1", "-fa", f"-p{m}", f"-n{n_bins}", path]
    monkeypatch.setenv("KMC_HIP_COUNT_MAP", "stats")
    assert tools.main(argv + [str(tmp_path / "b")]) == 0
    out = capsys.readouterr().out
    assert "the map from stage-0 statistics" in out and "%.2f" % want["stats"] in out and "the fixed signature map" not in out
    assert os.path.getsize(str(tmp_path / "b.kmc_suf")) > 0


@pytest.mark.parametrize("n_bins", [64, 512])
def test_a_recorded_run_counted_with_the_statistics_map_gives_the_golden_bytes(count_lib, n_bins, tmp_path):
    name = CC.CASE_IDS[0]
    out = str(tmp_path / "o")
    res = tools.count(CC.CASES[name][0] + ["-n%d" % n_bins, CC.input_argument(name, tmp_path), out, str(tmp_path)], ctx=count_lib, part_bytes=2048, signature_map="stats")
    assert res["map"] == "stats" and CC.database_bytes(out) == CC.database_bytes(CC.golden_out(name))
    assert res["stats"] == CC.case_oracle(name)["summary"] and res["n_parts"] >= 3
