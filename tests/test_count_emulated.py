"""CPU: the counting session — kmc_hip_count_open / _part / _finish / _order / _close, k_cnt_gather through kmc_hip_debug_gather_segments, and
`python -m kmc_amd.tools count` — in the PRODUCT'S host library compiled over the emulated HIP runtime (tests/emu.py build_hostlib, small geometry), against the numpy
oracle of tests/count_cases.py, which the first test holds to what the reference wrote (tests/golden/count_*). The -m gpu file runs the same cases on the device."""
import os

import numpy as np
import pytest

import count_cases as CC
import emu
import setops_cases as S
from kmc_amd import capi, tools

EINVAL = -1
K = 27


@pytest.fixture(scope="module")
def lib():
    os.environ["KMC_HIP_COUNT_GATHER_WGS"] = "7"  # a grid smaller than the tables
    c = CC.CountContext(emu.build_hostlib("small"))
    yield c
    c.close()
    del os.environ["KMC_HIP_COUNT_GATHER_WGS"]


# ---- 1: the oracle is the reference
@pytest.mark.parametrize("name", CC.CASE_IDS)
def test_the_oracle_writes_what_kmc_and_kmc_tools_wrote(name, tmp_path):
    k, ci, cx, cs, both, _ = CC.CASES[name][1]
    CC.write_oracle_database(str(tmp_path / "o"), CC.case_oracle(name), k, ci, cx, cs, both)
    assert CC.database_bytes(str(tmp_path / "o")) == CC.database_bytes(CC.golden_out(name))


def test_the_committed_inputs_are_the_builders(lib):
    for name in CC.CASE_IDS:
        for path, (_, _, data) in zip(CC.golden_input_paths(name), CC.CASES[name][2]):
            assert CC.committed_input(path) == data, path
    assert lib.L.kmc_hip_split_covers(capi.SPLIT_COVERS_COUNT) == 1 and lib.L.kmc_hip_split_covers(0x104) == 0 and lib.L.kmc_hip_split_covers(0x106) == 0


# ---- 2: the goldens through the front end, three parts or more, 8 bins
@pytest.mark.parametrize("name", CC.CASE_IDS)
def test_count_writes_the_golden_database(lib, name, tmp_path):
    out = str(tmp_path / "o")
    res = tools.count(CC.CASES[name][0] + ["-n8", "-t4", CC.input_argument(name, tmp_path), out, str(tmp_path)], ctx=lib, part_bytes=2048)
    assert CC.database_bytes(out) == CC.database_bytes(CC.golden_out(name))
    want = CC.case_oracle(name)
    assert res["stats"] == want["summary"] and res["n_records"] == len(want["kmers"])
    assert res["n_parts"] >= 3 and res["totals"]["n_kmers"] == want["summary"]["n_total"]
    assert res["totals"]["n_reads"] == len(CC.case_reads(name))


# ---- 3: the result depends neither on the bins, nor on the parts, nor on the map, nor on how the store and the arena are cut
@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("small")
    path = str(d / "small.fa")
    with open(path, "wb") as f:
        f.write(CC.fasta_text(CC.small_reads(K)))
    want = CC.count_oracle(CC.small_reads(K), K, ci=1)
    CC.write_oracle_database(str(d / "want"), want, K, 1, 10**9, 255, True)
    return path, CC.database_bytes(str(d / "want")), want


VARIANTS = {"bins_1": dict(n=1), "bins_3": dict(n=3), "bins_64": dict(n=64), "parts_1024": dict(part_bytes=1024), "whole_file": dict(part_bytes=1 << 20),
            "map_a": dict(mult=0x85EBCA6B), "map_b": dict(mult=1), "chunk_per_part": dict(part_bytes=1024, env=("KMC_HIP_COUNT_CHUNK_MB", "0")),
            "bin_per_batch": dict(env=("KMC_HIP_COUNT_ARENA_MB", "0"))}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_database_does_not_depend_on_how_the_run_is_cut(lib, small, variant, tmp_path, monkeypatch):
    path, want_bytes, want = small
    v = VARIANTS[variant]
    if "env" in v:
        monkeypatch.setenv(*v["env"])
    out = str(tmp_path / "o")
    res = tools.count([f"-k{K}", "-ci1", "-fa", "-n%d" % v.get("n", 8), path, out], ctx=lib, part_bytes=v.get("part_bytes", 512), map_multiplier=v.get("mult", tools.COUNT_MAP_MULTIPLIER))
    assert CC.database_bytes(out) == want_bytes
    assert res["stats"] == want["summary"]
    if variant == "bin_per_batch":
        assert res["n_batches"] > 1
    if variant == "whole_file":
        assert res["n_parts"] == 1
    if variant == "parts_1024":
        assert res["n_parts"] == 2


# ---- 4: one session looked at from every side
@pytest.fixture(scope="module")
def session(lib):
    """parts: good, one with a blank line (KMC_HIP_UNCOVERED), good; then _finish and two _order calls"""
    reads = CC.small_reads(K)
    ses = capi.CountSession(lib, K, 9, 8, True, tools.count_signature_map(9, 8))
    p = ses.split_params(file_type=0)
    got = dict(ses=ses, p=p)
    got["rc"] = [ses.part_rc(CC.fasta_text(reads[:8]), p)[0], ses.part_rc(b">x\nACGTACGTACGTACGTACGTACGTACGTACGT\n\n>y\nACGT\n", p)[0], ses.part_rc(CC.fasta_text(reads[8:]), p)[0]]
    got["parts_before"] = ses.info()["n_parts"]
    bp = capi.make_params(K, cutoff_min=1, lut_prefix_len=3)
    got["bp"] = bp
    got["finish"] = ses.finish(bp)
    got["bodies"] = {}
    for p_out in (3, 7):
        view = ses.order(p_out)
        lut, recs = CC.view_body(lib, K, view)
        got["bodies"][p_out] = (view.counter_size, view.n_recs, S.decode_body(K, p_out, view.counter_size, lut, recs))
    got["hist"] = CC.view_histogram(lib, K, view, 255)
    yield got
    ses.close()


def test_an_uncovered_part_leaves_the_session_as_it_was(session):
    assert session["rc"] == [0, capi.UNCOVERED, 0] and session["parts_before"] == 2
    want = CC.count_oracle(CC.small_reads(K), K, ci=1)
    st, tot, n = session["finish"]
    assert dict(zip(("n_unique", "n_below_min", "n_above_max", "n_total"), (int(x) for x in st))) == want["summary"]
    assert n == len(want["kmers"]) and int(tot[0]) == len(CC.small_reads(K)) and int(tot[2]) == want["summary"]["n_total"]
    assert session["bodies"][3][2] == (want["kmers"], want["counts"])


def test_two_orders_with_different_prefix_lengths_hold_the_same_kmers(session):
    a, b = session["bodies"][3], session["bodies"][7]
    assert a[0] == b[0] == 1 and a[1] == b[1] > 0 and a[2] == b[2]


def test_the_view_goes_straight_into_the_histogram_entry(session):
    want = CC.count_oracle(CC.small_reads(K), K, ci=1)
    assert np.array_equal(session["hist"], np.bincount(want["counts"], minlength=256).astype(np.uint64))


def test_refusals(lib, session):
    ses, p, bp = session["ses"], session["p"], session["bp"]
    assert ses.part_rc(b">a\nACGT\n", p)[0] == EINVAL  # _part after _finish
    with pytest.raises(capi.KmcHipError) as e:
        ses.finish(bp)  # a second _finish
    assert e.value.code == EINVAL
    with pytest.raises(capi.KmcHipError) as e:
        ses.order(4)  # (27 - 4) % 4 != 0
    assert e.value.code == EINVAL
    with pytest.raises(capi.KmcHipError) as e:
        capi.CountSession(lib, 225, 9, 8, True, tools.count_signature_map(9, 8))
    assert e.value.code == EINVAL and "224" in str(e.value)
    fresh = capi.CountSession(lib, K, 9, 8, True, tools.count_signature_map(9, 8))
    try:
        with pytest.raises(capi.KmcHipError) as e:
            fresh.order(3)  # before _finish
        assert e.value.code == EINVAL
        text = CC.fasta_text(CC.small_reads(K)[:2])
        assert fresh.part_rc(text, fresh.split_params(file_type=0, flags=capi.SPLIT_ESTIMATE))[0] == EINVAL
        assert fresh.part_rc(text, fresh.split_params(file_type=0, kmer_len=28))[0] == EINVAL
        assert fresh.part_rc(text, fresh.split_params(file_type=0, n_bins=9))[0] == EINVAL
        assert fresh.part_rc(text, fresh.split_params(file_type=0, both_strands=0))[0] == EINVAL
        assert fresh.info()["n_parts"] == 0
        with pytest.raises(capi.KmcHipError) as e:
            fresh.finish(capi.make_params(K, cutoff_min=1, lut_prefix_len=3, output_type=1))
        assert e.value.code == EINVAL
        with pytest.raises(capi.KmcHipError) as e:
            fresh.finish(capi.make_params(K, cutoff_min=1, lut_prefix_len=3, without_output=1))
        assert e.value.code == EINVAL
    finally:
        fresh.close()


@pytest.mark.parametrize("parts", [[], [b">a\nACGTACGT\n>b\nNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN\n", b">c\nACGTACGTACGTACGTACGTACGTAC\n"]], ids=["no_parts", "reads_shorter_than_k"])
def test_a_session_without_a_kmer_finishes_with_zeros(lib, parts):
    ses = capi.CountSession(lib, K, 9, 8, True, tools.count_signature_map(9, 8))
    try:
        for t in parts:
            assert ses.part(t, ses.split_params(file_type=0)) > 0
        st, tot, n = ses.finish(capi.make_params(K, lut_prefix_len=3))
        assert not st.any() and n == 0 and int(tot[0]) == (3 if parts else 0) and not tot[1:].any()
        view = ses.order(3)
        assert view.n_recs == 0 and view.lut_prefix_len == 3
        lut, recs = CC.view_body(lib, K, view)
        assert not lut.any() and recs.size == 0
    finally:
        ses.close()


def test_destroy_closes_open_sessions():
    c = CC.CountContext(emu.build_hostlib("small"))
    ses = capi.CountSession(c, K, 9, 8, True, tools.count_signature_map(9, 8))
    assert ses.part(CC.fasta_text(CC.small_reads(K)[:3]), ses.split_params(file_type=0)) == 3
    c.close()  # the session goes with the context


# ---- 5: the command line
def test_the_parser_reads_ignores_and_refuses():
    o = tools.parse_count(["-k31", "-ci3", "-cx500", "-cs1000", "-b", "-fa", "-hc", "-p7", "-n64", "-t16", "-m12", "-r", "-sf2", "-sp4", "-sr8", "-v", "in.fa", "out", "tmp"])
    assert (o["k"], o["ci"], o["cx"], o["cs"], o["both"], o["file_type"], o["hc"], o["m"], o["n_bins"], o["inputs"], o["out"]) == (31, 3, 500, 1000, False, 0, True, 7, 64, ["in.fa"], "out")
    d = tools.parse_count(["in.fq", "out"])
    assert (d["k"], d["ci"], d["cx"], d["cs"], d["both"], d["file_type"], d["hc"], d["m"], d["n_bins"]) == (25, 2, 10**9, 255, True, 1, False, 9, 512)
    assert tools.parse_count(["-fm", "in", "out"])["file_type"] == 2 and tools.parse_count(["-fa", "-fq", "in", "out"])["file_type"] == 1
    for bad in ("-okff", "-e", "--opt-out-size", "-fbam", "-fkmc", "-sm", "-jsummary.json", "-w", "-x", "-k13", "-k225", "-p4", "-p12", "-n0", "-n2049", "-kx"):
        with pytest.raises(tools.UsageError) as e:
            tools.parse_count([bad, "in", "out"])
        assert bad in str(e.value).split("\n")[0], (bad, str(e.value))  # the first line names the option; the usage text follows it
    with pytest.raises(tools.UsageError) as e:
        tools.parse_count(["-k13", "in", "out"])
    assert "kmc_hip_smallk_" in str(e.value)
    for argv in ([], ["in"], ["a", "b", "c", "d"], ["@/nonexistent/list", "out"]):
        with pytest.raises(tools.UsageError):
            tools.parse_count(argv)


def test_the_signature_map_is_the_stated_formula():
    m = tools.count_signature_map(5, 37)
    assert m.size == 4**5 + 1 and m.dtype == np.int32 and 0 <= m.min() and m.max() < 37
    assert [int(x) for x in m[[0, 1, 1024]]] == [0, ((0x9E3779B1 & 0xFFFFFFFF) >> 8) % 37, (((1024 * 0x9E3779B1) & 0xFFFFFFFF) >> 8) % 37]


def test_a_malformed_part_stops_the_run(lib, tmp_path):
    path = str(tmp_path / "bad.fa")
    with open(path, "wb") as f:
        f.write(b">a\nACGTACGTACGTACGTACGTACGTACGTACGT\n\n>b\nACGTACGTACGTACGTACGTACGTACGTACGT\n")
    with pytest.raises(tools.UsageError) as e:
        tools.count([f"-k{K}", "-fa", "-n8", path, str(tmp_path / "o")], ctx=lib)
    assert "KMC_HIP_UNCOVERED" in str(e.value) and not os.path.exists(str(tmp_path / "o.kmc_pre"))


def test_the_report_has_kmc_s_lines():
    text = tools.count_report(dict(stats=dict(n_unique=10, n_below_min=3, n_above_max=1, n_total=40), totals=dict(n_reads=5, n_superkmers=7, n_kmers=40, bin_bytes=99),
                                   n_records=6, n_parts=2, n_segments=9, n_batches=1, balance=1.5))
    for line, v in (("No. of k-mers below min. threshold", 3), ("No. of k-mers above max. threshold", 1), ("No. of unique k-mers", 10), ("No. of unique counted k-mers", 6),
                    ("Total no. of k-mers", 40), ("Total no. of reads", 5), ("Total no. of super-k-mers", 7)):
        assert any(ln.strip().startswith(line + " ") and ln.rstrip().endswith(" %d" % v) for ln in text.split("\n")), line


# ---- 6: the gather kernel on planted tables
def test_gather_every_alignment_and_length(lib):
    table, src, dst_size = CC.gather_table()
    assert table.shape[0] > 7 * 256  # more segments than the grid has workgroups
    CC.check_gather(lib, table, src, dst_size)


def test_gather_one_segment_and_none(lib):
    src = np.arange(70016 + 5, dtype=np.uint64).astype(np.uint8)
    CC.check_gather(lib, np.array([[5, 3, 70000]], dtype=np.uint64), src, 70100)
    CC.check_gather(lib, np.zeros((0, 3), dtype=np.uint64), src[:64], 64)
