"""-m gpu: the counting session on the device — `python -m kmc_amd.tools count` over libkmc_hip.so on the goldens of tests/count_cases.py and on a synthetic FASTQ of
about 3 MB against the numpy oracle, k_cnt_gather on the planted tables, the session's view handed to kmc_hip_db_histogram_device, and — where build() could make the
reference binaries — the same file through `kmc` + `kmc_tools transform sort`. tests/test_count_emulated.py runs the same cases on the CPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import count_cases as CC
from kmc_amd import capi, synth, tools

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")


@pytest.fixture(scope="module")
def ctx():
    capi.require_gpu_backend()
    c = capi.Context((0,))
    yield c
    c.close()


@pytest.fixture(scope="module")
def reads_file(tmp_path_factory):
    """genome 200 kbp, 20 000 reads of 150: about 6 MB of FASTQ, twelve parts and more at 256 KB"""
    path = str(tmp_path_factory.mktemp("count") / "reads.fq")
    synth.make_fastq(path, seed=41, genome_len=200_000, n_reads=20_000, read_len=150)
    with open(path, "rb") as f:
        seqs = CC.sequences(f.read(), "fq")
    return path, seqs


@pytest.fixture(scope="module")
def oracles(reads_file, tmp_path_factory):
    """k -> (the oracle's dict, the bytes of the database it writes), computed once"""
    d = tmp_path_factory.mktemp("want")
    out = {}
    for k in (27, 55):
        want = CC.count_oracle(reads_file[1], k)
        CC.write_oracle_database(str(d / f"k{k}"), want, k, 2, 10**9, 255, True)
        out[k] = (want, CC.database_bytes(str(d / f"k{k}")))
    return out


@pytest.mark.parametrize("name", CC.CASE_IDS)
def test_count_writes_the_golden_database(ctx, name, tmp_path):
    out = str(tmp_path / "o")
    res = tools.count(CC.CASES[name][0] + [CC.input_argument(name, tmp_path), out, str(tmp_path)], ctx=ctx, part_bytes=2048)
    assert CC.database_bytes(out) == CC.database_bytes(CC.golden_out(name))
    assert res["n_parts"] >= 3 and res["n_records"] == len(CC.case_oracle(name)["kmers"])


def test_gather_every_alignment_and_length(ctx):
    table, src, dst_size = CC.gather_table(every_long_pair=True)  # 70 000 bytes at all 256 offset pairs: 18 MB
    assert table.shape[0] > 2048  # more segments than the grid has workgroups
    CC.check_gather(ctx, table, src, dst_size)
    one = np.arange(70016 + 5, dtype=np.uint64).astype(np.uint8)
    CC.check_gather(ctx, np.array([[5, 3, 70000]], dtype=np.uint64), one, 70100)


@pytest.mark.parametrize("k", [27, 55])
def test_count_of_a_synthetic_file_is_the_oracle_s_database(ctx, reads_file, oracles, k, tmp_path):
    out = str(tmp_path / "o")
    res, ses, view = tools.count([f"-k{k}", reads_file[0], out], ctx=ctx, part_bytes=256 << 10, keep=True)
    try:
        want, want_bytes = oracles[k]
        assert CC.database_bytes(out) == want_bytes
        assert res["stats"] == want["summary"] and res["n_records"] == len(want["kmers"])
        assert res["n_parts"] >= 12 and res["n_segments"] >= 5000 and res["totals"]["n_reads"] == 20_000
        # the view goes straight into another entry: no file in between
        assert np.array_equal(CC.view_histogram(ctx, k, view, 255), np.bincount(want["counts"], minlength=256).astype(np.uint64))
    finally:
        ses.close()


def test_a_small_arena_runs_stage_2_in_several_batches(ctx, reads_file, oracles, tmp_path, monkeypatch):
    monkeypatch.setenv("KMC_HIP_COUNT_ARENA_MB", "1")
    monkeypatch.setenv("KMC_HIP_COUNT_CHUNK_MB", "1")
    out = str(tmp_path / "o")
    res = tools.count(["-k27", reads_file[0], out], ctx=ctx, part_bytes=256 << 10)
    assert CC.database_bytes(out) == oracles[27][1]
    assert res["n_batches"] > 1


_state = {"broken": False}  # one failed or hung run of the reference is enough


def _run_reference(argv, tmp_path):
    try:
        r = subprocess.run(argv, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    except subprocess.TimeoutExpired:
        _state["broken"] = True
        raise
    if r.returncode != 0:
        _state["broken"] = True
    assert r.returncode == 0, (argv, (r.stdout + r.stderr)[-1500:])
    return r.stdout


def test_the_live_reference_writes_the_same_database_and_prints_the_same_numbers(ctx, reads_file, tmp_path):
    missing = [n for n in ("kmc", "kmc_tools") if not os.path.exists(os.path.join(REF, n))]
    if missing:
        pytest.skip("needs the reference binaries (%s not built: the reference source tree was absent at build time)" % ", ".join(missing))
    if _state["broken"]:
        pytest.fail("an earlier run of the reference failed or hung")
    (tmp_path / "tmp").mkdir()
    text = _run_reference([os.path.join(REF, "kmc"), "-k27", "-t8", reads_file[0], str(tmp_path / "db"), str(tmp_path / "tmp")], tmp_path)
    _run_reference([os.path.join(REF, "kmc_tools"), "transform", str(tmp_path / "db"), "sort", str(tmp_path / "ref")], tmp_path)
    res = tools.count(["-k27", "-t8", reads_file[0], str(tmp_path / "ours"), str(tmp_path / "tmp")], ctx=ctx, part_bytes=256 << 10)
    assert CC.database_bytes(str(tmp_path / "ours")) == CC.database_bytes(str(tmp_path / "ref"))
    theirs = {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"^\s*((?:No\. of|Total no\. of)[^:]*):\s*(\d+)\s*$", text, re.M)}
    ours = {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"^\s*((?:No\. of|Total no\. of)[^:]*):\s*(\d+)\s*$", tools.count_report(res), re.M)}
    six = ("No. of k-mers below min. threshold", "No. of k-mers above max. threshold", "No. of unique k-mers", "No. of unique counted k-mers", "Total no. of k-mers",
           "Total no. of reads")
    assert all(name in theirs for name in six), text[-1500:]
    assert {n: ours[n] for n in six} == {n: theirs[n] for n in six}
