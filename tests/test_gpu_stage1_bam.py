"""-m gpu: stage 1 on the device for BAM input (-fbam) and KMC databases (-fkmc). The per-part cases of tests/test_stage1_bam_emulated.py on libkmc_hip.so
(k_s1_bam_chain + k_s1_bam_decode on gfx950) — a BAM part against the single-line FASTA part of the same sequences —, the densest chain over many tiles, one
8 MB part of mixed records, then kmc_hip_s1 -fbam / -fkmc against the reference's kmc: database bytes and the statistics lines."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from kmc_amd import build as B
from kmc_amd import capi, synth
from test_stage1_bam_emulated import (BAM, FLAG_SETS, LINE_CAP, SEAMS, TILE, UNCOVERED, BamLib, _seq, _write_bam, check_bam, dense_case, edge_reads, fasta_twin, good_reads,
                                      long_record_case, malformed_parts, seam_case, split)

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    L = BamLib(os.environ.get("KMC_HIP_LIB") or B.LIB_HIP)
    yield L
    L.close()


def test_the_library_says_it_covers_bam_records(lib):
    assert lib.L.kmc_hip_abi_version() == 4
    assert [lib.L.kmc_hip_split_covers(t) for t in (2, 3, 4, 5)] == [1, 0, 1, 0]


@pytest.mark.parametrize("both", [True, False], ids=["canonical", "b"])
@pytest.mark.parametrize("max_x", [0, 3])
def test_nibbles_lengths_and_flags(lib, both, max_x):
    for n_bins in (32, 64):
        reads = edge_reads(27, n_bins)
        got = check_bam(lib, reads, both=both, max_x=max_x, n_bins=n_bins)
        assert got["n_reads"] == sum(1 for _, f in reads if not f & 0x900)
    check_bam(lib, edge_reads(55, 1), both=both, max_x=max_x, k=55)


@pytest.mark.parametrize("kind,at", SEAMS, ids=["%s+%d" % s for s in SEAMS])
def test_a_record_across_the_tile_seam(lib, kind, at):
    reads, records = seam_case(kind, at)
    check_bam(lib, reads, records, both=False)
    check_bam(lib, reads, records, both=True)


@pytest.mark.parametrize("dense_around", [False, True], ids=["alone", "among-block-size-35"])
def test_a_record_longer_than_two_tiles(lib, dense_around):
    reads, records = long_record_case(dense_around)
    assert int(check_bam(lib, reads, records, both=False)["kmers"].sum()) > 5000


def test_the_densest_chain(lib):
    """block_size-35 records only, 210 hops in each of ~120 tiles. Reads of one base hold no k-mer, so the expectation needs no twin (a FASTA part of 25 000
    two-byte lines is beyond the line arrays of the single-line road): every included record is counted and every bin stays empty. The first 700 records are
    the CPU file's case, which does go through the twin."""
    reads, records = dense_case(25_000)
    rc, got = split(lib, synth.bam_part(records), BAM)
    assert rc == 0, got
    assert got["n_reads"] == sum(1 for _, f in reads if not f & 0x900) and all(b.size == 0 for b in got["bins"])
    assert not any(int(got[key].sum()) for key in ("kmers", "supers", "plus_x"))
    check_bam(lib, reads[:700], records[:700])


def test_many_tiles(lib):
    """one 8 MB part, ~1 000 tiles of the chain kernel: reads of 0 .. 400 bases with every flag, names of 1 .. 40 bytes, 0 .. 3 cigar operations, tags, N and the
    other nibble values, and three records longer than a tile"""
    rng = np.random.default_rng(31)
    alphabet = np.frombuffer(b"ACGT" * 30 + b"N=RY", dtype=np.uint8)
    reads, records, size = [], [], 0
    while size < 8_000_000:
        i = len(reads)
        n = 30_000 if i in (100, 5_000, 20_000) else int(rng.integers(0, 400))
        s = alphabet[rng.integers(0, alphabet.size, size=n)].tobytes().decode()
        f = int(rng.choice([0, 0x10, 0x100, 0x800, 0x1, 0x910]))
        reads.append((s, f))
        records.append(synth.bam_record(s, f, b"n" * int(rng.integers(0, 40)), n_cigar=i % 4, tags=b"NMC\x01" if i % 2 else b""))
        size += len(records[-1])
    assert size // TILE > 900
    got = check_bam(lib, reads, records, both=False, n_bins=64)
    assert got["n_reads"] > 10_000


def test_trivial_parts(lib):
    rc, got = split(lib, b"", BAM)
    assert rc == 0 and got["n_reads"] == 0 and int(got["kmers"].sum()) == 0
    check_bam(lib, [("ACGT" * 20, 0)])
    check_bam(lib, [("", 0)])


@pytest.mark.parametrize("name", sorted(malformed_parts()))
def test_malformed_records_are_refused_and_the_context_goes_on(lib, name):
    part, line_cap = malformed_parts()[name]
    rc, _ = split(lib, part, BAM, line_cap=line_cap)
    assert rc == UNCOVERED
    check_bam(lib, good_reads())


def test_bam_parts_with_the_flags(lib):
    rng = np.random.default_rng(11)
    reads = [(synth.homopolymer_rich_sequence(rng, int(rng.integers(30, 500)), 2.0).tobytes().decode(), int(rng.choice([0, 0x10, 0x100]))) for _ in range(300)]
    got = check_bam(lib, reads, both=False, flags=capi.SPLIT_HOMOPOLYMER, n_bins=64)
    assert int(got["kmers"].sum()) < int(check_bam(lib, reads, both=False, n_bins=64)["kmers"].sum())
    k, s, r = 27, 2, 12
    counters = []
    for file_type in (BAM, 0):
        assert lib.open(k, s, r) == 0
        text = synth.bam_part([synth.bam_record(q, f, b"e%d" % i) for i, (q, f) in enumerate(reads)]) if file_type == BAM else fasta_twin(reads, False)[0]
        rc, got = split(lib, text, file_type, both=False, flags=capi.SPLIT_ESTIMATE)
        assert rc == 0, got
        counters.append(lib.read_all(r))
        lib.close_estimator()
    assert np.array_equal(counters[0], counters[1]) and int(counters[0].sum()) > 1000


# ---- kmc_hip_s1 against kmc
def _exe(name):
    return os.path.join(ROOT, "kmc_amd", "bin", name) if name.startswith("kmc_hip") else os.path.join(ROOT, "oracle", "_ref", name)


def _require_binaries():
    missing = [n for n in ("kmc", "kmc_hip_s1") if not os.path.exists(_exe(n))]
    if missing:
        pytest.skip("needs the reference pipeline binaries (%s not built: the reference source tree was absent at build time)" % ", ".join(missing))


_state = {"broken": False}  # one failed or hung run is enough: the other parameter sets do not spend GPU time on the same problem


def _run(exe, flags, inp, tmp_path, tag, env=None):
    t = tmp_path / ("tmp_" + tag)
    t.mkdir(exist_ok=True)
    db = str(tmp_path / ("db_" + tag))
    e = dict(os.environ, KMC_HIP_LIB=os.environ.get("KMC_HIP_LIB") or B.LIB_HIP, **(env or {}))
    try:
        r = subprocess.run([_exe(exe), *flags, inp, db, str(t)], capture_output=True, text=True, env=e, timeout=300)
    except subprocess.TimeoutExpired:
        _state["broken"] = True
        raise
    if r.returncode != 0:
        _state["broken"] = True
    assert r.returncode == 0, (exe, flags, (r.stdout + r.stderr)[-1500:])
    md5 = tuple(hashlib.md5(open(db + x, "rb").read()).hexdigest() for x in (".kmc_pre", ".kmc_suf"))
    stats = [ln.split(":")[1].strip() for ln in r.stdout.splitlines() if "No. of" in ln or "Total no." in ln]
    return md5, stats, r.stderr


@pytest.mark.parametrize("flags", FLAG_SETS, ids=["default", "b", "hc", "opt-out-size", "k55"])
def test_kmc_hip_s1_fbam_writes_the_reference_database(flags, tmp_path):
    _require_binaries()
    if _state["broken"]:
        pytest.fail("an earlier run of kmc_hip_s1 failed or hung")
    inp = str(tmp_path / "in.bam")
    reads = _write_bam(inp, 23, 4000)
    common = flags + ["-fbam", "-m2", "-sf1"]
    want = _run("kmc", common + ["-sp1", "-sr1"], inp, tmp_path, "ref")
    assert int(want[1][5]) == sum(1 for _, f in reads if not f & 0x900)  # the reference reads what the generator wrote
    got = _run("kmc_hip_s1", common + ["-sp2", "-sr2"], inp, tmp_path, "hip", env={"KMC_HIP_VERBOSE": "1"})
    assert got[:2] == want[:2] and len(want[1]) >= 5
    rep = re.findall(r"(\d+) uncovered parts, .* (\d+) BAM parts", got[2])
    assert rep and sum(int(u) for u, _ in rep) == 0 and sum(int(b) for _, b in rep) >= 1, got[2][-2000:]


def test_kmc_hip_s1_fkmc_writes_the_reference_database(tmp_path):
    _require_binaries()
    if _state["broken"]:
        pytest.fail("an earlier run of kmc_hip_s1 failed or hung")
    fq = str(tmp_path / "in.fq")
    synth.make_fastq(fq, 3, 50_000, 2000, 100)
    _run("kmc", ["-k27", "-ci1", "-m2", "-sf1", "-sp1", "-sr1"], fq, tmp_path, "src")
    db = str(tmp_path / "db_src")
    common = ["-k25", "-ci1", "-fkmc", "-m2", "-sf1"]
    want = _run("kmc", common + ["-sp1", "-sr1"], db, tmp_path, "ref")
    got = _run("kmc_hip_s1", common + ["-sp2", "-sr2"], db, tmp_path, "hip", env={"KMC_HIP_VERBOSE": "1"})
    assert got[:2] == want[:2] and int(want[1][4]) > 50_000
    assert "0 uncovered parts" in got[2]
