"""-m gpu: stage 1 on the device for multi-line FASTA (-fm). The per-part parity cases of tests/test_stage1_multiline_emulated.py on libkmc_hip.so
(k_s1_ml_text_to_codes / k_s1_ml_marks on gfx950), then kmc_hip_s1 -fm against the reference's kmc -fm on a synthetic assembly whose longest contig
is larger than one 32 MB reader part: continuation parts and piece cuts both occur. Database md5 and the five statistics lines."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from kmc_amd import build as B
from kmc_amd import synth
from test_stage1_multiline_emulated import SplitLib, check_part, multiline_cases, reader_parts

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    L = SplitLib(os.environ.get("KMC_HIP_LIB") or B.LIB_HIP)
    yield L
    L.close()


@pytest.mark.parametrize("k", [27, 21, 55])
def test_multiline_parts_on_the_device_match_getseq(lib, k):
    cases, line_cap = multiline_cases(k)
    for name, text in cases.items():
        for part in reader_parts(text, 700 if name != "long_sequence" else 12000, k):
            check_part(lib, part, k, line_cap)
        check_part(lib, text, k, line_cap)


def test_large_multiline_part_on_the_device(lib):
    """one 8 MB part (thousands of tiles: the three look-backs walk) with 60-column lines, soft-masking, N runs and a sequence beyond a 1 MB line cap"""
    rng = np.random.default_rng(17)
    a = np.frombuffer(b"ACGTacgtACGTACGTN", dtype=np.uint8)
    out = []
    for i in range(40):
        seq = a[rng.integers(0, a.size, size=int(rng.integers(1000, 150_000)) if i != 7 else 2_500_000)].tobytes()
        out.append(b">ctg%d\n" % i + seq)  # the reader's output: no line ends inside a sequence
    check_part(lib, b"".join(out) + b">amp\n" * 3000, 27, 1 << 20)
    # a million 20 bp amplicons in one ~24 MB part: more titles than the line arrays of single-line FASTA would take
    amp = a[rng.integers(0, 4, size=(1_000_000, 20))]
    recs = np.concatenate([np.tile(np.frombuffer(b">a\n", dtype=np.uint8), (amp.shape[0], 1)), amp], axis=1)
    rc, got = lib.split_part(recs.tobytes(), 17, 7, 64, np.random.default_rng(1).integers(0, 64, size=(1 << 14) + 1).astype(np.int32), 17 + 4105)
    assert rc == 0, got
    assert got["n_reads"] == 1_000_000 and int(got["kmers"].sum()) == 4_000_000  # 20 - 17 + 1 k-mers per amplicon (a is ACGT for indices < 4)
    rc, _ = lib.split_part(b">t\nACGT" * 1000 + b">unterminated", 27, 9, 8, np.zeros((1 << 18) + 1, dtype=np.int32), 27 + 4105)
    assert rc == 1


# ---- kmc_hip_s1 -fm against kmc -fm
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


_FA = {}


def _assembly(tmp_path_factory, eol):
    """~45 Mbp: one 36 Mbp contig (beyond a 32 MB reader part), a few Mbp-sized ones, many small ones, empty records"""
    if eol not in _FA:
        p = str(tmp_path_factory.mktemp("fm") / ("asm_%s.fa" % ("crlf" if eol == b"\r\n" else "lf")))
        rng = np.random.default_rng(3)
        lens = [36_000_000, 4_000_000, 2_500_000] + [int(x) for x in rng.integers(200, 20_000, size=300)]
        synth.make_multiline_fasta(p, seed=21, contig_lens=lens, line_width=60 if eol == b"\n" else 80, lower_frac=0.3, n_run_per_mbp=3, n_run_len=500,
                                   n_empty=5, eol=eol)
        _FA[eol] = p
    return _FA[eol]


@pytest.mark.parametrize("flags,eol", [(["-k27", "-ci1"], b"\n"), (["-k21"], b"\n"), (["-k55"], b"\n"), (["-k27", "-b"], b"\n"), (["-k27", "-ci1"], b"\r\n")],
                         ids=["k27ci1", "k21", "k55", "k27b", "k27ci1-crlf"])
def test_kmc_hip_s1_fm_writes_the_reference_database(flags, eol, tmp_path, tmp_path_factory):
    _require_binaries()
    if _state["broken"]:
        pytest.fail("an earlier run of kmc_hip_s1 -fm failed or hung")
    fa = _assembly(tmp_path_factory, eol)
    want = _run("kmc", flags + ["-fm", "-m8", "-sf1", "-sp1", "-sr1"], fa, tmp_path, "ref")
    got = _run("kmc_hip_s1", flags + ["-fm", "-m8", "-sf1", "-sp2", "-sr4"], fa, tmp_path, "hip", env={"KMC_HIP_VERBOSE": "1"})
    assert got[:2] == want[:2] and len(want[1]) >= 5
    rep = re.findall(r"(\d+) uncovered parts, .* (\d+) multi-line FASTA parts", got[2])
    assert rep and sum(int(u) for u, _ in rep) == 0 and sum(int(m) for _, m in rep) >= 2, got[2][-2000:]
