"""-m gpu: stage 1 on the device with homopolymer compression (-hc). The per-part cases of tests/test_stage1_hc_emulated.py on libkmc_hip.so
(k_s1_hc_compact on gfx950), one 8 MB part whose look-back walks over thousands of tiles, then kmc_hip_s1 -hc against the reference's kmc -hc on
generated long reads that the reader hands out as long-read parts: database bytes and the statistics lines."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from kmc_amd import build as B
from kmc_amd import capi, synth
from test_stage1_emulated import _records_text, _sig_map
from test_stage1_hc_emulated import HcLib, _norun, _write_multiline, check_hc, piece_lines, seam_reads
from test_stage1_multiline_emulated import _wrap, multiline_cases, reader_parts

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    L = HcLib(os.environ.get("KMC_HIP_LIB") or B.LIB_HIP)
    yield L
    L.close()


def test_the_library_says_it_covers_homopolymer_compression(lib):
    assert lib.L.kmc_hip_abi_version() == 4
    assert lib.L.kmc_hip_split_covers(capi.SPLIT_COVERS_HOMOPOLYMER) == 1 and lib.L.kmc_hip_split_covers(0x101) == 0
    rc, msg = lib.split(b">t\nACGTACGT\n", 27, 9, 8, _sig_map(9, 8, 1), 27 + 4105, 0, flags=2)
    assert rc == -1 and b"flags" in msg


@pytest.mark.parametrize("k,both", [(27, True), (21, True), (55, True), (27, False)], ids=["k27", "k21", "k55", "k27-b"])
def test_seams_pieces_long_read_and_multiline_parts_on_the_device(lib, k, both):
    reads = seam_reads(k)
    for fmt, eol in (("fq", b"\n"), ("fq", b"\r\n"), ("fa", b"\n"), ("fa", b"\r\n")):
        check_hc(lib, _records_text(fmt, eol, reads), 1 if fmt == "fq" else 0, k, 1 << 17, both=both)
    rng = np.random.default_rng(50 + k)
    lines, line_cap, special = piece_lines(k, rng)
    stride = line_cap - k + 1
    for fmt, eol in (("fq", b"\n"), ("fa", b"\r\n")):
        ft = 1 if fmt == "fq" else 0
        assert check_hc(lib, _records_text(fmt, eol, lines), ft, k, line_cap, both=both)["pieces"] >= len(lines) + 11
        for name in ("a", "b", "c"):
            check_hc(lib, _records_text(fmt, eol, [special[name]]), ft, k, line_cap, both=both)
    body = bytearray(synth.homopolymer_rich_sequence(rng, 4 * stride + 1234, 1.8, 0.2).tobytes())
    for ft, marker in ((0, b">"), (1, b"@")):
        for shift in (1, 0):
            b = bytearray(body)
            b[stride - shift] = b[stride - shift - 1]
            b[2 * stride - shift + 4] = b[2 * stride - shift + 5] = ord("c")
            b[3 * stride - shift] = ord("N")
            w = check_hc(lib, (marker + b"a long read\n" if shift else b"") + bytes(b), ft, k, line_cap, long_read=True, both=both)
            assert w["n_reads"] == shift and w["pieces"] == 5
    base = _norun(rng, stride + 700)
    check_hc(lib, base[:stride] + base[stride - 1:stride] + base[stride:], 0, k, line_cap, long_read=True, both=both)
    cases, _ = multiline_cases(k)
    rich = lambda n: synth.homopolymer_rich_sequence(rng, n, 1.8, 0.2, 2000, 9).tobytes()
    long_seq = bytearray(rich(3 * stride + 777))
    long_seq[stride] = long_seq[stride - 1]
    text = b">long\n" + _wrap(bytes(long_seq), 60, b"\n") + b">e1\n>e2\r\n>cap\n" + _wrap(rich(line_cap), 60, b"\n") + b">poly\n" + _wrap(b"A" * 500, 60, b"\n")
    parts = reader_parts(text, 12000, k)
    assert any(p[:1] != b">" for p in parts)
    for part in parts + reader_parts(cases["empty_records"], 700, k) + reader_parts(cases["lower_and_n"], 700, k):
        check_hc(lib, part, 2, k, line_cap, both=both)


def test_large_part_on_the_device(lib):
    """one 8 MB part: ~2 000 tiles, so the look-back of k_s1_hc_compact walks; homopolymer-rich records with mixed case and N runs, one of 2.5 Mbp beyond a 1 MB
    line cap (two piece starts), and a run of 20 000 identical symbols (tiles that keep nothing, in the middle of the walk)"""
    rng = np.random.default_rng(17)
    recs = []
    for i in range(45):
        n = 2_500_000 if i == 7 else int(rng.integers(1000, 250_000))
        recs.append(synth.homopolymer_rich_sequence(rng, n, 2.0, 0.2, 30, 40).tobytes())
        if i == 20:
            recs.append(b"G" * 20_000)
    text = b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(recs))
    assert 7_000_000 < len(text) < 10_000_000
    want = check_hc(lib, text, 0, 27, 1 << 20, n_bins=64)
    assert want["pieces"] == len(recs) + 2 and want["n_reads"] == len(recs)


# ---- kmc_hip_s1 -hc against kmc -hc
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


_IN = {}


def _long_reads(tmp_path_factory, fmt):
    """~6 Mbp of homopolymer-rich long reads; the 3.4 Mbp record does not fit the reader's buffer under -m2, so it arrives as long-read parts, and the
    600 kbp ones are lines beyond mem_part_pmm_reads inside ordinary parts"""
    if fmt not in _IN:
        p = str(tmp_path_factory.mktemp("hc") / ("reads." + fmt))
        if fmt == "ml":
            rng = np.random.default_rng(5)
            with open(p, "wb") as f:
                for i, n in enumerate([900_000, 0, 3_400_000, 20_000, 600_000]):
                    f.write(b">ctg%d\n" % i + _wrap(synth.homopolymer_rich_sequence(rng, n, 2.0, 0.2, 30, 40).tobytes(), 60, b"\n"))
        else:
            synth.make_long_reads(p, 4, [200, 600_000, 150, 3_400_000, 90, 530_000, 40_000, 1_200_000], fmt=fmt, mean_run=2.0, lower_frac=0.2, n_run_per_mbp=30, n_run_len=40)
        _IN[fmt] = p
    return _IN[fmt]


@pytest.mark.parametrize("flags,fmt", [(["-k27", "-ci1"], "fq"), (["-k21"], "fa"), (["-k55"], "fq"), (["-k27", "-b"], "fq"), (["-k27", "-fm"], "ml")],
                         ids=["k27ci1", "k21-fa", "k55", "k27b", "k27fm"])
def test_kmc_hip_s1_hc_writes_the_reference_database(flags, fmt, tmp_path, tmp_path_factory):
    _require_binaries()
    if _state["broken"]:
        pytest.fail("an earlier run of kmc_hip_s1 -hc failed or hung")
    inp = _long_reads(tmp_path_factory, fmt)
    common = flags + (["-fa"] if fmt == "fa" else []) + ["-hc", "-m2", "-sf1"]
    want = _run("kmc", common + ["-sp1", "-sr1"], inp, tmp_path, "ref")
    got = _run("kmc_hip_s1", common + ["-sp2", "-sr2"], inp, tmp_path, "hip", env={"KMC_HIP_VERBOSE": "1"})
    assert got[:2] == want[:2] and len(want[1]) >= 5
    assert "homopolymer-compressed" in got[2]
    rep = re.findall(r"(\d+) of them long-read parts\), (\d+) uncovered parts", got[2])
    assert rep and sum(int(u) for _, u in rep) == 0, got[2][-2000:]
    if fmt != "ml":  # the multi-line reader makes ReadType::na parts, never long-read parts
        assert sum(int(n) for n, _ in rep) >= 2, got[2][-2000:]
