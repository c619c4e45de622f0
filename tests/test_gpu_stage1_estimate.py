"""-m gpu: histogram estimation while counting (--opt-out-size) on the device. The per-part cases of tests/test_stage1_estimate_emulated.py on
libkmc_hip.so (k_s1_nthash_estimate on gfx950), one 8 MB part at the reference's r = 27, then kmc_hip_s1 --opt-out-size against the reference's
kmc --opt-out-size: database bytes, statistics lines, the estimated number of unique k-mers — and one input on which the estimate decides lut_prefix_len."""
import hashlib
import os
import subprocess
import threading

import numpy as np
import pytest

from kmc_amd import build as B
from kmc_amd import capi, synth
from test_stage1_emulated import _parse_bin, _records_text
from test_stage1_estimate_emulated import (ECAPACITY, EINVAL, M, N_BINS, R_SMALL, UNCOVERED, EstLib, _smap, accepted_homopolymer, add_part, check_est,
                                           check_pair, nt_counters, nt_hits, run_pair)
from test_stage1_hc_emulated import _rnd, getseq_returns, piece_lines, seam_reads
from test_stage1_multiline_emulated import _wrap, reader_parts

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    L = EstLib(os.environ.get("KMC_HIP_LIB") or B.LIB_HIP)
    yield L
    L.close()


def test_the_library_says_it_covers_the_estimate_and_keeps_its_contract(lib):
    L = lib.L
    assert L.kmc_hip_abi_version() == 4
    assert L.kmc_hip_split_covers(capi.SPLIT_COVERS_ESTIMATE) == 1 and [L.kmc_hip_split_covers(t) for t in (0x100, 0x101, 0x200)] == [1, 0, 0]
    lib.close_estimator()
    text, cap = b">t\nACGTACGTTGCATGCATTGACCAGTAGGATCCAGT\n", 27 + 4105
    rc, msg = lib.split(text, 27, M, N_BINS, _smap(), cap, 0, flags=4)
    assert rc == EINVAL and b"estimate_open" in msg
    assert lib.open(27, 0, R_SMALL) == EINVAL and lib.open(27, 7, 28) == EINVAL
    assert lib.open(27, 7, R_SMALL) == 0 and lib.open(27, 7, R_SMALL) == 0 and lib.open(27, 11, R_SMALL) == EINVAL and lib.open(21, 7, R_SMALL) == EINVAL
    rc, msg = lib.split(text, 21, M, N_BINS, _smap(), 21 + 4105, 0, flags=4)
    assert rc == EINVAL and b"kmer_len" in msg
    for flags in (2, 3, 0x100):
        rc, msg = lib.split(text, 27, M, N_BINS, _smap(), cap, 0, flags=flags)
        assert rc == EINVAL and b"flags" in msg, flags
    big = _records_text("fq", b"\n", seam_reads(27))
    rc, with_est = lib.split(big, 27, M, N_BINS, _smap(), 1 << 17, 1, flags=0)
    assert rc == 0 and not lib.read_all(R_SMALL).any()
    lib.close_estimator()
    rc, without = lib.split(big, 27, M, N_BINS, _smap(), 1 << 17, 1, flags=0)
    assert rc == 0 and all(a.size == b.size and _parse_bin(a, 27) == _parse_bin(b, 27) for a, b in zip(with_est["bins"], without["bins"]))
    assert all(np.array_equal(with_est[key], without[key]) for key in ("kmers", "supers", "plus_x"))


@pytest.mark.parametrize("k", [21, 27, 31, 33, 55, 62, 66, 127, 256])
def test_windows_across_every_seam_of_the_estimate_kernel(lib, k):
    reads = seam_reads(k)
    at = sum(len(x) + 1 for x in reads)
    body = bytearray(_rnd(np.random.default_rng(k), 4 * 4096 - at + k + 50))
    body[4 * 4096 - at + 3] = ord("N")  # an invalid code inside the fourth tile's halo
    reads.append(bytes(body))
    for s in (1, 7):
        for fmt, eol in (("fq", b"\n"), ("fq", b"\r\n"), ("fa", b"\n"), ("fa", b"\r\n")):
            text = _records_text(fmt, eol, reads)
            if fmt == "fa":
                text = text[:len(text) - len(eol)]  # a window that ends on the last code of the stream
            want, _ = check_est(lib, text, 1 if fmt == "fq" else 0, k, s, 1 << 17)
            assert want.any()


def test_same_address_atomics_pieces_formats_and_homopolymer_compression(lib):
    k, letter = accepted_homopolymer()
    want, _ = check_est(lib, b">poly\n" + letter * 9000 + b"\n>other\n" + _rnd(np.random.default_rng(4), 500) + b"\n", 0, k, 1, 1 << 17)
    assert want.max() >= 9000 - k + 1
    for fmt, k, s in (("fq", 27, 7), ("fa", 21, 1), ("fa", 55, 1)):
        rng = np.random.default_rng(50 + k)
        lines, line_cap, _ = piece_lines(k, rng)
        ft = 1 if fmt == "fq" else 0
        text = _records_text(fmt, b"\n", lines)
        want, returns = check_est(lib, text, ft, k, s, line_cap)
        assert len(returns) >= len(lines) + 11
        lib.reopen(k, s, R_SMALL)  # with -hc: the counters of flags = 4, the bins of flags = 1
        both = add_part(lib, text, ft, k, line_cap, flags=5)
        assert np.array_equal(lib.read_all(R_SMALL), want)
        hc = add_part(lib, text, ft, k, line_cap, flags=1)
        assert all(a.size == b.size and _parse_bin(a, k) == _parse_bin(b, k) for a, b in zip(both["bins"], hc["bins"]))
        assert np.array_equal(lib.read_all(R_SMALL), want)
    for fmt, k in (("fa", 27), ("fq", 21)):
        rng = np.random.default_rng(70 + k)
        line_cap = k + 4105
        stride = line_cap - k + 1
        ft, marker = (1, b"@") if fmt == "fq" else (0, b">")
        body = synth.homopolymer_rich_sequence(rng, 3 * stride + 1234, 1.8, 0.2, 2000, 9).tobytes()
        for titled in (True, False):
            check_est(lib, (marker + b"read 1 of a long-read file\n" if titled else b"") + body, ft, k, 1, line_cap, long_read=True)
        seq = synth.homopolymer_rich_sequence(rng, 3 * stride + 777, 1.8, 0.2, 2000, 9).tobytes()
        text = b">long\n" + _wrap(seq, 60, b"\n") + b">e1\n>e2\r\n>short\n" + _wrap(_rnd(rng, 50), 60, b"\n") + b">poly\n" + _wrap(b"A" * 500, 60, b"\n")
        parts = reader_parts(text, 9000, k)
        assert any(p[:1] != b">" for p in parts)
        for part in parts:
            check_est(lib, part, 2, k, 7 if k == 27 else 1, line_cap)


def test_accumulation_and_calls_that_add_nothing(lib):
    k, s = 27, 1
    rng = np.random.default_rng(11)
    texts = [_records_text("fq", b"\n", [_rnd(rng, int(n)) for n in rng.integers(20, 300, size=40)] + [b"A" * 400]) for _ in range(4)]
    each = [nt_counters(getseq_returns(t, 1, k, 1 << 17)[0], k, s, R_SMALL) for t in texts]
    lib.reopen(k, s, R_SMALL)
    smap = _smap()
    assert lib.L.kmc_hip_split_set_map(lib.h, 0, smap.ctypes.data, M) == 0
    for t in texts[:2]:
        assert lib.split_slot(0, t, k, M, N_BINS, smap, 1 << 17, 1, 0, 4)[0] == 0
    rcs = {}

    def work(slot, t):
        rcs[slot] = lib.split_slot(slot, t, k, M, N_BINS, smap, 1 << 17, 1, 0, 4)[0]

    th = [threading.Thread(target=work, args=(1 + i, texts[2 + i])) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert rcs == {1: 0, 2: 0}
    want = each[0] + each[1] + each[2] + each[3]
    assert np.array_equal(lib.read_all(R_SMALL), want) and np.array_equal(lib.read_all(R_SMALL), want)
    n = 1 << R_SMALL
    assert np.array_equal(lib.read(n - 100, 300), want[n - 100:n + 200])
    lib.reopen(k, s, R_SMALL)
    blank = b">a\n" + _rnd(rng, 200) + b"\n\n>b\n" + _rnd(rng, 200) + b"\n"
    assert lib.split_slot(0, blank, k, M, N_BINS, smap, 1 << 17, 0, 0, 4)[0] == UNCOVERED
    text = _records_text("fa", b"\n", [_rnd(rng, 300) for _ in range(30)])
    rc, need = lib.split_slot(0, text, k, M, N_BINS, smap, 1 << 17, 0, 0, 4, recs_capacity=16)
    assert rc == ECAPACITY and need > 16 and not lib.read_all(R_SMALL).any()
    assert lib.split_slot(0, text, k, M, N_BINS, smap, 1 << 17, 0, 0, 4, recs_capacity=need)[0] == 0
    assert np.array_equal(lib.read_all(R_SMALL), nt_counters(getseq_returns(text, 0, k, 1 << 17)[0], k, s, R_SMALL))


def test_large_part_on_the_device_at_the_reference_geometry(lib):
    """one 8 MB part of the -hc large-part kind (~2 000 tiles): homopolymer-rich records with mixed case and N runs, one of 2.5 Mbp beyond a 1 MB line cap, a run
    of 20 000 identical symbols; k = 27, s = 7, r = 27, the non-zero counters read back in chunks"""
    rng = np.random.default_rng(17)
    recs = []
    for i in range(45):
        n = 2_500_000 if i == 7 else int(rng.integers(1000, 250_000))
        recs.append(synth.homopolymer_rich_sequence(rng, n, 2.0, 0.2, 30, 40).tobytes())
        if i == 20:
            recs.append(b"G" * 20_000)
    text = b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(recs))
    assert 7_000_000 < len(text) < 10_000_000
    k, s, r = 27, 7, 27
    lib.reopen(k, s, r)
    add_part(lib, text, 0, k, 1 << 20)
    ent, cnt = lib.read_nonzero(r)
    lib.close_estimator()
    w_ent, w_cnt = nt_hits(getseq_returns(text, 0, k, 1 << 20)[0], k, s, r)
    assert w_ent.size > 50_000 and np.array_equal(ent, w_ent) and np.array_equal(cnt, w_cnt)


# ---- kmc_hip_s1 --opt-out-size against kmc --opt-out-size
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
        return r.returncode, None, r.stdout + r.stderr
    md5 = tuple(hashlib.md5(open(db + x, "rb").read()).hexdigest() for x in (".kmc_pre", ".kmc_suf"))
    stats = [ln.split(":")[1].strip() for ln in r.stdout.splitlines() if "No. of" in ln or "Total no." in ln]
    return 0, (md5, stats), r.stdout + r.stderr


_IN = {}


def _reads(tmp_path_factory, fmt):
    """~5 Mbp: the 3.4 Mbp record arrives as long-read parts under -m2, the 600 kbp ones are lines beyond mem_part_pmm_reads inside ordinary parts"""
    if fmt not in _IN:
        p = str(tmp_path_factory.mktemp("est") / ("reads." + fmt))
        if fmt == "ml":
            rng = np.random.default_rng(5)
            with open(p, "wb") as f:
                for i, n in enumerate([900_000, 0, 3_400_000, 20_000, 600_000]):
                    f.write(b">ctg%d\n" % i + _wrap(synth.homopolymer_rich_sequence(rng, n, 2.0, 0.2, 30, 40).tobytes(), 60, b"\n"))
        else:
            synth.make_long_reads(p, 4, [200, 600_000, 150, 3_400_000, 90, 530_000, 40_000], fmt=fmt, mean_run=2.0, lower_frac=0.2, n_run_per_mbp=30, n_run_len=40)
        _IN[fmt] = p
    return _IN[fmt]


@pytest.mark.parametrize("flags,fmt", [(["-k27", "-ci1"], "fq"), (["-k55"], "fq"), (["-k27", "-hc"], "fq"), (["-k27", "-fm"], "ml")], ids=["k27ci1", "k55", "k27hc", "k27fm"])
def test_kmc_hip_s1_opt_out_size_writes_the_reference_database(flags, fmt, tmp_path, tmp_path_factory):
    _require_binaries()
    if _state["broken"]:
        pytest.fail("an earlier run of kmc_hip_s1 --opt-out-size failed or hung")
    check_pair(*run_pair(_run, flags, _reads(tmp_path_factory, fmt), tmp_path, {}))


def lut_prefix_len(pre_path):
    """lut_prefix_len from the header at the end of a .kmc_pre file (kmc_file.cpp:181-198: the byte 8 from the end is the header's offset)"""
    raw = open(pre_path, "rb").read()
    assert raw[-4:] == b"KMCP"
    header = raw[len(raw) - (raw[-8] + 8):]
    return int.from_bytes(header[12:16], "little")  # kmer_length, mode, counter_size, lut_prefix_length


def test_the_estimate_decides_lut_prefix_len_and_the_device_estimate_decides_the_same(tmp_path):
    """16 Mbp of uniform random sequence in 64 reads of 250 kbp, -k27 -ci1 -n64. Without --opt-out-size stage 2 guesses 4 x n_reads = 256 unique k-mers and takes
    the smallest LUT (kmc.h:1436-1468): lut_prefix_len 3. With it the estimate is about 16 M, and 64 bins x 4^7 x 8 B = 8.4 MB of LUT plus 16 M x 5 B of suffixes is
    less than 16 M x 6 B: lut_prefix_len 7. Checked with the reference alone on the CPU: 3 without the flag, 7 with it ("Estimated number of unique counted
    k-mers: 16055770" of 15 998 336). kmc_hip_s1 --opt-out-size must write the bytes of the reference's run WITH the flag."""
    _require_binaries()
    if _state["broken"]:
        pytest.fail("an earlier run of kmc_hip_s1 --opt-out-size failed or hung")
    inp = str(tmp_path / "random.fa")
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    with open(inp, "wb") as f:
        for i in range(64):
            f.write(b">r%d\n" % i + acgt[rng.integers(0, 4, size=250_000)].tobytes() + b"\n")
    flags = ["-k27", "-ci1", "-fa", "-n64"]
    rc, plain, log = _run("kmc", flags + ["-m2", "-sf1", "-sp1", "-sr1"], inp, tmp_path, "plain")
    assert rc == 0, log[-1500:]
    plain_lut = lut_prefix_len(str(tmp_path / "db_plain.kmc_pre"))
    want, got, ref_log, hip_log = run_pair(_run, flags, inp, tmp_path, {})
    ref_lut, hip_lut = lut_prefix_len(str(tmp_path / "db_ref.kmc_pre")), lut_prefix_len(str(tmp_path / "db_hip.kmc_pre"))
    print("lut_prefix_len: kmc", plain_lut, "kmc --opt-out-size", ref_lut, "kmc_hip_s1 --opt-out-size", hip_lut)
    assert (plain_lut, ref_lut) == (3, 7) and plain[0] != want[0]  # the reference alone: the estimate matters on this input
    assert hip_lut == ref_lut
    check_pair(want, got, ref_log, hip_log)
