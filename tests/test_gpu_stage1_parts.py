"""-m gpu: plain FASTA / FASTQ parts on the device — kmc_hip_split_part with file_type 0 or 1 and no flags on libkmc_hip.so, the call kmc_hip_s1 makes for
nearly every part — against the reference's GetSeq + ProcessReads restatement: bin records, the three per-bin sums and n_reads. The cases of
tests/stage1_part_cases.py (tests/test_stage1_parts_emulated.py runs them on the CPU) at device sizes: more than three cutting windows of k_s1_cut, more
than one tile of k_s1_bin_totals / k_s1_bin_plus_x / k_s1_emit where k allows it within 100 KB of text. What only a device shows — wave64 ballots and
shuffles in the look-backs, LDS limits, launch bounds — for the narrow and wide minimum windows, every signature length, k up to 256, piece marks
reaching the cut, the second cut attempt and the sorted emit. No reference binaries are needed."""
import os

import pytest

import stage1_part_cases as P
from kmc_amd import build as B
from test_stage1_hc_emulated import HcLib

pytestmark = pytest.mark.gpu

CODES = 3 * P.S1_WG_TILE  # 12 288 positions: more than three cutting windows


@pytest.fixture(scope="module")
def lib():
    L = HcLib(os.environ.get("KMC_HIP_LIB") or B.LIB_HIP)
    yield L
    L.close()


def _supers(k):
    return P.S1_SK_TILE if k <= 65 else 0  # beyond k = 65 a second tile of super-k-mers needs more than 100 KB of text


# ---- (a)
@pytest.mark.parametrize("case", P.grid_cases(), ids=P.grid_ids())
def test_plain_parts_match_the_oracle_over_k_and_signature_length(lib, case):
    P.check_grid_case(lib, case, CODES, _supers(case["k"]))


@pytest.mark.parametrize("n_bins", [1, 2000, P.S1_MAX_BINS])
def test_plain_parts_match_the_oracle_at_the_extremes_of_the_bin_count(lib, n_bins):
    case = dict(k=27, m=9, fmt="fq", eol=b"\n", max_x=3, both=True)
    P.check_grid_case(lib, case, CODES, P.S1_SK_TILE, n_bins=n_bins)


# ---- (b)
@pytest.mark.parametrize("k,m,both", P.PIECE_KM, ids=["k27-m9", "k27-m9-b", "k14-m11", "k256-m11"])
def test_piece_marks_of_over_long_lines_reach_the_cut(lib, k, m, both):
    """k_s1_check_records sets S1_PIECE_MARK, k_s1_cut<true> starts a run there (its has_marks branch)"""
    P.check_piece_part(lib, k, m, both, "fq", b"\n")
    P.check_piece_part(lib, k, m, both, "fa", b"\r\n")
    P.check_piece_part(lib, k, m, both, "fa", b"\n", cut_last=True)


@pytest.mark.parametrize("k,m,fmt", [(27, 9, "fa"), (27, 9, "fq"), (14, 11, "fq"), (256, 11, "fa")])
def test_long_read_parts_on_the_plain_path(lib, k, m, fmt):
    """k_s1_mark_raw sets the marks of a long-read part"""
    P.check_long_read_parts(lib, k, m, fmt, both=(fmt == "fa"))


# ---- (c)
@pytest.mark.parametrize("k,m,n_reads", [(5, 5, 60), (14, 11, 300)])
def test_the_second_cut_attempt_when_the_first_guess_is_short(lib, k, m, n_reads):
    """s1_split_part sizes the super-k-mer arrays by guess, and cuts again with the exact number when there were more"""
    P.check_retry(lib, k, m, n_reads)


# ---- (d)
@pytest.fixture
def sorted_emit(monkeypatch):
    monkeypatch.setenv("KMC_HIP_S1_SORTED_EMIT", "1")  # the library reads the variable on every call


def test_sorted_emit_writes_the_pieces_of_over_long_lines_in_read_order(lib, sorted_emit):
    P.check_piece_part(lib, 27, 9, True, "fq", b"\n", exact=True)


@pytest.mark.parametrize("k,m", [(14, 11), (256, 11)])
def test_sorted_emit_writes_every_bin_in_read_order(lib, sorted_emit, k, m):
    case = next(c for c in P.grid_cases() if (c["k"], c["m"]) == (k, m))
    P.check_grid_case(lib, case, CODES, _supers(k), exact=True)


@pytest.mark.parametrize("n_bins", [1, 2000])
def test_sorted_emit_over_several_tiles_of_super_k_mers(lib, sorted_emit, n_bins):
    """more than three tiles of k_s1_emit_sorted: its look-back walks; one bin (every record relative to cum_bytes[0]) and 2000 (nearly every record another bin)"""
    text, k, m = P.sorted_walk_text(3 * P.S1_TILE)
    want = P.check_plain(lib, text, 1, k, 1 << 17, m=m, n_bins=n_bins, exact=True)
    assert int(want["supers"].sum()) > 3 * P.S1_TILE
