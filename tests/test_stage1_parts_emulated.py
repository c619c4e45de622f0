"""CPU: plain FASTA / FASTQ parts — kmc_hip_split_part with file_type 0 or 1 and no flags, the call kmc_hip_s1 makes for nearly every part — through THE
PRODUCT'S host library compiled over the emulated HIP runtime (tests/emu.py build_hostlib), against the reference's GetSeq + ProcessReads restatement.
The cases of tests/stage1_part_cases.py at the small geometry's sizes (a cutting window of 2048 positions, 64 super-k-mers per scatter tile): the
(k, m) grid with its narrow and wide minimum windows, piece marks reaching the cut, the second cut attempt, the sorted emit. tests/test_gpu_stage1_parts.py
runs the same cases on the device."""
import pytest

import emu
import stage1_part_cases as P
from test_stage1_hc_emulated import HcLib

CODES = 3 * 2048  # three cutting windows of the small geometry
SUPERS = 2 * 64   # two scatter tiles of the small geometry


@pytest.fixture(scope="module")
def hostlib():
    lib = HcLib(emu.build_hostlib("small"))
    yield lib
    lib.close()


# ---- (a)
@pytest.mark.parametrize("case", P.grid_cases(), ids=P.grid_ids())
def test_plain_parts_match_the_oracle_over_k_and_signature_length(hostlib, case):
    P.check_grid_case(hostlib, case, CODES, SUPERS)


@pytest.mark.parametrize("n_bins", [1, 2000, P.S1_MAX_BINS])
def test_plain_parts_match_the_oracle_at_the_extremes_of_the_bin_count(hostlib, n_bins):
    case = dict(k=27, m=9, fmt="fq", eol=b"\n", max_x=3, both=True)
    P.check_grid_case(hostlib, case, CODES, SUPERS, n_bins=n_bins)


# ---- (b)
@pytest.mark.parametrize("k,m,both", P.PIECE_KM, ids=["k27-m9", "k27-m9-b", "k14-m11", "k256-m11"])
def test_piece_marks_of_over_long_lines_reach_the_cut(hostlib, k, m, both):
    """k_s1_check_records sets S1_PIECE_MARK, k_s1_cut<true> starts a run there (its has_marks branch)"""
    P.check_piece_part(hostlib, k, m, both, "fq", b"\n")
    P.check_piece_part(hostlib, k, m, both, "fa", b"\r\n")
    P.check_piece_part(hostlib, k, m, both, "fa", b"\n", cut_last=True)


@pytest.mark.parametrize("k,m,fmt", [(27, 9, "fa"), (27, 9, "fq"), (14, 11, "fq"), (256, 11, "fa")])
def test_long_read_parts_on_the_plain_path(hostlib, k, m, fmt):
    """k_s1_mark_raw sets the marks of a long-read part"""
    P.check_long_read_parts(hostlib, k, m, fmt, both=(fmt == "fa"))


# ---- (c)
def test_the_second_cut_attempt_when_the_first_guess_is_short(hostlib):
    """s1_split_part sizes the super-k-mer arrays by guess, and cuts again with the exact number when there were more"""
    P.check_retry(hostlib, 5, 5, 60)


# ---- (d)
@pytest.fixture
def sorted_emit(monkeypatch):
    monkeypatch.setenv("KMC_HIP_S1_SORTED_EMIT", "1")  # the library reads the variable on every call


def test_sorted_emit_writes_the_pieces_of_over_long_lines_in_read_order(hostlib, sorted_emit):
    P.check_piece_part(hostlib, 27, 9, True, "fq", b"\n", exact=True)


@pytest.mark.parametrize("k,m", [(14, 11), (256, 11)])
def test_sorted_emit_writes_every_bin_in_read_order(hostlib, sorted_emit, k, m):
    case = next(c for c in P.grid_cases() if (c["k"], c["m"]) == (k, m))
    P.check_grid_case(hostlib, case, CODES, SUPERS, exact=True)


@pytest.mark.parametrize("n_bins", [1, 2000])
def test_sorted_emit_over_several_tiles_of_super_k_mers(hostlib, sorted_emit, n_bins):
    """more than three tiles of k_s1_emit_sorted: its look-back walks; one bin (every record relative to cum_bytes[0]) and 2000 (nearly every record another bin)"""
    text, k, m = P.sorted_walk_text(3 * P.S1_TILE)
    want = P.check_plain(hostlib, text, 1, k, 1 << 17, m=m, n_bins=n_bins, exact=True)
    assert int(want["supers"].sum()) > 3 * P.S1_TILE
