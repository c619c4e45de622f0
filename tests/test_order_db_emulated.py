"""CPU: a globally ordered database from planted bins (kmc_hip_order_database_device: k_db_cumsum, k_db_unpack, the library's stable LSD passes, k_db_pack) in the
PRODUCT'S host library compiled over the emulated HIP runtime (tests/emu.py build_hostlib, small geometry) — every record width (SIZE 1..7), the LUT prefix across a
64-bit word boundary on either side, empty and single-record bins, 0 / 1 / 2 records, every counter width. The oracle is setops_cases.encode_body of all the k-mers
(tests/order_cases.py); nothing here needs oracle/_ref. The -m gpu file tests/test_gpu_order_db.py runs the same cases on the device."""
import numpy as np
import pytest

import emu
import order_cases as R
import setops_cases as S
from kmc_amd import dbio


@pytest.fixture(scope="module")
def lib():
    c = S.LibContext(emu.build_hostlib("small"))
    yield c
    c.close()


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_order_database_on_planted_bins(lib, case):
    R.check_case(lib, case)


def test_the_planted_bins_are_what_they_claim():
    """the helper against itself: every bin's records decode (with the bin's own LUT sums) to the k-mers dealt into it, ascending, and the bins partition the k-mers"""
    case = R.CASES[R.CASE_IDS.index("nine_bins_one_of_a_single_record")]
    _, k, p_in, _, cb, _, _ = case
    _, bins, kmers, counts = R.make_case(case)
    seen = {}
    for recs, lut in bins:
        sums = np.concatenate([[0], np.cumsum(lut)[:-1]]).astype(np.uint64)
        ks, cs = S.decode_body(k, p_in, cb, sums, recs)
        assert ks == sorted(ks) and not set(ks) & set(seen)
        seen.update(zip(ks, cs))
    assert seen == dict(zip(kmers, counts)) and kmers[0] == 0 and kmers[-1] == (1 << (2 * k)) - 1


@pytest.mark.parametrize("k", sorted(S.RAW_A))
def test_a_raw_kmc2_database_is_ordered_into_what_transform_sort_writes(lib, k):
    """the database `kmc` wrote (tests/golden/setops_k<k>_raw_a, read by dbio) through the device call == the database the reference's `kmc_tools transform sort`
    made of it (setops_k<k>_a), byte for byte. k = 33: lut_prefix_len 5 on both sides, across the word boundary"""
    raw, want = dbio.read_database(S.golden_path(k, S.RAW_A[k])), S.golden_db(k, "a")
    assert raw.kmc2 and not want.kmc2 and raw.counter_size == want.counter_size and S.straddles(k, raw.lut_prefix_len) and S.straddles(k, want.lut_prefix_len)
    assert sum(b[0].size > 0 for b in raw.bins) > 8 and sum(int(b[1].sum()) for b in raw.bins) == raw.total_kmers == want.total_kmers
    hparams = R.capi.make_params(k, both_strands=int(raw.both_strands), cutoff_min=raw.min_count, cutoff_max=raw.max_count, counter_max=(1 << (8 * raw.counter_size)) - 1,
                                 lut_prefix_len=raw.lut_prefix_len)
    out, lut, n = R.order_database_on_device(lib, hparams, raw.bins, want.lut_prefix_len)
    assert n == want.total_kmers
    assert np.array_equal(out, want.recs) and np.array_equal(lut, want.lut)
