"""GPU: a globally ordered database from planted bins (kmc_hip_order_database_device) — the cases of tests/test_order_db_emulated.py on the device: every record
width (SIZE 1..7), the LUT prefix across a 64-bit word boundary on either side, empty and single-record bins, 0 / 1 / 2 records, every counter width; and the raw
KMC2 fixture against what the reference's `transform sort` made of it. Reads tests/golden only."""
import numpy as np
import pytest

import order_cases as R
import setops_cases as S
from kmc_amd import capi, dbio

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_order_database_on_planted_bins(ctx, case):
    R.check_case(ctx, case)


@pytest.mark.parametrize("k", sorted(S.RAW_A))
def test_a_raw_kmc2_database_is_ordered_into_what_transform_sort_writes(ctx, k):
    raw, want = dbio.read_database(S.golden_path(k, S.RAW_A[k])), S.golden_db(k, "a")
    assert raw.kmc2 and not want.kmc2 and S.straddles(k, raw.lut_prefix_len) and S.straddles(k, want.lut_prefix_len)
    hparams = capi.make_params(k, both_strands=int(raw.both_strands), cutoff_min=raw.min_count, cutoff_max=raw.max_count, counter_max=(1 << (8 * raw.counter_size)) - 1,
                               lut_prefix_len=raw.lut_prefix_len)
    out, lut, n = R.order_database_on_device(ctx, hparams, raw.bins, want.lut_prefix_len)
    assert n == want.total_kmers
    assert np.array_equal(out, want.recs) and np.array_equal(lut, want.lut)
