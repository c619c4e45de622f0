"""GPU (-m gpu): every record width, 1 to 8 words (k = 32, 64, ..., 256), through the three stage-2 entries that dispatch on it — kmc_hip_process_bins_device,
kmc_hip_debug_expand and kmc_hip_debug_compact — byte for byte against the oracle. A width routed to its neighbour reads and writes records at the wrong stride
and fails at once; a few hundred reads per width is the smallest input that still fills more than one tile of the small records.

The widths of the database family (1 to 7) are in test_gpu_order_db.py, test_gpu_db_setops.py, test_gpu_db_query.py and test_gpu_db_transform.py.

The bins are those of tests/hostlib_sanitize_case.py. Its reads are 150 symbols long, and the model makes no read shorter than k: from k = 128 on the reads are
k + 50 symbols long, so that every width gets bins of several thousand k-mers."""
import numpy as np
import pytest

import oracle_py as O
from kmc_amd import capi
from test_gpu_parity import _first_diff, _run_batch, op

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", list(range(32, 257, 32)))
def test_every_record_width_through_the_stage2_dispatchers(ctx, k):
    assert (k + 31) // 32 == k // 32  # k / 32 words: the last bit of the last word is in use
    bins = capi.synth_bins(seed=7, genome_len=3000, n_reads=300, k=k, n_bins=2, n_threads=1, read_len=max(150, k + 50))
    assert all(b[1] > 2000 for b in bins), [b[1] for b in bins]
    p = capi.make_params(k, lut_prefix_len=4)
    want = [O.process_bin(op(p), img, nrec) for img, nrec, _, _ in bins]
    # kmc_hip_process_bins_device: both bins in one call (run_group_device)
    got, err = _run_batch(ctx, p, bins, 1)
    assert err is None, err
    for i, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(("out", "lut", "stats"), g, w):
            assert np.array_equal(a, b), (i, name, _first_diff(a, b))
    # the two test hooks, on the first bin: the records of the expansion, and the oracle's sorted records through the compaction
    img, nrec, packs, _ = bins[0]
    recs = O.expand(op(p), img)
    assert recs.shape == (nrec, k // 32)
    exp = ctx.debug_expand(p, img, nrec, packs)
    assert np.array_equal(exp, recs), _first_diff(exp, recs)
    for name, a, b in zip(("out", "lut", "stats"), ctx.debug_compact(p, O.sort(recs)), want[0]):
        assert np.array_equal(a, b), (name, _first_diff(a, b))
