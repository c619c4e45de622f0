"""A globally ordered database from the bins of stage 2 (kmc_hip_order_database_device, what `kmc_tools transform <db> sort <out>` does): planted bins whose
expected output is setops_cases.encode_body — the restatement tests/test_db_setops_emulated.py pins to the bytes kmc_tools writes — of all their k-mers, and the
helper that drives the call. No live reference is needed. TEST INFRASTRUCTURE shared by tests/test_order_db_emulated.py, tests/test_gpu_order_db.py and
tests/test_gpu_parity.py."""
from __future__ import annotations

import numpy as np

import setops_cases as S
from kmc_amd import capi


def order_database_on_device(ctx, hparams, bins, p_out):
    """bins: [(record bytes, LUT counts)] -> (records bytes, LUT, records) of kmc_hip_order_database_device"""
    rb = ctx.out_rec_bytes(hparams)
    n = len(bins)
    descs = (capi.BinDesc * n)()
    allocs = []
    total = 0
    for i, (recs, lut) in enumerate(bins):
        d_out, d_lut, d_small = ctx.malloc(recs.size + 256), ctx.malloc(lut.nbytes), ctx.malloc(64)
        if recs.size:
            ctx.h2d(d_out, recs)
        ctx.h2d(d_lut, lut)
        ctx.h2d(d_small, np.array([0, 0, 0, 0, recs.size, 0, 0, 0], dtype=np.uint64))
        allocs += [d_out, d_lut, d_small]
        descs[i] = capi.BinDesc(0, 0, 0, 0, 0, d_out, recs.size, d_small + 32, d_lut, d_small)
        total += recs.size // rb
    rb_out = (hparams.kmer_len - p_out) // 4 + (rb - (hparams.kmer_len - hparams.lut_prefix_len) // 4)
    d_res, d_lut_out = ctx.malloc(total * rb_out + 256), ctx.malloc(8 << (2 * p_out))
    got_n = ctx.order_database_device(hparams, descs, p_out, d_res, total * rb_out, d_lut_out)
    out = np.zeros(got_n * rb_out, dtype=np.uint8)
    lut = np.zeros(1 << (2 * p_out), dtype=np.uint64)
    if out.size:
        ctx.d2h(out, d_res)
    ctx.d2h(lut, d_lut_out)
    for a in allocs + [d_res, d_lut_out]:
        ctx.free(a)
    return out, lut, got_n


# counter bytes -> (cutoff_max, counter_max) of the bin parameters: MIN(BYTE_LOG(cutoff_max), BYTE_LOG(counter_max)), none at counter_max == 1 (defs.h:154-159).
# 2 and 4 are decided by cutoff_max, 1 and 3 by counter_max
COUNTER_PARAMS = {0: (10**9, 1), 1: (10**9, 255), 2: (65535, S.U32), 3: (S.U32, (1 << 24) - 1), 4: (S.U32, S.U32)}


def bin_params(k, p_in, cbytes):
    cx, cs = COUNTER_PARAMS[cbytes]
    return capi.make_params(k, lut_prefix_len=p_in, cutoff_min=1, cutoff_max=cx, counter_max=cs)


def bin_of(x, n_live):
    """the fixed hash that deals a k-mer into one of n_live bins (a signature's stand-in: any partition of the k-mers will do)"""
    return ((x ^ (x >> 29) ^ (x >> 61)) * 0x9E3779B97F4A7C15 >> 17) % n_live


def deal(k, p_in, cbytes, kmers, counts, n_bins, empty=(), single=None):
    """kmers: ascending, distinct. -> [(record bytes, LUT COUNTS)] per bin as stage 2 leaves them: records ascending inside the bin, (suffix big-endian, counter
    little-endian) for p_in, and how many records every prefix has. empty: bins that get nothing; single: a bin that gets exactly one record (the first k-mer)"""
    live = [b for b in range(n_bins) if b not in empty and b != single]
    sb, bits = (k - p_in) // 4, 2 * (k - p_in)
    per_bin = [[] for _ in range(n_bins)]
    for i, (x, c) in enumerate(zip(kmers, counts)):
        per_bin[single if single is not None and i == 0 else live[bin_of(x, len(live))]].append((x, c))
    bins = []
    for members in per_bin:
        recs = b"".join((x & ((1 << bits) - 1)).to_bytes(sb, "big") + (c & ((1 << (8 * cbytes)) - 1)).to_bytes(cbytes, "little") for x, c in members)
        lut = np.bincount(np.array([x >> bits for x, _ in members], dtype=np.int64), minlength=1 << (2 * p_in)).astype(np.uint64)
        bins.append((np.frombuffer(recs, dtype=np.uint8).copy(), lut))
    return bins


N = 1500  # records of a case: at 4 bins several 256-thread blocks per bin

# widths and alignments: (k, p_in, p_out). Every SIZE 1..7; the prefix across a 64-bit word boundary on the input side, on the output side, on both, on neither
WIDTHS = [(33, 5, 9), (34, 6, 2), (35, 7, 7), (65, 9, 5), (97, 5, 1), (129, 1, 5), (161, 5, 5), (193, 9, 5),
          (27, 3, 7), (32, 4, 8), (64, 8, 4), (96, 4, 4), (128, 4, 8), (160, 8, 4), (192, 4, 4), (224, 4, 4)]
assert {(k + 31) // 32 for k, _, _ in WIDTHS} == set(range(1, 8))
assert all(S.straddles(k, pi) for k, pi, _ in WIDTHS[:8] if k != 129) and all(S.straddles(k, po) for k, _, po in WIDTHS[:8] if k not in (34, 97))
assert not S.straddles(129, 1) and not S.straddles(34, 2) and not S.straddles(97, 1) and not any(S.straddles(k, pi) or S.straddles(k, po) for k, pi, po in WIDTHS[8:])

# (name, k, p_in, p_out, counter bytes, n_bins, dict(n, empty, single, where: None | "first" | "last" | "middle" prefix of the wider LUT))
# (a bin with a LUT of 4^9 entries costs the emulated k_db_cumsum seconds: the two widths that read one take 2 bins, and no other case reads one)
CASES = [(f"k{k}_p{pi}_to_p{po}", k, pi, po, 1 + (k & 1), 4 if pi < 9 else 2, {}) for k, pi, po in WIDTHS] + [
    ("one_bin", 33, 5, 5, 1, 1, {}),
    ("four_bins_first_and_last_empty", 33, 5, 9, 1, 4, dict(empty=(0, 3))),
    ("nine_bins_first_middle_last_empty", 35, 7, 3, 2, 9, dict(empty=(0, 4, 8))),
    ("nine_bins_one_of_a_single_record", 65, 5, 9, 1, 9, dict(empty=(5,), single=2)),
    ("first_prefix", 33, 5, 9, 1, 4, dict(where="first")),
    ("last_prefix", 35, 7, 3, 1, 4, dict(where="last")),
    ("middle_prefix", 97, 5, 9, 1, 4, dict(where="middle")),
    ("last_prefix_seven_words", 193, 5, 9, 2, 4, dict(where="last")),
    ("no_records_one_bin", 33, 5, 5, 1, 1, dict(n=0)),
    ("no_records_four_bins", 55, 3, 7, 1, 4, dict(n=0)),
    ("one_record", 33, 5, 9, 1, 4, dict(n=1)),
    ("two_records", 33, 5, 1, 1, 4, dict(n=2)),
    ("two_records_one_bin", 129, 5, 9, 2, 1, dict(n=2)),
] + [(f"counter_bytes_{cb}_k{k}", k, pi, po, cb, 4, {}) for cb, (k, pi, po) in enumerate([(33, 5, 5), (27, 3, 7), (65, 5, 9), (33, 5, 1), (161, 5, 9)])]
CASE_IDS = [c[0] for c in CASES]


def make_case(case, seed=3):
    """-> (bin parameters, bins, k-mers, counts): k-mers ascending with the k-mer 0 and the all-ones k-mer among them where the case leaves them room, counts up to
    the top of the counter width"""
    name, k, p_in, p_out, cb, n_bins, kw = case
    rng = np.random.default_rng(seed + k + 7 * cb + len(name))
    n, where = kw.get("n", N), kw.get("where")
    pw = max(p_in, p_out)
    pref = {None: None, "first": 0, "last": (1 << (2 * pw)) - 1, "middle": (1 << (2 * pw)) // 3}[where]
    ends = [x for x, on in ((0, where in (None, "first")), ((1 << (2 * k)) - 1, where in (None, "last"))) if on][: n]
    kmers = sorted(set(S.random_kmers(rng, k, n, lo_prefix=pref, p=pw)[: n - len(ends)]) | set(ends)) if n else []
    top = (1 << (8 * cb)) - 1
    counts = [max(top - int(x), 1) if i % 3 == 0 else int(x) + 1 for i, x in enumerate(rng.integers(0, min(top, 200) + 1, size=len(kmers)))] if cb else [1] * len(kmers)
    counts[: 2] = [top or 1, max(top - 1, 1)][: len(counts)]
    return bin_params(k, p_in, cb), deal(k, p_in, cb, kmers, counts, n_bins, kw.get("empty", ()), kw.get("single")), kmers, counts


def check_case(ctx, case):
    """the device call on the planted bins must equal the restatement: records, LUT and the returned count"""
    name, k, p_in, p_out, cb, n_bins, kw = case
    hparams, bins, kmers, counts = make_case(case)
    assert ctx.out_rec_bytes(hparams) == (k - p_in) // 4 + cb and len(bins) == n_bins and sum(int(b[1].sum()) for b in bins) == len(kmers)
    for e in kw.get("empty", ()):
        assert bins[e][0].size == 0
    if "single" in kw:
        assert int(bins[kw["single"]][1].sum()) == 1
    if "n" not in kw:
        assert len(kmers) >= N - 2 and sum(b[0].size > 0 for b in bins) == n_bins - len(kw.get("empty", ()))
    want_lut, want_recs = S.encode_body(k, p_out, cb, kmers, counts)
    out, lut, n = order_database_on_device(ctx, hparams, bins, p_out)
    assert n == len(kmers), (n, len(kmers))
    assert np.array_equal(out, want_recs), "records differ"
    assert np.array_equal(lut, want_lut), "LUT differs"
