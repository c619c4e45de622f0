"""KFF output (kmc_hip_db_kff_export_device, kmc_amd/dbio.write_kff, `python -m kmc_amd.tools export`, `count` with output_format="kff"): the recorded reference files
tests/golden/kffout_*.kff and the command lines that made them, the planted bodies, and the helpers that run the entry. The oracle for a record is
kff_cases.encode_records, for the container kff_cases.encode_container — both pinned to the reference's own files by tests/test_kff_emulated.py. TEST INFRASTRUCTURE
shared by tests/make_kffout_golden.py, tests/test_kff_export_emulated.py and tests/test_gpu_kff_export.py."""
from __future__ import annotations

import os

import numpy as np

import kff_cases as K
import setops_cases as S
import transform_cases as T

GOLDEN = K.GOLDEN
U32 = K.U32
EINVAL, ECORRUPT, ECAPACITY = K.EINVAL, K.ECORRUPT, K.ECAPACITY
THREADS = K.THREADS  # KFF_THREADS
GUARD = K.GUARD

# ---- the recorded files: name -> the arguments of `kmc_tools -t1 -hp transform ...`; `export` takes the same line without `reduce` and `-okff`
FILES = {
    "kffout_k27_bounds": ["{g}/setops_k27_a", "reduce", "{out}", "-ci3", "-cx20", "-cs10", "-okff"],  # output bounds
    "kffout_k55_inbounds": ["{g}/setops_k55_a", "-ci2", "-cx50", "reduce", "{out}", "-okff"],  # input bounds
    "kffout_k33_cs3": ["{g}/setops_k33_a", "reduce", "{out}", "-cs70000", "-okff"],  # counters wider than the input's
    "kffout_k33_raw": ["{g}/setops_k33_raw_a", "reduce", "{out}", "-okff"],  # a KMC2 input: reduce orders it
    "kffout_k27_multi": ["{g}/kff_k27_multi.kff", "reduce", "{out}", "-okff"],  # 58 sections to one; the twin of `count -k27 -ci1 -p5 count_k27_fq.fq` as KFF
    "kffout_k27_empty": ["{g}/setops_k27_a", "reduce", "{out}", "-ci250", "-okff"],  # an output without records
}
# the files recorded with the import (kff_cases.FILES) are outputs of the same kind: name -> what `export` takes
OLD_FILES = {
    "kff_k27_a": ["{g}/setops_k27_a", "{out}"], "kff_k33_a": ["{g}/setops_k33_a", "{out}"], "kff_k55_a": ["{g}/setops_k55_a", "{out}"],
    "kff_k27_a_cs2": ["{g}/setops_k27_a", "{out}", "-cs65535"],
}
# what the new files hold (make_kffout_golden.py asserts it): k, data_size, records (None: not pinned here), min_count, max_count
FILE_SHAPES = {"kffout_k27_bounds": (27, 1, None, 3, 20), "kffout_k55_inbounds": (55, 1, None, 2, 50), "kffout_k33_cs3": (33, 3, 8473, None, None),
               "kffout_k33_raw": (33, 1, 8473, None, None), "kffout_k27_multi": (27, 1, 2140, 1, 10**9), "kffout_k27_empty": (27, 1, 0, 250, None)}
COUNT_ARGV = ["-k27", "-ci1", "-p5"]  # + the input (tests/golden/count_k27_fq.fq) and the output: the flags kff_k27_multi.kff was counted with


def kff_file(name):
    return os.path.join(GOLDEN, name + ".kff")


def reference_argv(name, out):
    return ["transform"] + [a.format(g=GOLDEN, out=out) for a in FILES[name]]


def export_argv(name, out):
    args = OLD_FILES[name] if name in OLD_FILES else [a for a in FILES[name] if a not in ("reduce", "-okff")]
    return [a.format(g=GOLDEN, out=out) for a in args]


# ---- the geometry
def default_ipt(k, p, cs, ds):
    """kff_default_ipt over the export's two records: (k - p) / 4 + cs bytes in, ceil(k / 4) + ds bytes out, both images of the tile in 32 KiB of LDS, at most 8; then
    lowered while ipt records of either image are a multiple of 64 bytes (the entry avoids that distance between neighbouring lanes: LDS banks)"""
    rb_in, rb_out = (k - p) // 4 + cs, (k + 3) // 4 + ds
    ipt = max(1, min(8, 32 * 1024 // (THREADS * (rb_in + rb_out))))
    while ipt > 1 and ((ipt * rb_in) % 64 == 0 or (ipt * rb_out) % 64 == 0):
        ipt -= 1
    return ipt


def tile_records(k, p, cs, ds=None, ipt=None):
    return THREADS * (ipt or default_ipt(k, p, cs, cs if ds is None else ds))


# ---- the device call
class ExportContext(K.KffContext):
    """K.KffContext (set operations, transform, KFF import) with the counting session and kmc_hip_db_kff_export_device: the interface of capi.Context on a library given by path"""

    def __init__(self, path):
        super().__init__(path)
        C, capi = self.C, self.capi
        vp = C.c_void_p
        capi.bind_count(self.L)
        self.L.kmc_hip_split_covers.argtypes = [C.c_uint32]
        self.L.kmc_hip_db_kff_export_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, vp, C.c_uint64]


def _bind():
    from kmc_amd import capi

    ExportContext.db_kff_export_device = capi.Context.db_kff_export_device  # the binding under test is the one the product ships


_bind()


def run_export(ctx, k, p, cs, lut, recs, n_seg=1, first=0, count=None, ds=None, in_off=0, out_off=0, capacity=None) -> bytes:
    """The body (lut, recs) uploaded — d_recs in_off bytes and d_kff out_off bytes behind an aligned address — and records [first, first + count) framed with data_size
    ds. d_kff lies between guard bytes that must come back intact. -> the KFF record bytes"""
    from kmc_amd import capi

    recs, lut = np.asarray(recs, dtype=np.uint8), np.asarray(lut, dtype=np.uint64)
    rb_in, ds = (k - p) // 4 + cs, cs if ds is None else ds
    rb_out = (k + 3) // 4 + ds
    n = recs.size // rb_in
    count = n - first if count is None else count
    cap = count * rb_out if capacity is None else capacity
    obuf = np.full(64 + out_off + cap + 64, GUARD, dtype=np.uint8)
    allocs = [ctx.malloc(in_off + recs.size + 256), ctx.malloc(lut.nbytes + 256), ctx.malloc(obuf.size + 256)]
    try:
        if recs.size:
            ctx.h2d(allocs[0] + in_off, np.ascontiguousarray(recs))
        ctx.h2d(allocs[1], np.ascontiguousarray(lut))
        ctx.h2d(allocs[2], obuf)
        view = capi.DbView(allocs[0] + in_off, n, allocs[1], p, cs, 0xDEAD, 3)  # cutoffs that would cut everything: the entry does not read them
        got = ctx.db_kff_export_device(k, view, n_seg, first, count, ds, allocs[2] + 64 + out_off, cap)
        assert got == count * rb_out
        ctx.d2h(obuf, allocs[2])
        assert np.all(obuf[:64 + out_off] == GUARD) and np.all(obuf[64 + out_off + got:] == GUARD), "bytes outside the records were written"
        return obuf[64 + out_off:64 + out_off + got].tobytes()
    finally:
        for d in allocs:
            ctx.free(d)


def mask(counts, cs):
    return [c & ((1 << (8 * cs)) - 1) for c in counts]


def ordered_body(k, p, cs, sections):
    """the sections' records as one ascending body -> (lut, recs, kmers, counts)"""
    pairs = sorted((x, c) for ks, cc in sections for x, c in zip(ks, mask(cc, cs)))
    kmers, counts = [x for x, _ in pairs], [c for _, c in pairs]
    return (*S.encode_body(k, p, cs, kmers, counts), kmers, counts)


def segmented_body(k, p, cs, sections):
    """the sections as the bins of a KMC2 body in file order -> (lut with the closing entry, recs, kmers, counts)"""
    secs = [(ks, mask(cc, cs)) for ks, cc in sections]
    return (*T.encode_segmented(k, p, cs, secs), [x for ks, _ in secs for x in ks], [c for _, cc in secs for c in cc])


def check_export(ctx, k, p, cs, lut, recs, kmers, counts, n_seg=1, ds=None, **kw):
    got = run_export(ctx, k, p, cs, lut, recs, n_seg=n_seg, ds=ds, **kw)
    first = kw.get("first", 0)
    count = kw.get("count")
    count = len(kmers) - first if count is None else count
    assert got == K.encode_records(k, cs if ds is None else ds, kmers[first:first + count], counts[first:first + count]), "KFF records differ"
    return got


def round_trips(ctx, k, p, cs, sections):
    """import(export(body)) is the body and its LUT in both `ordered` modes, and export(import(KFF records)) is the KFF records — for the sections as one ascending body
    and, where there is a section, as a segmented body in file order"""
    lut, recs, kmers, counts = ordered_body(k, p, cs, sections)
    kff = check_export(ctx, k, p, cs, lut, recs, kmers, counts)
    lut1, recs1 = K.run_import(ctx, k, cs, p, kff, [len(kmers)], True)
    assert np.array_equal(lut1, lut) and np.array_equal(recs1, recs), "ordered body: import(export) with ordered = 1 differs"
    lut0, recs0 = K.run_import(ctx, k, cs, p, kff, [len(kmers)], False)
    assert np.array_equal(lut0[:-1], lut) and int(lut0[-1]) == len(kmers) and np.array_equal(recs0, recs), "ordered body: import(export) with ordered = 0 differs"
    assert run_export(ctx, k, p, cs, lut1, recs1) == kff, "ordered body: export(import) differs"
    if not sections:
        return
    slut, srecs, skmers, scounts = segmented_body(k, p, cs, sections)
    sec_n = [len(ks) for ks, _ in sections]
    skff = check_export(ctx, k, p, cs, slut, srecs, skmers, scounts, n_seg=len(sections))
    lut0, recs0 = K.run_import(ctx, k, cs, p, skff, sec_n, False)
    assert np.array_equal(lut0, slut) and np.array_equal(recs0, srecs), "segmented body: import(export) with ordered = 0 differs"
    if len(set(skmers)) == len(skmers):
        lut1, recs1 = K.run_import(ctx, k, cs, p, skff, sec_n, True)
        assert np.array_equal(lut1, lut) and np.array_equal(recs1, recs), "segmented body: import(export) with ordered = 1 differs"
    assert run_export(ctx, k, p, cs, lut0, recs0, n_seg=len(sections)) == skff, "segmented body: export(import) differs"


# ---- planted bodies
WIDTHS = [(27, 3), (28, 4), (32, 4), (33, 5), (33, 9), (64, 4), (127, 3), (224, 4)]
WIDTH_IDS = [f"{k}-p{p}" for k, p in WIDTHS]
WIDEST = (33, 9)  # the widest LUT of the list: 4^9 entries


def prefix_change_cases(k, p, tile, seed=23):
    """-> [(name, data_size, sections)]: one section whose prefix changes exactly on a tile seam, one record to either side of it, on a wave seam and on a wave seam
    of the second tile — between neighbouring prefixes and between the first and the last one (a walk of one entry, and one that must give up)"""
    rng = np.random.default_rng(seed + 5 * k + p)
    n_pref = 1 << (2 * p)
    n = 2 * tile + 70
    cases = []
    for where, at in (("tile_seam", tile), ("before_tile_seam", tile - 1), ("behind_tile_seam", tile + 1), ("wave_seam", 64), ("wave_seam_second_tile", tile + 128)):
        for far, (a, b) in (("near", (n_pref // 2, n_pref // 2 + 1)), ("far", (0, n_pref - 1))):
            ks = S.random_kmers(rng, k, at, lo_prefix=a, p=p) + S.random_kmers(rng, k, n - at, lo_prefix=b, p=p)
            cases.append((f"prefix_change_{where}_{far}", 1, [(ks, K.edge_counts(1, n, at))]))
    # a new prefix with every record around the tile seam: the walk takes one step per record
    base = max(0, n_pref // 2 - 8)
    span = min(n_pref - base, 16)
    ks = S.random_kmers(rng, k, tile - span // 2, lo_prefix=base, p=p)
    for i in range(1, span):
        ks += S.random_kmers(rng, k, 1, lo_prefix=base + i, p=p)
    ks = sorted(set(ks + S.random_kmers(rng, k, 40, lo_prefix=base + span - 1, p=p)))
    cases.append(("a_prefix_per_record_across_the_tile_seam", 2, [(ks, K.edge_counts(2, len(ks)))]))
    return cases


def planted_cases(k, p, tile):
    """kff_cases.planted_cases (3 1/3 tiles at every counter width with counters at the byte edges, one tile, one record, no record, all records under the first, the last
    or one middle prefix, five records, 2 / 7 / 300 sections with empty ones at the front, in the middle and at the end) and the prefix changes above"""
    return K.planted_cases(k, p, tile) + prefix_change_cases(k, p, tile)
