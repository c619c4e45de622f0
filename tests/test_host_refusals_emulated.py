"""CPU: what the host layer of the PRODUCT'S library refuses, entry by entry — the return code and the entry's name in kmc_hip_last_error, from tables — in the host
library compiled over the emulated HIP runtime (tests/emu.py build_hostlib, small geometry).

The five database entries share one check of a kmc_hip_db_view, the two stage-1 part entries one preamble, the estimator and the small-k table one accumulator:
these tables hold every entry to the same refusals, so that one `kmc_tools` operation cannot take a database another refuses, nor small k a part the bin path
takes. Refusals with a test of their own elsewhere (NULL arguments, the capacities, the operations' own parameters: test_db_*_emulated.py, test_stage1_*_emulated.py)
are not repeated."""
import ctypes as C

import numpy as np
import pytest

import emu
from kmc_amd import capi

EINVAL, ECORRUPT = -1, -4
vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
S1_WG_TILE = 1024 * int(next(f for f in emu.GEOMETRY_FLAGS["small"] if f.startswith("-DS1_SUB_N=")).split("=")[1])  # stage1_kernels.hip.h: S1_TILE x S1_SUB


class Lib:
    def __init__(self, path):
        L = self.L = C.CDLL(path)
        L.kmc_hip_init.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
        L.kmc_hip_destroy.argtypes = [vp]
        L.kmc_hip_destroy.restype = None
        L.kmc_hip_last_error.argtypes = [vp]
        L.kmc_hip_last_error.restype = C.c_char_p
        L.kmc_hip_malloc.argtypes = [vp, C.c_int, C.c_uint64, C.POINTER(vp)]
        L.kmc_hip_free.argtypes = [vp, C.c_int, vp]
        L.kmc_hip_memcpy_h2d.argtypes = [vp, C.c_int, vp, vp, C.c_uint64]
        L.kmc_hip_db_set_op_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.POINTER(capi.DbView), C.POINTER(capi.DbOp), vp, C.c_uint64, vp, u64p, u64p]
        L.kmc_hip_db_query_reads_device.argtypes = [vp, C.c_int, C.POINTER(capi.DbView), C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32, vp, vp, vp, vp, u64p]
        L.kmc_hip_db_reduce_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, u64p, u64p]
        L.kmc_hip_db_histogram_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.c_uint32, C.c_uint32, C.c_uint64, vp, u64p]
        L.kmc_hip_db_dump_device.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(capi.DbView), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, vp, C.c_uint64, u64p, u64p]
        L.kmc_hip_split_set_map.argtypes = [vp, C.c_int, vp, C.c_uint32]
        L.kmc_hip_split_part.argtypes = [vp, C.c_int, C.c_int, C.POINTER(capi.SplitParams), vp, C.c_uint64, vp, C.c_uint64] + [vp] * 7
        L.kmc_hip_smallk_part.argtypes = [vp, C.c_int, C.c_int, C.POINTER(capi.SplitParams), vp, C.c_uint64, vp, vp]
        L.kmc_hip_estimate_open.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]
        L.kmc_hip_smallk_open.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32]
        for name in ("estimate", "smallk"):
            getattr(L, f"kmc_hip_{name}_read").argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, vp]
            getattr(L, f"kmc_hip_{name}_close").argtypes = [vp, C.c_int]
        self.h = vp()
        assert L.kmc_hip_init((C.c_int * 1)(0), 1, C.byref(self.h)) == 0
        self.allocs = []

    def close(self):
        for d in self.allocs:
            self.L.kmc_hip_free(self.h, 0, d)
        self.L.kmc_hip_destroy(self.h)

    def upload(self, a):
        a = np.ascontiguousarray(a)
        d = vp()
        assert self.L.kmc_hip_malloc(self.h, 0, max(a.nbytes, 8), C.byref(d)) == 0
        if a.nbytes:
            assert self.L.kmc_hip_memcpy_h2d(self.h, 0, d, a.ctypes.data, a.nbytes) == 0
        self.allocs.append(d.value)
        return d.value

    def error(self):
        return self.L.kmc_hip_last_error(self.h).decode()


@pytest.fixture(scope="module")
def lib():
    c = Lib(emu.build_hostlib("small"))
    yield c
    c.close()


# ---- 1: the five database entries and their views
N_RECS = 4
DB_ENTRIES = ("kmc_hip_db_set_op_device:a", "kmc_hip_db_set_op_device:b", "kmc_hip_db_query_reads_device", "kmc_hip_db_reduce_device", "kmc_hip_db_histogram_device",
              "kmc_hip_db_dump_device")


@pytest.fixture(scope="module")
def luts(lib):
    """device LUTs over N_RECS records, by name: sound ones of 4^p entries (every record under the last prefix), one whose last entry lies behind the records, and two of
    two segments with their closing entry: a sound one and one whose closing entry lies behind the records"""
    def lut(p, last, n_seg=1, closing=None):
        a = np.zeros((n_seg << (2 * p)) + (closing is not None), dtype=np.uint64)
        a[(n_seg << (2 * p)) - 1] = last
        if closing is not None:
            a[-1] = closing
        return lib.upload(a)

    out = {("ok", p): lut(p, N_RECS) for p in (1, 3, 4)}
    out["behind"] = lut(3, N_RECS + 1)
    out["seg_ok"] = lut(3, N_RECS, 2, N_RECS)
    out["seg_behind"] = lut(3, N_RECS, 2, N_RECS + 1)
    out["empty"] = lut(1, 0)
    for name in ("recs", "out", "lut_out"):  # records of zeros; room for every output of the sound calls
        out[name] = lib.upload(np.zeros(1 << 16, dtype=np.uint8))
    return out


def db_call(lib, luts, entry, k=27, p=3, cs=1, lut=None, n_seg=1, p_out=3, n_recs=N_RECS):
    """one call of `entry` on a view of n_recs records with the given prefix length, counter size and LUT; everything else is sound -> the return code"""
    L, h, d_recs, d, d_lut_out = lib.L, lib.h, luts["recs"], luts["out"], luts["lut_out"]
    d_lut = luts[("ok", p)] if lut is None else luts[lut]
    view = capi.DbView(d_recs, n_recs, d_lut, p, cs, 1, 255)
    n_out, st = C.c_uint64(), (C.c_uint64 * 8)()
    name, _, which = entry.partition(":")
    if name == "kmc_hip_db_set_op_device":
        q = next(q for q in (3, 4, 1) if (k - q) % 4 == 0)  # the other input: sound at this kmer_len
        other = capi.DbView(d_recs, n_recs, luts[("ok", q)], q, 1, 1, 255)
        a, b = (view, other) if which == "a" else (other, view)
        op = capi.DbOp(capi.DB_OPS["union"], capi.DB_COUNTER_OPS["sum"], 1, 255, 255, p_out)
        return L.kmc_hip_db_set_op_device(h, 0, k, C.byref(a), C.byref(b), C.byref(op), d, 1 << 16, d_lut_out, C.byref(n_out), st)
    if name == "kmc_hip_db_query_reads_device":
        return L.kmc_hip_db_query_reads_device(h, 0, C.byref(view), k, 1, None, 0, None, 0, 1, None, None, None, None, st)
    if name == "kmc_hip_db_reduce_device":
        return L.kmc_hip_db_reduce_device(h, 0, k, C.byref(view), 1, 255, 255, 0, p_out, d, 1 << 16, d_lut_out, C.byref(n_out), st)
    if name == "kmc_hip_db_histogram_device":
        return L.kmc_hip_db_histogram_device(h, 0, k, C.byref(view), n_seg, 1, 255, d, st)
    assert name == "kmc_hip_db_dump_device"
    return L.kmc_hip_db_dump_device(h, 0, k, C.byref(view), n_seg, 0, 0, 1, 255, 255, d, 1 << 16, C.byref(n_out), st)


VIEW_REFUSALS = [  # (id, arguments of db_call, code)
    ("counter_size_0", dict(cs=0), EINVAL),
    ("counter_size_5", dict(cs=5), EINVAL),
    ("prefix_not_a_multiple_of_4_below_k", dict(p=4), EINVAL),  # (27 - 4) % 4 != 0
    ("prefix_0", dict(k=28, p=0, p_out=4, lut=("ok", 1)), EINVAL),  # 28 % 4 == 0: the range alone refuses
    ("prefix_16", dict(k=28, p=16, p_out=4, lut=("ok", 1)), EINVAL),
    ("lut_ends_behind_the_records", dict(lut="behind"), ECORRUPT),
]


@pytest.mark.parametrize("entry", DB_ENTRIES)
@pytest.mark.parametrize("case", VIEW_REFUSALS, ids=[c[0] for c in VIEW_REFUSALS])
def test_every_database_entry_refuses_the_same_views(lib, luts, entry, case):
    _, kw, code = case
    assert db_call(lib, luts, entry) == 0, lib.error()  # the sound call the refused one differs from in one thing
    assert db_call(lib, luts, entry, **kw) == code
    assert entry.partition(":")[0] in lib.error()


@pytest.mark.parametrize("entry", DB_ENTRIES[:4])
def test_kmer_len_225_is_refused_where_records_are_unpacked(lib, luts, entry):
    """set operations, filter and reduce unpack records of (k + 31) / 32 + 1 words, 8 at most; histogram and dump read the packed records and take every k"""
    assert db_call(lib, luts, entry, k=221, p=1, p_out=1) == 0, lib.error()  # seven words: the widest there is
    assert db_call(lib, luts, entry, k=225, p=1, p_out=1) == EINVAL
    assert entry.partition(":")[0] in lib.error() and "224" in lib.error()


def test_histogram_takes_kmer_len_225(lib, luts):
    assert db_call(lib, luts, "kmc_hip_db_histogram_device", k=225, p=1, n_recs=0, lut="empty") == 0, lib.error()


@pytest.mark.parametrize("entry", ("kmc_hip_db_histogram_device", "kmc_hip_db_dump_device"))
def test_a_segmented_lut_is_checked_at_its_closing_entry(lib, luts, entry):
    assert db_call(lib, luts, entry, lut="seg_ok", n_seg=2) == 0, lib.error()
    assert db_call(lib, luts, entry, lut="seg_behind", n_seg=2) == ECORRUPT
    assert entry in lib.error()


@pytest.mark.parametrize("entry", ("kmc_hip_db_set_op_device:a", "kmc_hip_db_reduce_device"))
@pytest.mark.parametrize("k,p_out", [(27, 4), (28, 0), (28, 16)])
def test_the_output_prefix_is_held_to_the_rule_of_the_inputs(lib, luts, entry, k, p_out):
    p = 3 if k == 27 else 4
    assert db_call(lib, luts, entry, k=k, p=p, p_out=p) == 0, lib.error()
    assert db_call(lib, luts, entry, k=k, p=p, p_out=p_out) == EINVAL
    assert entry.partition(":")[0] in lib.error()


# ---- 2: the two stage-1 part entries, one list
K, M = 5, 5  # a k both entries take (small k: k <= 13; the bin path: signature_len <= k)
TEXT = b"".join(b">r%d\n" % i + b"ACGTTGCAAGGCTTAACCGT"[i % 7:] + b"\n" for i in range(12))
SOUND = dict(file_type=0, part_kind=0, line_cap=K + S1_WG_TILE + 2, flags=0, slot=0)  # line_cap: the smallest the entries take
PART_REFUSALS = [
    ("file_type_3", dict(file_type=3)),
    ("file_type_5", dict(file_type=5)),
    ("part_kind_2", dict(part_kind=2)),
    ("multiline_fasta_as_a_long_read", dict(file_type=2, part_kind=1)),
    ("bam_as_a_long_read", dict(file_type=4, part_kind=1)),
    ("line_cap_one_short", dict(line_cap=K + S1_WG_TILE + 1)),
    ("unknown_flag_bit_1", dict(flags=2)),
    ("unknown_flag_bit_7", dict(flags=0x80)),
    ("slot_below", dict(slot=-1)),
    ("slot_above", dict(slot=None)),  # kmc_hip_num_slots()
]


def part_call(lib, entry, file_type, part_kind, line_cap, flags, slot, prepare=True):
    """one call of `entry` on TEXT; prepare: with the signature map set and the small-k table open, so that the part's parameters alone decide"""
    L = lib.L
    if prepare:
        smap = (np.arange((1 << (2 * M)) + 1) % 3).astype(np.int32)
        assert L.kmc_hip_split_set_map(lib.h, 0, smap.ctypes.data, M) == 0 and L.kmc_hip_smallk_open(lib.h, 0, K, 1) == 0
    slot = L.kmc_hip_num_slots() if slot is None else slot
    t = np.frombuffer(TEXT, dtype=np.uint8)
    n_reads, n_kmers = C.c_uint64(0), C.c_uint64(0)
    if entry == "kmc_hip_smallk_part":
        p = capi.SplitParams(K, 0, 0, 0, 1, file_type, line_cap, part_kind, flags)
        return L.kmc_hip_smallk_part(lib.h, 0, slot, C.byref(p), t.ctypes.data, t.size, C.byref(n_reads), C.byref(n_kmers))
    n_bins = 3
    p = capi.SplitParams(K, M, n_bins, 0, 1, file_type, line_cap, part_kind, flags)
    recs = np.zeros(1 << 16, dtype=np.uint8)
    arr = [np.zeros(n_bins, dtype=np.uint64) for _ in range(5)]
    return L.kmc_hip_split_part(lib.h, 0, slot, C.byref(p), t.ctypes.data, t.size, recs.ctypes.data, recs.size, C.byref(n_kmers), *[a.ctypes.data for a in arr], C.byref(n_reads))


@pytest.mark.parametrize("entry", ("kmc_hip_split_part", "kmc_hip_smallk_part"))
def test_the_sound_part_is_taken(lib, entry):
    """the call every refused one below differs from in one thing"""
    assert part_call(lib, entry, **SOUND) == 0, lib.error()
    assert lib.L.kmc_hip_smallk_close(lib.h, 0) == 0


@pytest.mark.parametrize("entry", ("kmc_hip_split_part", "kmc_hip_smallk_part"))
@pytest.mark.parametrize("case", PART_REFUSALS, ids=[c[0] for c in PART_REFUSALS])
def test_both_part_entries_refuse_the_same_parts(lib, entry, case):
    assert part_call(lib, entry, **dict(SOUND, **case[1])) == EINVAL
    assert entry in lib.error()
    assert lib.L.kmc_hip_smallk_close(lib.h, 0) == 0


# ---- 3: the two accumulators
ACCUMULATORS = [  # (name, parameters of open, the same with one changed, entries)
    ("estimate", (27, 4, 10), (27, 4, 11), 2 << 10),
    ("estimate", (27, 4, 10), (26, 4, 10), 2 << 10),
    ("smallk", (5, 1), (5, 0), 1 << 10),
    ("smallk", (5, 1), (6, 1), 1 << 10),
]


@pytest.mark.parametrize("name,par,other,entries", ACCUMULATORS, ids=["estimate_r", "estimate_k", "smallk_strands", "smallk_k"])
def test_an_accumulator_opens_once_and_is_read_inside_its_range(lib, name, par, other, entries):
    L, h = lib.L, lib.h
    fn = {s: getattr(L, f"kmc_hip_{name}_{s}") for s in ("open", "read", "close")}
    dst = np.zeros(entries + 1, dtype=np.uint64)
    assert fn["close"](h, 0) == 0  # nothing open: closing is fine
    assert fn["read"](h, 0, 0, 1, dst.ctypes.data) == EINVAL and f"kmc_hip_{name}_read" in lib.error()  # read without open
    assert fn["open"](h, 0, *par) == 0 and fn["open"](h, 0, *par) == 0  # the same parameters again: a no-op
    assert fn["open"](h, 0, *other) == EINVAL and f"kmc_hip_{name}_open" in lib.error()
    for first, count in ((0, entries + 1), (entries, 1), (entries + 1, 0), (1, entries)):  # one past the end, from either side
        assert fn["read"](h, 0, first, count, dst.ctypes.data) == EINVAL, (first, count)
        assert f"kmc_hip_{name}_read" in lib.error()
    assert fn["read"](h, 0, 0, entries, dst.ctypes.data) == 0 and fn["read"](h, 0, entries, 0, dst.ctypes.data) == 0 and not dst.any()
    assert fn["read"](h, 0, 0, 1, None) == EINVAL
    assert fn["close"](h, 0) == 0 and fn["close"](h, 0) == 0
    assert fn["open"](h, 0, *other) == 0 and fn["close"](h, 0) == 0  # closed: other parameters open


def test_a_part_call_without_its_accumulator_is_refused(lib):
    L, h = lib.L, lib.h
    assert part_call(lib, "kmc_hip_split_part", **SOUND) == 0, lib.error()  # sets the map
    assert L.kmc_hip_estimate_close(h, 0) == 0 and L.kmc_hip_smallk_close(h, 0) == 0
    assert part_call(lib, "kmc_hip_split_part", prepare=False, **dict(SOUND, flags=capi.SPLIT_ESTIMATE)) == EINVAL and "kmc_hip_split_part" in lib.error()
    assert part_call(lib, "kmc_hip_smallk_part", prepare=False, **SOUND) == EINVAL and "kmc_hip_smallk_part" in lib.error()
    # one open with another kmer_len is no better
    assert L.kmc_hip_estimate_open(h, 0, K + 1, 4, 10) == 0 and L.kmc_hip_smallk_open(h, 0, K + 1, 1) == 0
    assert part_call(lib, "kmc_hip_split_part", prepare=False, **dict(SOUND, flags=capi.SPLIT_ESTIMATE)) == EINVAL and "kmc_hip_split_part" in lib.error()
    assert part_call(lib, "kmc_hip_smallk_part", prepare=False, **SOUND) == EINVAL and "kmc_hip_smallk_part" in lib.error()
    assert L.kmc_hip_estimate_close(h, 0) == 0 and L.kmc_hip_smallk_close(h, 0) == 0
