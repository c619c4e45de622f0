"""KFF files read as database bodies (kmc_hip_kff_import_device, kmc_amd/dbio.read_kff, the KFF inputs of `python -m kmc_amd.tools`): the container and the record
restated on Python ints and bytes — no code shared with the kernels or with dbio —, the recorded reference files and command lines under tests/golden/kff_*, the planted
sections, the corruption cases, and the helpers that run the entry. TEST INFRASTRUCTURE shared by tests/make_kff_golden.py, tests/test_kff_emulated.py and
tests/test_gpu_kff.py."""
from __future__ import annotations

import gzip
import os

import numpy as np

import setops_cases as S
import transform_cases as T

GOLDEN = S.GOLDEN
U32 = S.U32
EINVAL, ECORRUPT, ECAPACITY = -1, -4, -5
THREADS = 256  # KFF_THREADS
GUARD = 0xA7


def default_ipt(k, p, cs):
    """kff_default_ipt: records per thread of a k_kff_repack workgroup, both images of the tile in 32 KiB of LDS, at most 8"""
    return max(1, min(8, 32 * 1024 // (THREADS * ((k + 3) // 4 + cs + (k - p) // 4 + cs))))


def tile_records(k, p, cs, ipt=None):
    """what one k_kff_repack workgroup covers"""
    return THREADS * (ipt or default_ipt(k, p, cs))


def smallest_p(k):
    return k % 4 or 4


# ---- the record (kff_db_reader.h:374-401, kb_completer.h:350-356): ceil(k/4) k-mer bytes, most significant first, right-aligned; data_size counter bytes, most significant first
def encode_records(k, cs, kmers, counts) -> bytes:
    kb = (k + 3) // 4
    return b"".join(x.to_bytes(kb, "big") + (c & ((1 << (8 * cs)) - 1)).to_bytes(cs, "big") for x, c in zip(kmers, counts))


def decode_records(k, cs, data):
    kb = (k + 3) // 4
    rb = kb + cs
    assert len(data) % rb == 0
    kmers = [int.from_bytes(data[i:i + kb], "big") for i in range(0, len(data), rb)]
    counts = [int.from_bytes(data[i + kb:i + rb], "big") for i in range(0, len(data), rb)]
    return kmers, counts


# ---- the container (kmc_core/kff_writer.cpp): header, 'v', one 'r' per section, 'i', the footer 'v', "KFF"
def _var_section(pairs) -> bytes:
    return b"v" + len(pairs).to_bytes(8, "big") + b"".join(name.encode() + b"\0" + val.to_bytes(8, "big") for name, val in pairs)


def encode_container(k, cs, canonical, min_count, max_count, sections, encoding=0b00011011, ordered=1, max_in_block=1, all_unique=1) -> bytes:
    """sections: the record bytes of every raw section, in file order -> the file CKFFWriter writes"""
    rb = (k + 3) // 4 + cs
    out = bytearray(b"KFF" + bytes([1, 0, encoding, all_unique, canonical]) + (0).to_bytes(4, "big"))
    index = [len(out)]
    out += _var_section([("k", k), ("max", max_in_block), ("data_size", cs), ("ordered", ordered)])
    for data in sections:
        assert len(data) % rb == 0
        index.append(len(out))
        out += b"r" + (len(data) // rb).to_bytes(8, "big") + data
    index_start = len(out)
    index_end = index_start + 1 + 8 + (len(index) + 1) * 9 + 8
    out += b"i" + (len(index) + 1).to_bytes(8, "big")
    for i, pos in enumerate(index):
        out += (b"v" if i == 0 else b"r") + ((pos - index_end) & ((1 << 64) - 1)).to_bytes(8, "big")
    out += b"v" + (0).to_bytes(8, "big") + (0).to_bytes(8, "big")  # the footer follows the index; next_index 0: the only index
    assert len(out) == index_end
    footer = [("first_index", index_start), ("min_count", min_count), ("max_count", max_count), ("counter_size", cs)]
    footer.append(("footer_size", 1 + 8 + sum(len(n) + 1 + 8 for n, _ in footer) + len("footer_size") + 1 + 8))
    out += _var_section(footer) + b"KFF"
    return bytes(out)


def decode_container(raw: bytes) -> dict:
    """the inverse, for files of the shape encode_container writes -> dict(k, cs, canonical, min_count, max_count, encoding, sections [(offset, n_recs)])"""
    assert raw[:3] == b"KFF" and raw[-3:] == b"KFF" and raw[3:5] == b"\x01\x00"
    pos = 12 + int.from_bytes(raw[8:12], "big")

    def variables(at):
        assert raw[at:at + 1] == b"v"
        n, at, out = int.from_bytes(raw[at + 1:at + 9], "big"), at + 9, {}
        for _ in range(n):
            end = raw.index(b"\0", at)
            out[raw[at:end].decode()] = int.from_bytes(raw[end + 1:end + 9], "big")
            at = end + 9
        return out, at

    v, pos = variables(pos)
    rb = (v["k"] + 3) // 4 + v["data_size"]
    sections = []
    while raw[pos:pos + 1] == b"r":
        n = int.from_bytes(raw[pos + 1:pos + 9], "big")
        sections.append((pos + 9, n))
        pos += 9 + n * rb
    assert raw[pos:pos + 1] == b"i"
    n_idx = int.from_bytes(raw[pos + 1:pos + 9], "big")
    assert n_idx == len(sections) + 2
    footer, end = variables(pos + 9 + 9 * n_idx + 8)
    assert end == len(raw) - 3 and footer["first_index"] == pos
    return dict(k=v["k"], cs=v["data_size"], max=v["max"], ordered=v["ordered"], encoding=raw[5], all_unique=raw[6], canonical=raw[7], min_count=footer["min_count"],
                max_count=footer["max_count"], sections=sections)


def file_sections(raw: bytes):
    """-> (header dict, [(kmers, counts)] per section)"""
    h = decode_container(raw)
    rb = (h["k"] + 3) // 4 + h["cs"]
    return h, [decode_records(h["k"], h["cs"], raw[o:o + n * rb]) for o, n in h["sections"]]


# ---- the recorded reference files: name -> how make_kff_golden.py makes it
FILES = {
    "kff_k27_a": ("tools", ["transform", "{g}/setops_k27_a", "reduce", "{out}", "-okff"]),
    "kff_k33_a": ("tools", ["transform", "{g}/setops_k33_a", "reduce", "{out}", "-okff"]),
    "kff_k55_a": ("tools", ["transform", "{g}/setops_k55_a", "reduce", "{out}", "-okff"]),
    "kff_k27_a_cs2": ("tools", ["transform", "{g}/setops_k27_a", "reduce", "{out}", "-cs65535", "-okff"]),  # data_size = 2
    # the flags of count case k27_fq with -ci1, and -p5: with the default signature length these few reads fall into one bin, and `kmc` writes one section per bin pack
    "kff_k27_multi": ("kmc", ["-k27", "-ci1", "-p5", "-okff", "{g}/count_k27_fq.fq", "{out}"]),
}
# what the files hold (make_kff_golden.py asserts it, test_kff_emulated.py too): k, data_size, sections, records
FILE_SHAPES = {"kff_k27_a": (27, 1, 1, 3448), "kff_k33_a": (33, 1, 1, 8473), "kff_k55_a": (55, 1, 1, 3301), "kff_k27_a_cs2": (27, 2, 1, 3448), "kff_k27_multi": (27, 1, 58, 2140)}


def kff_file(name):
    return os.path.join(GOLDEN, name + ".kff")


# ---- the recorded command lines: (name, mode, arguments, kinds of the outputs {o0}, {o1} ...: "db" | "txt" | "fq", text of the definition file of `complex` or None)
_CX = "INPUT:\na = {g}/kff_k27_a.kff -ci2\nb = {g}/setops_k27_b\nOUTPUT:\n{o0} = a + b\nOUTPUT_PARAMS:\n-cx30\n"
LINES = [
    ("multi_sort", "transform", ["{g}/kff_k27_multi.kff", "sort", "{o0}"], ["db"], None),
    ("multi_dump", "transform", ["{g}/kff_k27_multi.kff", "dump", "{o0}"], ["txt"], None),
    ("multi_dump_s", "transform", ["{g}/kff_k27_multi.kff", "dump", "-s", "{o0}"], ["txt"], None),
    ("multi_dump_hist", "transform", ["{g}/kff_k27_multi.kff", "dump", "{o0}", "histogram", "{o1}"], ["txt", "txt"], None),  # a histogram alone: see make_kff_golden.py
    ("k27_union", "simple", ["{g}/kff_k27_a.kff", "{g}/setops_k27_b", "union", "{o0}"], ["db"], None),
    ("k33_union", "simple", ["{g}/kff_k33_a", "{g}/setops_k33_b", "union", "{o0}"], ["db"], None),  # named without the extension: kmc_tools' path rule
    ("k55_kff_kff_intersect", "simple", ["{g}/kff_k55_a.kff", "-ci2", "{g}/kff_k55_a.kff", "intersect", "{o0}", "-ocsum"], ["db"], None),
    ("k27_complex", "complex", ["{cfg}"], ["db"], _CX),
    ("k27_reduce", "transform", ["{g}/kff_k27_a.kff", "reduce", "{o0}", "-ci3", "-cx20", "-cs10"], ["db"], None),
    ("k33_reduce", "transform", ["{g}/kff_k33_a.kff", "reduce", "{o0}", "-ci2"], ["db"], None),  # total_kmers 0: lut_prefix_len 1, where the KMC twin has 5
    ("k27_cs2_reduce_hist", "transform", ["{g}/kff_k27_a_cs2.kff", "reduce", "{o0}", "histogram", "{o1}"], ["db", "txt"], None),
    ("k27_filter", "filter", ["{g}/kff_k27_a.kff", "{g}/filter_reads.fq.gz", "{o0}"], ["fq"], None),
]
LINE_IDS = [ln[0] for ln in LINES]
# the twin KMC runs already recorded: line -> the golden whose records the line's output 0 must equal (header and lut_prefix_len apart)
TWINS = {"k27_union": "setops_k27_union", "k33_union": "setops_k33_union", "k27_reduce": "transform_k27_reduce_0", "k33_reduce": "transform_k33raw_reduce_dump_0"}
LIVE_LINES = ["multi_sort", "k27_union"]  # against a live kmc_tools, where oracle/_ref is present


def golden_out(line, i):
    return os.path.join(GOLDEN, f"kffline_{line[0]}_{i}")


def command_line(line, out_dir):
    """-> (argv of kmc_tools / python -m kmc_amd.tools, output paths); writes the definition file of a `complex` line into out_dir"""
    name, mode, args, kinds, cfg = line
    outs = [os.path.join(out_dir, f"{name}_{i}") for i in range(len(kinds))]
    sub = dict(g=GOLDEN, cfg=os.path.join(out_dir, name + ".cfg"), **{f"o{i}": o for i, o in enumerate(outs)})
    if cfg is not None:
        with open(sub["cfg"], "w") as f:
            f.write(cfg.format(**sub))
    return [mode] + [a.format(**sub) for a in args], outs


def output_bytes(path, kind):
    """what a run left at an output path -> tuple of bytes"""
    if kind == "db":
        return tuple(open(path + e, "rb").read() for e in (".kmc_pre", ".kmc_suf"))
    return (open(path, "rb").read(),)


def write_golden(line, i, kind, data):
    if kind == "db":
        for e, d in zip((".kmc_pre", ".kmc_suf"), data):
            with open(golden_out(line, i) + e, "wb") as f:
                f.write(d)
    else:
        with open(golden_out(line, i) + ".gz", "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
            f.write(data[0])


def read_golden(line, i, kind):
    if kind == "db":
        return tuple(open(golden_out(line, i) + e, "rb").read() for e in (".kmc_pre", ".kmc_suf"))
    with gzip.open(golden_out(line, i) + ".gz", "rb") as f:
        return (f.read(),)


# ---- the import restated
def restate_import(k, cs, p, sections, ordered):
    """sections: [(kmers ascending, counts)] -> (lut, recs) the entry must leave: ordered, the KMC1 body of all records; otherwise the file's order under the segmented LUT"""
    if ordered:
        pairs = sorted((x, c) for ks, cs_ in sections for x, c in zip(ks, cs_))
        return S.encode_body(k, p, cs, [x for x, _ in pairs], [c for _, c in pairs])
    return T.encode_segmented(k, p, cs, sections)


class Imported:
    """what one kmc_hip_kff_import_device call left on the device, and the body interface T.run_dump / T.run_histogram take"""

    def __init__(self, ctx, k, cs, p, n_seg, n, d_out, d_lut, allocs):
        self.ctx, self.k, self.cb, self.p, self.n_seg, self.n, self.d_recs, self.d_lut, self.allocs = ctx, k, cs, p, n_seg, n, d_out, d_lut, allocs

    def view(self, in_cut=(1, U32)):
        from kmc_amd import capi

        return capi.DbView(self.d_recs, self.n, self.d_lut, self.p, self.cb, in_cut[0], in_cut[1])

    def free(self):
        for d in self.allocs:
            self.ctx.free(d)
        self.allocs = []


def run_import(ctx, k, cs, p, data: bytes, sec_n, ordered, in_off=0, out_off=0, capacity=None, keep=False):
    """data: the records of all sections back to back; sec_n: records per section. d_kff starts in_off bytes and d_out out_off bytes behind an aligned address; d_out and
    d_lut_out lie between guard bytes that must come back intact. -> (lut, recs) or, with keep, (lut, recs, Imported)"""
    rb_out = (k - p) // 4 + cs
    n = sum(sec_n)
    cap = n * rb_out if capacity is None else capacity
    lut_n = (1 << (2 * p)) if ordered else (len(sec_n) << (2 * p)) + 1
    src = np.frombuffer(data, dtype=np.uint8)
    obuf = np.full(64 + out_off + cap + 64, GUARD, dtype=np.uint8)
    lbuf = np.full(8 + lut_n + 8, 0xA7A7A7A7A7A7A7A7, dtype=np.uint64)
    allocs = [ctx.malloc(in_off + src.size + 256), ctx.malloc(obuf.size + 256), ctx.malloc(lbuf.nbytes + 256)]
    try:
        if src.size:
            ctx.h2d(allocs[0] + in_off, src)
        ctx.h2d(allocs[1], obuf)
        ctx.h2d(allocs[2], lbuf)
        d_out, d_lut = allocs[1] + 64 + out_off, allocs[2] + 64
        got_n = ctx.kff_import_device(k, cs, allocs[0] + in_off, sec_n, ordered, p, d_out, cap, d_lut)
        assert got_n == n
        ctx.d2h(obuf, allocs[1])
        ctx.d2h(lbuf, allocs[2])
        assert np.all(obuf[:64 + out_off] == GUARD) and np.all(obuf[64 + out_off + n * rb_out:] == GUARD), "bytes outside the records were written"
        assert np.all(lbuf[:8] == lbuf[0]) and np.all(lbuf[8 + lut_n:] == lbuf[0]) and lbuf[0] == 0xA7A7A7A7A7A7A7A7, "words outside the LUT were written"
        lut, recs = lbuf[8:8 + lut_n].copy(), obuf[64 + out_off:64 + out_off + n * rb_out].copy()
        if keep:
            body = Imported(ctx, k, cs, p, 1 if ordered else len(sec_n), n, d_out, d_lut, allocs)
            allocs = []
            return lut, recs, body
        return lut, recs
    finally:
        for d in allocs:
            ctx.free(d)


def check_import(ctx, k, cs, p, sections, ordered, **kw):
    data = b"".join(encode_records(k, cs, ks, cc) for ks, cc in sections)
    want_lut, want_recs = restate_import(k, cs, p, [(ks, [c & ((1 << (8 * cs)) - 1) for c in cc]) for ks, cc in sections], ordered)
    lut, recs = run_import(ctx, k, cs, p, data, [len(ks) for ks, _ in sections], ordered, **kw)
    assert np.array_equal(recs, want_recs), "records differ"
    assert np.array_equal(lut, want_lut), "LUT differs"


# ---- planted sections
WIDTHS = [(27, 3), (28, 4), (32, 4), (33, 5), (33, 9), (64, 4), (65, 5), (127, 3), (129, 5), (224, 4)]  # every k % 4, 1 to 3 prefix bytes, a prefix across a 64-bit word (33, 5) and inside one, SIZE 1 2 3 4 5 7
WIDTH_IDS = [f"{k}-p{p}" for k, p in WIDTHS]
COUNTER_EDGES = [1, 255, 256, 65535, 65536, 1 << 24, U32]


def edge_counts(cs, n, at=0):
    edges = [e for e in COUNTER_EDGES if e < (1 << (8 * cs))]
    return [edges[(at + i) % len(edges)] for i in range(n)]


def split(kmers, counts, cuts):
    """one ascending sequence cut into consecutive sections at the given positions"""
    b = [0] + sorted(cuts) + [len(kmers)]
    return [(kmers[a:z], counts[a:z]) for a, z in zip(b, b[1:])]


def deal(rng, kmers, counts, sizes):
    """sections whose key ranges interleave completely: the k-mers dealt at random into sections of the given sizes, each then ascending"""
    order = rng.permutation(len(kmers))
    out, at = [], 0
    for sz in sizes:
        idx = sorted(int(i) for i in order[at:at + sz])
        out.append(([kmers[i] for i in idx], [counts[i] for i in idx]))
        at += sz
    assert at == len(kmers)
    return out


def planted_cases(k, p, tile, seed=11):
    """-> [(name, data_size, sections)]; `tile`: records of a k_kff_repack workgroup in the build under test. Every case is run with ordered = 0 and ordered = 1."""
    rng = np.random.default_rng(seed + 7 * k + p)
    n = 3 * tile + tile // 3 + 5
    n_pref = 1 << (2 * p)
    kmers = S.random_kmers(rng, k, n)
    cases = []
    for cs in (1, 2, 3, 4):  # 3 1/3 tiles in one section, every counter width, counters at the byte edges
        cases.append((f"one_section_cs{cs}", cs, [(kmers, edge_counts(cs, n))]))
    c2 = edge_counts(2, n, 1)
    cases.append(("one_tile", 1, [(kmers[:tile], edge_counts(1, tile))]))
    cases.append(("one_record", 2, [(kmers[7:8], [65535])]))
    cases.append(("no_section", 1, []))
    cases.append(("empty_sections_only", 1, [([], []), ([], []), ([], [])]))
    for name, pref in (("first_prefix", 0), ("last_prefix", n_pref - 1), ("one_prefix", n_pref // 3)):
        ks = S.random_kmers(rng, k, tile + 9, lo_prefix=pref, p=p)
        cases.append((name, 1, split(ks, edge_counts(1, len(ks)), [tile // 2])))
    few = S.random_kmers(rng, k, 5)  # long runs of empty LUT entries
    cases.append(("five_records", 3, [(few[:2], [1, 1 << 16]), ([], []), (few[2:], [65535, 65536, (1 << 24) - 1])]))
    cases.append(("two_sections", 2, split(kmers, c2, [n // 2])))
    cases.append(("seven_sections", 2, split(kmers, c2, [1, 2, tile, tile + 1, 2 * tile - 1, n - 1])))
    cases.append(("empties_front_middle_end", 2, [([], []), ([], [])] + split(kmers, c2, [tile - 1, tile - 1, tile - 1, 2 * tile + 3]) + [([], []), ([], [])]))
    for d in (-1, 0, 1):  # a section seam at the tile seam and next to it, on both tile seams
        cases.append((f"seam_{d}", 1, split(kmers, edge_counts(1, n), [tile + d, 2 * tile + d])))
    n_many = 300 if n_pref <= 1024 else 24  # a wide LUT: fewer sections, the restatement's LUT of sections x 4^p Python ints stays small
    sizes = [int(x) for x in rng.integers(0, 41, size=n_many)]
    sizes[0] = sizes[n_many // 2] = sizes[n_many // 2 + 1] = sizes[-1] = 0
    many = S.random_kmers(rng, k, sum(sizes))
    cases.append((f"{n_many}_sections_interleaved", 2, deal(rng, many, edge_counts(2, len(many)), sizes)))
    cases.append(("7_sections_interleaved", 4, deal(rng, kmers, edge_counts(4, n), [0, n // 3, 1, n // 5, 0, n - n // 3 - 1 - n // 5 - 2, 2])))
    return cases


def corruption_cases(k, p, tile, seed=5):
    """-> [(name, sections as record bytes, corrupt with ordered = 0, corrupt with ordered = 1, the record number named (of the file) or None)]. data_size 1.
    Two sections of 2 tiles + 70 and 1 tile + 9 records with disjoint, ascending ranges; the planted faults sit at record 0 of a tile, on a wave seam and at the file's last record."""
    rng = np.random.default_rng(seed + k)
    n_a, n_b = 2 * tile + 70, tile + 9
    kmers = S.random_kmers(rng, k, n_a + n_b)
    # room below every k-mer for an equal / smaller neighbour: nothing to do, the faults copy neighbours
    a, b = kmers[:n_a], kmers[n_a:]
    kb = (k + 3) // 4

    def build(a_, b_):
        return [encode_records(k, 1, a_, [7] * len(a_)), encode_records(k, 1, b_, [9] * len(b_))]

    def swap(seq, i):  # seq[i] <-> seq[i - 1]: record i is the first that is not greater than its predecessor
        s = list(seq)
        s[i], s[i - 1] = s[i - 1], s[i]
        return s

    def same(seq, i):
        s = list(seq)
        s[i] = s[i - 1]
        return s

    cases = [("clean", build(a, b), False, False, None)]
    last = n_a + n_b - 1
    for where, i in (("tile_record_0", tile), ("second_tile_record_0", 2 * tile), ("wave_seam", tile + 64), ("inside", 5)):
        cases.append((f"descending_{where}", build(swap(a, i), b), True, True, i))
        cases.append((f"equal_{where}", build(same(a, i), b), True, True, i))
    cases.append(("descending_last_record", build(a, swap(b, n_b - 1)), True, True, last))
    cases.append(("equal_last_record", build(a, same(b, n_b - 1)), True, True, last))
    if k % 4:  # a padding bit: the top bit of the first byte
        for where, i in (("tile_record_0", tile), ("last_record", last), ("record_0", 0)):
            secs = build(a, b)
            which, j = (0, i) if i < n_a else (1, i - n_a)
            raw = bytearray(secs[which])
            raw[j * (kb + 1)] |= 0x80
            secs[which] = bytes(raw)
            cases.append((f"padding_bit_{where}", secs, True, True, i))
    # descending across the SECTION seam is legal: the second section's range lies below the first's
    cases.append(("descending_across_section_seam", build(b, a), False, False, None))
    cases.append(("section_seam_on_tile_seam_descending", [encode_records(k, 1, kmers[tile:2 * tile], [3] * tile), encode_records(k, 1, kmers[:tile], [4] * tile)], False, False, None))
    # a k-mer in two sections: corrupt only for one ascending body
    dup = sorted(b + [a[3]])
    cases.append(("duplicate_across_sections", build(a, dup), False, True, None))
    return cases


class KffContext(T.TransformContext):
    """T.TransformContext with kmc_hip_kff_import_device: the interface of capi.Context on a library given by path"""

    def __init__(self, path):
        super().__init__(path)
        C = self.C
        vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
        self.L.kmc_hip_kff_import_device.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, u64p]


def _bind():
    from kmc_amd import capi

    KffContext.kff_import_device = capi.Context.kff_import_device  # the binding under test is the one the product ships


_bind()
