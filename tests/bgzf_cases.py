"""BGZF cases shared by tests/test_bgzf_emulated.py (the product's host library over the CPU emulation) and tests/test_gpu_bgzf.py (the device): members of every
deflate block type, match geometry, sizes and placements, header variants for the scan, and corruptions — one damaged member among good ones.

The oracle is Python's zlib, the library the reference calls (kmc_core/fastq_reader.cpp:141-189): zlib.decompressobj(-15) over a member's deflate data and
zlib.crc32 over what it returns. A member is good when inflate ends at the end of the data with ISIZE bytes whose CRC32 is the member's; everything else is refused.
Members that zlib's own deflate never writes (a match at distance 32768: its window stops 262 bytes short of that) are assembled bit by bit here and held to the
same oracle."""
import struct
import zlib

import numpy as np

from kmc_amd import capi, synth

EOF = synth.BGZF_EOF


# ---- members
def frame(comp: bytes, crc: int, isize: int, extra_before: bytes = b"", fname: bytes = None, fhcrc: bool = False) -> bytes:
    """a BGZF member around raw deflate data; extra_before: other subfields in front of BC; fname: sets FLG.FNAME"""
    extra = extra_before + b"BC" + struct.pack("<H", 2)
    tail = (fname + b"\0" if fname is not None else b"") + (b"\x12\x34" if fhcrc else b"")
    bsize = 12 + len(extra) + 2 + len(tail) + len(comp) + 8
    assert bsize <= 0x10000, bsize
    flg = 4 | (8 if fname is not None else 0) | (2 if fhcrc else 0)
    return struct.pack("<4BI2BH", 0x1F, 0x8B, 8, flg, 0, 0, 0xFF, len(extra) + 2) + extra + struct.pack("<H", bsize - 1) + tail + comp + struct.pack("<II", crc & 0xFFFFFFFF, isize)


def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), flush_mode=zlib.Z_FULL_FLUSH) -> bytes:
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = b"", 0
    for cut in flush_at:
        out += z.compress(data[at:cut]) + z.flush(flush_mode)
        at = cut
    return out + z.compress(data[at:]) + z.flush()


def member(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **kw) -> bytes:
    fr = {k: kw.pop(k) for k in ("extra_before", "fname", "fhcrc") if k in kw}
    return frame(deflate(data, level, strategy, **kw), zlib.crc32(data), len(data), **fr)


def raw_member(comp: bytes, data: bytes) -> bytes:
    """hand-made deflate data that inflates to `data`"""
    return frame(comp, zlib.crc32(data), len(data))


# ---- deflate assembled by hand (RFC 1951): fields least significant bit first, Huffman codes most significant bit first
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        self.put(int(format(code, "0%db" % nbits)[::-1], 2), nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self) -> bytes:
        self.align()
        return bytes(self.out)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def fixed_symbol(b: Bits, s: int):
    if s < 144:
        b.code(0x30 + s, 8)
    elif s < 256:
        b.code(0x190 + s - 144, 9)
    elif s < 280:
        b.code(s - 256, 7)
    else:
        b.code(0xC0 + s - 280, 8)


def fixed_match(b: Bits, length: int, dist: int):
    ls = max(i for i in range(29) if _LEN_BASE[i] <= length) if length < 258 else 28
    fixed_symbol(b, 257 + ls)
    b.put(length - _LEN_BASE[ls], _LEN_EXTRA[ls])
    ds = max(i for i in range(30) if _DIST_BASE[i] <= dist)
    b.code(ds, 5)
    b.put(dist - _DIST_BASE[ds], _DIST_EXTRA[ds])


def stored_block(b: Bits, data: bytes, final: bool):
    b.put(1 if final else 0, 1)
    b.put(0, 2)
    b.align()
    b.put(len(data), 16)
    b.put(len(data) ^ 0xFFFF, 16)
    b.align()
    b.out += data


def fixed_block(b: Bits, ops, final: bool):
    """ops: bytes (literals) or (length, distance)"""
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    for op in ops:
        if isinstance(op, tuple):
            fixed_match(b, *op)
        else:
            for c in op:
                fixed_symbol(b, c)
    fixed_symbol(b, 256)


def replay(ops_blocks) -> bytes:
    """what the hand-made blocks inflate to: [("stored", bytes) | ("fixed", ops)]"""
    out = bytearray()
    for kind, x in ops_blocks:
        if kind == "stored":
            out += x
        else:
            for op in x:
                if isinstance(op, tuple):
                    for _ in range(op[0]):
                        out.append(out[-op[1]])
                else:
                    out += op
    return bytes(out)


def hand_member(blocks) -> bytes:
    b = Bits()
    for i, (kind, x) in enumerate(blocks):
        (stored_block if kind == "stored" else fixed_block)(b, x, i == len(blocks) - 1)
    return raw_member(b.bytes(), replay(blocks))


def dynamic_header(b: Bits, lit_lens, dist_lens):
    """a dynamic block's header whose code-length code has the two symbols 0 and 1, one bit each: every literal/length and distance length is 0 or 1"""
    assert set(lit_lens) | set(dist_lens) <= {0, 1} and len(lit_lens) >= 257 and len(dist_lens) >= 1
    b.put(1, 1)
    b.put(2, 2)
    b.put(len(lit_lens) - 257, 5)
    b.put(len(dist_lens) - 1, 5)
    b.put(18 - 4, 4)  # 18 lengths of the code-length code: up to symbol 1 in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1
    for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1):
        b.put(1 if s in (0, 1) else 0, 3)
    for v in list(lit_lens) + list(dist_lens):
        b.code(v, 1)


# ---- the oracle
def py_table(blob: bytes) -> np.ndarray:
    """the member table of a well-formed BGZF blob, by RFC 1952 and the SAM specification: what kmc_hip_bgzf_scan must return for it"""
    rows, pos, out = [], 0, 0
    while pos < len(blob):
        assert blob[pos:pos + 3] == b"\x1f\x8b\x08" and blob[pos + 3] & 4
        flg, xlen = blob[pos + 3], struct.unpack_from("<H", blob, pos + 10)[0]
        x, bsize = pos + 12, None
        while x < pos + 12 + xlen:
            slen = struct.unpack_from("<H", blob, x + 2)[0]
            if blob[x:x + 2] == b"BC" and slen == 2:
                bsize = struct.unpack_from("<H", blob, x + 4)[0] + 1
            x += 4 + slen
        hd = pos + 12 + xlen
        for bit in (8, 16):
            if flg & bit:
                hd = blob.index(b"\0", hd) + 1
        hd += 2 if flg & 2 else 0
        crc, isize = struct.unpack_from("<II", blob, pos + bsize - 8)
        rows.append((hd, out, pos + bsize - 8 - hd, isize, crc, 0))
        out += isize
        pos += bsize
    return np.array(rows, dtype=capi.BGZF_MEMBER)


def oracle(blob: bytes, members: np.ndarray):
    """per member of the table: the bytes zlib inflates, or None where zlib (or the trailer) refuses the member"""
    out = []
    for m in members:
        comp = blob[int(m["src_off"]):int(m["src_off"]) + int(m["comp_len"])]
        d = zlib.decompressobj(-15)
        try:
            data = d.decompress(comp) + d.flush()
        except zlib.error:
            out.append(None)
            continue
        good = d.eof and not d.unused_data and len(data) == int(m["isize"]) and zlib.crc32(data) == int(m["crc"])
        out.append(data if good else None)
    return out


def check(ctx, blob: bytes, members: np.ndarray = None, expect_bad=None, device=False, src_shift=0):
    """blob through the scan (unless a table is given) and the inflate entry against the oracle: zlib's bytes for every good member, KMC_HIP_ECORRUPT naming the first
    member zlib refuses, the error words set for exactly the refused ones. device: through kmc_hip_bgzf_inflate_device with d_src `src_shift` bytes into its allocation
    and every output byte outside the good members' ranges left as it was. -> (what came back, member_errors or None)"""
    if members is None:
        members, used, total = capi.bgzf_scan(blob, L=ctx.L)
        assert used == len(blob) and total == int(members["isize"].sum()) and members.tobytes() == py_table(blob).tobytes()
    want = oracle(blob, members)
    bad = [i for i, w in enumerate(want) if w is None]
    if expect_bad is not None:
        assert bad == list(expect_bad), (bad, expect_bad)
    total = int(members["dst_off"][-1] + members["isize"][-1]) if members.size else 0
    errs = None
    if device:
        src = np.frombuffer(blob, dtype=np.uint8)
        d_src, d_dst = ctx.malloc(src.size + 32), ctx.malloc(total + 64)
        try:
            ctx.h2d(d_src + src_shift, src)
            ctx.h2d(d_dst, np.full(total + 64, 0xA5, dtype=np.uint8))
            try:
                capi.bgzf_inflate_device(ctx, d_src + src_shift, src.size, members, d_dst + 16, total)
                assert not bad
            except capi.BgzfError as e:
                assert bad and e.first_bad == bad[0] and e.code == -4, (e.first_bad, bad)
                errs = e.member_errors
            got_all = np.zeros(total + 64, dtype=np.uint8)
            ctx.d2h(got_all, d_dst)
        finally:
            ctx.free(d_src)
            ctx.free(d_dst)
        assert np.all(got_all[:16] == 0xA5) and np.all(got_all[16 + total:] == 0xA5), "bytes outside the output were written"
        got = got_all[16:16 + total]
    else:
        try:
            got = capi.bgzf_inflate(ctx, blob, members)
            assert not bad
        except capi.BgzfError as e:
            assert bad and e.first_bad == bad[0] and e.code == -4, (e.first_bad, bad)
            assert f"member {bad[0]} " in str(e) and f"at byte {int(members['src_off'][bad[0]])}" in str(e), str(e)
            got, errs = e.out, e.member_errors
    for i, (m, w) in enumerate(zip(members, want)):
        lo = int(m["dst_off"])
        if w is not None:
            assert got[lo:lo + len(w)].tobytes() == w, f"member {i}: wrong bytes"
        elif device:
            assert np.all(got[lo:lo + int(m["isize"])] == 0xA5), f"member {i} was refused and wrote"
    if bad:
        assert [i for i, e in enumerate(errs) if e] == bad, (list(errs), bad)
    return got, errs


# ---- data
def text(seed: int, n: int) -> bytes:
    """FASTQ-like text: compressible, with literals and short and long matches"""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=400, dtype=np.uint8)
    out = bytearray()
    i = 0
    while len(out) < n:
        s = int(rng.integers(0, 300))
        out += b"@read%d\n" % i + bytes(b"ACGT"[c] for c in genome[s:s + 100]) + b"\n+\n" + b"I" * 100 + b"\n"
        i += 1
    return bytes(out[:n])


def noise(seed: int, n: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


HIGH = bytes(range(240, 256)) * 8 + bytes([255, 254, 255, 0, 255, 253, 128, 127, 255, 255]) * 20  # literal 255 and its neighbours


def block_type_members() -> dict:
    t = text(1, 3000)
    return {
        "stored": member(t[:700], 0),
        "fixed": member(t[:900], 6, zlib.Z_FIXED),
        "level1": member(t, 1),
        "level6": member(t, 6),
        "level9": member(t, 9),
        "huffman_only": member(t[:1500], 6, zlib.Z_HUFFMAN_ONLY),
        "rle_run": member(b"A" * 60000, 6, zlib.Z_RLE),
        "full_flush": member(t, 6, flush_at=(1000, 2000), flush_mode=zlib.Z_FULL_FLUSH),
        "sync_flush": member(t, 6, flush_at=(700, 701, 2500), flush_mode=zlib.Z_SYNC_FLUSH),
        "high_literals": member(HIGH, 6),
        "high_literals_fixed": member(HIGH, 6, zlib.Z_FIXED),
        "noise_dynamic": member(noise(2, 2000) + text(3, 500), 6),
        "long_codes": member(bytes(np.random.default_rng(4).geometric(0.08, size=6000).clip(1, 255).astype(np.uint8)), 9, zlib.Z_HUFFMAN_ONLY),  # a skewed alphabet: codes of 11 bits and more
    }


def geometry_members() -> dict:
    head = noise(5, 32768)
    lit = b"abcdefgh"
    every = [("fixed", [lit] + [op for d in range(1, 9) for op in ((258, d), (3, d), bytes([65 + d]), (d + 2, d), (100, d))])]
    return {
        "dist_32768": hand_member([("stored", head), ("fixed", [(258, 32768), (3, 32768), b"x", (40, 32768)])]),
        "dist_32767": hand_member([("stored", head), ("fixed", [(258, 32767), b"yz", (3, 32767)])]),
        "tail_repeats_head": member(noise(6, 20000) + noise(6, 20000)[:300] + noise(7, 19700) + noise(6, 20000)[100:400], 9),  # 40 KB, matches as far back as zlib writes them
        "len_3_and_258": hand_member([("fixed", [b"abc", (3, 3), (258, 6), (258, 258), (3, 1), (258, 1)])]),
        "overlap_1_to_8": hand_member(every),
    }


def size_members() -> dict:
    comp = text(8, 65536)
    out = {"isize_%d" % n: member(text(9, n), 6) for n in (1, 15, 16, 17)}
    out.update({"eof": EOF, "stored_65280": member(noise(10, 65280), 0), "level6_65536": member(comp, 6)})
    return out


def mixed_members(n: int, seed: int = 11) -> list:
    """n members of mixed kinds and odd sizes: dst_off takes every residue modulo 16"""
    rng = np.random.default_rng(seed)
    kinds = [(0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_HUFFMAN_ONLY), (6, zlib.Z_RLE)]
    out = []
    for i in range(n):
        size = int(rng.integers(1, 120)) if i % 3 else int(rng.integers(200, 900))
        if i % 17 == 5:
            out.append(EOF)  # an empty member in the middle of a file
            continue
        level, strategy = kinds[i % len(kinds)]
        data = text(100 + i, size) if i % 4 else noise(100 + i, size)
        out.append(member(data, level, strategy))
    return out


PLACEMENT_COUNTS = (1, 2, 63, 64, 65, 300)
GOOD = [member(text(20, 300), 6), member(text(21, 455), 1), member(noise(22, 77), 0)]


# ---- corruptions: name -> (blob, table or None, index of the damaged member)
def _with_good(bad: bytes):
    return GOOD[0] + GOOD[1] + bad + GOOD[2] + EOF, 2


def _patched(m: bytes, at: int, f) -> bytes:
    b = bytearray(m)
    b[at] = f(b[at])
    return bytes(b)


def corruptions() -> dict:
    t = text(30, 1200)
    good6, stored = member(t, 6), member(t[:300], 0)
    out = {}

    def file_case(name, bad):
        blob, i = _with_good(bad)
        out[name] = (blob, None, i)

    def table_case(name, base, f):
        blob, i = _with_good(base)
        members = py_table(blob)
        f(members[i:i + 1])
        members["dst_off"] = np.cumsum(members["isize"], dtype=np.uint64) - members["isize"]
        out[name] = (blob, members, i)

    file_case("crc_flipped", _patched(good6, len(good6) - 8, lambda x: x ^ 1))
    table_case("isize_one_too_small", good6, lambda m: m.__setitem__("isize", m["isize"] - 1))
    table_case("isize_one_too_large", good6, lambda m: m.__setitem__("isize", m["isize"] + 1))
    file_case("block_type_3", frame(b"\x07" + b"\0" * 10, 0, 0))
    file_case("nlen_damaged", _patched(stored, 18 + 3, lambda x: x ^ 0x10))
    b = Bits()
    dynamic_header(b, [1] * 257, [0])
    file_case("oversubscribed_lengths", frame(b.bytes() + b"\0" * 4, 0, 0))
    b = Bits()
    b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(0, 5), b.put(15, 4)
    for _ in range(19):
        b.put(1, 3)
    file_case("oversubscribed_code_length_code", frame(b.bytes() + b"\0" * 4, 0, 0))
    b = Bits()
    dynamic_header(b, [1, 1] + [0] * 255, [0])
    b.code(0, 1)
    file_case("no_end_of_block_code", frame(b.bytes() + b"\0" * 4, zlib.crc32(b"\0"), 1))
    b = Bits()
    b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(0, 5), b.put(0, 4)
    for v in (1, 0, 0, 1):  # the code-length code: symbols 16 and 0, one bit each; the first length is a repeat
        b.put(v, 3)
    b.code(1, 1), b.put(0, 2)
    file_case("repeat_with_nothing_before", frame(b.bytes() + b"\0" * 4, 0, 0))
    b = Bits()
    fixed_block(b, [(3, 1), b"abc"], True)
    file_case("match_before_the_output", frame(b.bytes(), zlib.crc32(b"abcabc"), 6))
    b = Bits()
    fixed_block(b, [b"abcdefgh", (8, 9)], True)
    file_case("distance_one_too_far", frame(b.bytes(), 0, 16))
    b = Bits()
    b.put(1, 1), b.put(1, 2), b.code(0xC0 + 6, 8)  # fixed literal/length symbol 286
    file_case("length_symbol_286", frame(b.bytes() + b"\0" * 2, 0, 0))
    b = Bits()
    b.put(1, 1), b.put(1, 2)
    fixed_symbol(b, 65), fixed_symbol(b, 257), b.code(30, 5)  # distance symbol 30
    file_case("distance_symbol_30", frame(b.bytes() + b"\0" * 2, 0, 4))
    table_case("comp_len_minus_1", good6, lambda m: m.__setitem__("comp_len", m["comp_len"] - 1))
    table_case("comp_len_minus_8", good6, lambda m: m.__setitem__("comp_len", m["comp_len"] - 8))
    table_case("comp_len_plus_1", good6, lambda m: m.__setitem__("comp_len", m["comp_len"] + 1))
    table_case("comp_len_plus_4_stored", stored, lambda m: m.__setitem__("comp_len", m["comp_len"] + 4))
    b = Bits()
    b.put(1, 1), b.put(0, 2), b.align(), b.put(100, 16), b.put(100 ^ 0xFFFF, 16)
    file_case("stored_len_past_the_member", frame(b.bytes() + b"0123456789", zlib.crc32(b"0123456789"), 100))
    b = Bits()
    fixed_block(b, [b"abc"], False)  # no final block: the data ends where inflate wants another block header
    file_case("no_final_block", frame(b.bytes(), zlib.crc32(b"abc"), 3))
    return out


# ---- scan variants
def header_variants() -> bytes:
    t = text(40, 500)
    return (member(t, 6, extra_before=b"XY" + struct.pack("<H", 3) + b"\1\2\3") + member(t[:100], 6, fname=b"reads.fq") + member(t[:50], 1, fname=b"n", fhcrc=True,
            extra_before=b"AB\0\0") + EOF)


# ---- BAM files for `count` / `count-small` with input_format="bam": tests/golden/bgzf_<name>.bam and what the reference wrote for them (tests/make_bgzf_golden.py)
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAM_BLOCK_BYTES = 3000  # records span members
BAM_TEXT = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@CO\tline %04d of a header that spans three BGZF members %s\n" % (i, b"x" * 40) for i in range(70))
BAM_REFS = tuple((b"chr%d" % i, 1000 * (i + 1)) for i in range(5))


def bam_reads(seed: int, k: int, flags: bool) -> list:
    """[(sequence as the record stores it, flag)]: 300 reads of 100 bases from a 1.5 kbp genome, among them reads with N, one shorter than k, one of exactly k; with
    `flags` every fifth record is reversed (0x10), some are secondary (0x100) or supplementary (0x800: both left out by the reference), one has no bases"""
    import count_cases as CC

    reads = [(r.decode().upper(), 0) for r in CC.golden_reads(seed, k, n_reads=300)]
    if flags:
        reads = [(s, 0x10 if i % 5 == 0 else 0x100 if i % 23 == 1 else 0x800 if i % 29 == 2 else 0x110 if i % 31 == 3 else 0) for i, (s, _) in enumerate(reads)]
        reads[50] = ("", 0)
    return reads


# name -> (flags of the `kmc` line in front of -fbam, (k, ci, cx, cs, both, hc), the reads)
BAM_CASES = {
    "k27": (["-k27"], (27, 2, 10**9, 255, True, False), bam_reads(201, 27, False)),
    "k27_b": (["-k27", "-ci1", "-b"], (27, 1, 10**9, 255, False, False), bam_reads(202, 27, True)),
    "k27_hc": (["-k27", "-hc"], (27, 2, 10**9, 255, True, True), bam_reads(203, 27, True)),
    "k9": (["-k9"], (9, 2, 10**9, 255, True, False), bam_reads(204, 9, True)),
}


def bam_path(name) -> str:
    return os.path.join(GOLDEN, "bgzf_" + name + ".bam")


def bam_out(name) -> str:
    return os.path.join(GOLDEN, "bgzf_" + name + "_out")


def write_case_bam(name, path) -> int:
    recs = [synth.bam_record(s, flag, name=b"r%d" % i) for i, (s, flag) in enumerate(BAM_CASES[name][2])]
    return synth.write_bam(path, recs, BAM_BLOCK_BYTES, BAM_TEXT, BAM_REFS)


def bam_as_fasta(name) -> bytes:
    """the case's reads as the reference's splitter sees them (synth.bam_reads_as_getseq), as 2-line FASTA"""
    seqs, _ = synth.bam_reads_as_getseq(BAM_CASES[name][2], BAM_CASES[name][1][4])
    return b"".join(b">r%d\n" % i + s + b"\n" for i, s in enumerate(seqs) if s)


def make_context(path):
    """the interface of capi.Context on a library given by path, with the entries `count`, `count-small` and `filter` go through"""
    import count_cases as CC
    import query_cases as Q
    import smallk_db_cases as K

    class BgzfContext(CC.CountContext, K.SkContext, Q.LibContext):
        pass

    return BgzfContext(path)


# ---- what both test files run (ctx: a capi.Context or make_context's)
def bgzipped(data: bytes, block_bytes: int = 700) -> bytes:
    return synth.bgzf_blocks(data, block_bytes) + EOF


def check_kernel_cases(ctx, device=False):
    for group in (block_type_members, geometry_members, size_members):
        for name, m in group().items():
            try:
                check(ctx, m + EOF, expect_bad=[], device=device)
                check(ctx, GOOD[2] + EOF + m + GOOD[0], expect_bad=[], device=device)  # an empty member in front, an odd dst_off
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}")


def check_placements(ctx, device=False):
    members = mixed_members(max(PLACEMENT_COUNTS))
    for n in PLACEMENT_COUNTS:
        blob = b"".join(members[:n])
        table = py_table(blob)
        if n == 300:
            assert set(int(x) % 16 for x in table["dst_off"]) == set(range(16))  # both copy-out edges at every residue
        check(ctx, blob, expect_bad=[], device=device)
    for shift in (1, 7):  # a d_src that begins at an odd address
        check(ctx, b"".join(members[:40]), expect_bad=[], device=True, src_shift=shift)


def check_corruptions(ctx, device=False):
    """-> {name: the damaged member's error word}"""
    words = {}
    for name, (blob, table, i) in corruptions().items():
        try:
            _, errs = check(ctx, blob, table, expect_bad=[i], device=device)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}")
        words[name] = capi.BGZF_REASONS[int(errs[i])]
    return words


# the reason the device names for each corruption (zlib's own message says the same in its words)
CORRUPTION_REASONS = {
    "crc_flipped": "crc", "isize_one_too_small": "out_long", "isize_one_too_large": "out_short", "block_type_3": "btype", "nlen_damaged": "stored",
    "oversubscribed_lengths": "codeset", "oversubscribed_code_length_code": "codeset", "no_end_of_block_code": "no_eob", "repeat_with_nothing_before": "repeat",
    "match_before_the_output": "distance", "distance_one_too_far": "distance", "length_symbol_286": "symbol", "distance_symbol_30": "symbol",
    "comp_len_minus_1": "in_short", "comp_len_minus_8": "in_short", "comp_len_plus_1": "in_left", "comp_len_plus_4_stored": "in_left",
    "stored_len_past_the_member": "stored", "no_final_block": "in_short",
}


def database_bytes(path) -> tuple:
    with open(path + ".kmc_pre", "rb") as f, open(path + ".kmc_suf", "rb") as g:
        return f.read(), g.read()
