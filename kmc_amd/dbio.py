"""KMC databases on disk <-> numpy: what `python -m kmc_amd.tools` reads and writes.

read_kff() takes a KFF file (kmc_core/kff_writer.cpp) as kmc_tools' CKFFInfoReader does; write_kff() writes one as CKFFWriter does.
read_database() takes a database as `kmc` writes it (KMC2: records ordered inside every signature bin, kmc_core/kb_completer.cpp:287-320) or as `kmc_tools`
writes it (KMC1: one ascending sequence, kmc_tools/kmc1_db_writer.h:296-372); the header is parsed as kmc_tools/kmer_file_header.cpp:63-93 does.
write_kmc1() writes the KMC1 form: markers, LUT, header, records."""
from __future__ import annotations

import mmap
import os
from dataclasses import dataclass, field

import numpy as np


class DbFormatError(ValueError):
    pass


@dataclass
class Database:
    kmer_len: int
    mode: int
    counter_size: int
    lut_prefix_len: int
    signature_len: int  # 0 for KMC1
    min_count: int
    max_count: int
    total_kmers: int
    both_strands: bool  # canonical k-mers
    kmc2: bool
    lut: np.ndarray = None   # KMC1: uint64[4^p], entry i = records with a prefix below i
    recs: np.ndarray = None  # KMC1: uint8, total_kmers records of (k - p) / 4 + counter_size bytes
    bins: list = field(default_factory=list)  # KMC2: per bin (record bytes, uint64[4^p] records per prefix)
    raw_recs: np.ndarray = None  # KMC2: the body as it lies in the file (the bins' records one after the other), uint8
    raw_lut: np.ndarray = None   # KMC2: the file's LUT, uint64[n_bins * 4^p + 1] global record offsets, the last one total_kmers (kmc2_db_reader.h:1731-1791)

    @property
    def rec_bytes(self) -> int:
        return (self.kmer_len - self.lut_prefix_len) // 4 + self.counter_size


def kff_path(path: str):
    """kmc_tools' rule (kmer_file_header.cpp:104-114): the name itself where it is a file, the name + '.kff' only where it is not; None where neither is a file"""
    if os.path.isfile(path):
        return path
    return path + ".kff" if os.path.isfile(path + ".kff") else None


def is_kff(path: str) -> bool:
    """the file kff_path() names starts with 'KFF' (kmer_file_header.cpp is_kff_file; the end marker is read_kff's to refuse)"""
    p = kff_path(path)
    if p is None:
        return False
    with open(p, "rb") as f:
        return f.read(3) == b"KFF"


KFF_ENCODING = 0b00011011  # A, C, G, T = 0, 1, 2, 3: what kmc and kmc_tools write
KFF_MAX_K = 224


@dataclass
class KffFile:
    """A KFF file as kmc_tools takes it (kmer_file_header.cpp:128-174): counter_size is the scopes' data_size, min_count / max_count come from the footer (1 and
    2^32 - 1 without one), both_strands is the `canonical` byte, and total_kmers STAYS 0 — so CKMC1DbWriter::calc_lut_prefix_len (kmc1_db_writer.h:425-456) picks the
    smallest valid prefix length for a database written from it. The fields a front end reads of a Database have the same names."""
    path: str  # the file itself (the name given, or the name + '.kff')
    kmer_len: int
    counter_size: int
    min_count: int
    max_count: int
    both_strands: bool
    sections: list  # (file offset of the first record, n_recs) of every raw section in file order, the scopes flattened
    raw: np.ndarray = None  # the file's bytes: a read-only view of the mapped file, not a copy
    mode: int = 0
    total_kmers: int = 0
    lut_prefix_len: int = 0
    signature_len: int = 0
    kmc2: bool = False
    # what `kmc_tools info` prints beyond the fields above (kmc_tools.cpp:157-216)
    scopes: list = field(default_factory=list)  # per scope with a data section, in file order: (its variables as a dict, [(file offset of the first record, n_recs)])
    encoding: int = 0b00011011  # KFF_ENCODING
    all_unique: int = 1
    footer: dict = field(default_factory=dict)  # the footer's variables by name

    @property
    def rec_bytes(self) -> int:
        return (self.kmer_len + 3) // 4 + self.counter_size

    @property
    def n_recs(self) -> int:
        return sum(n for _, n in self.sections)

    def records(self) -> np.ndarray:
        """the records of all sections back to back: what kmc_hip_kff_import_device takes. One section that is not empty: a view of the mapped file, no copy"""
        rb = self.rec_bytes
        parts = [self.raw[o:o + n * rb] for o, n in self.sections if n]
        return parts[0] if len(parts) == 1 else np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def read_kff(path: str) -> KffFile:
    """The container as CKFFInfoReader walks it (kff_info_reader.cpp:26-202): markers, header, footer, the index chain from the footer's first_index (or an index as the
    first section), then every indexed section in file order. Accepted: raw sections only, every scope ordered = 1, max = 1, one k (<= 224), one data_size in 1..4,
    all_unique = 1, the encoding kmc writes. Everything else is a DbFormatError that names the cause; no file is read in part."""
    name = kff_path(path)
    if name is None:
        raise DbFormatError(f"{path}: no such KFF file")
    size = os.path.getsize(name)
    if size < 15:
        raise DbFormatError(f"{name}: KFF file refused: truncated ({size} bytes: no room for the header and the KFF marker at the end)")
    with open(name, "rb") as f:
        raw = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)  # parsed and handed on where it lies: the file is held once
    b = np.frombuffer(raw, dtype=np.uint8)

    def bad(why):
        return DbFormatError(f"{name}: KFF file refused: {why}")

    def be(pos, width=8, what="a field"):
        if pos < 0 or pos + width > size:
            raise bad(f"truncated ({what} at byte {pos} lies behind the end of the file)")
        return int.from_bytes(raw[pos:pos + width], "big")

    def variables(pos, what):
        """a 'v' section whose type byte is at pos -> dict"""
        out = {}
        n_vars = be(pos + 1, 8, what)
        pos += 9
        if n_vars > size:
            raise bad(f"truncated ({what} announces {n_vars} variables)")
        for _ in range(n_vars):
            end = raw.find(b"\0", pos)
            if end < 0:
                raise bad(f"truncated (a variable name of {what} does not end)")
            out[raw[pos:end].decode("latin-1")] = be(end + 1, 8, what)
            pos = end + 9
        return out

    if raw[:3] != b"KFF":
        raise bad("no KFF marker at the beginning")
    if size < 15 or raw[-3:] != b"KFF":
        raise bad("no KFF marker at the end (a truncated file?)")
    encoding, all_unique, canonical = raw[5], raw[6], raw[7]
    if all_unique == 0:
        raise bad("all_unique = 0: only files of unique k-mers are read, as by kmc_tools")
    if encoding != KFF_ENCODING:
        raise bad(f"encoding {encoding:#010b}: only {KFF_ENCODING:#010b} (A, C, G, T = 0, 1, 2, 3) is read")
    footer = {}
    if size >= 26 and raw[size - 23:size - 11] == b"footer_size\0":
        start = size - 3 - be(size - 11)
        if start < 12 or raw[start:start + 1] != b"v":
            raise bad("the footer does not start as a 'v' section")
        footer = variables(start, "the footer")
    first = 12 + be(8, 4, "the free block's size")
    if first >= size:
        raise bad("truncated (the free block reaches behind the end of the file)")
    index_at = footer.get("first_index")
    if raw[first:first + 1] == b"i":
        if index_at is not None and index_at != first:
            raise bad("the footer's first_index and the index that is the first section are inconsistent")
        index_at = first
    if index_at is None:
        raise bad("no index: no first_index in the footer and the first section is not an index")
    index, seen = [], set()
    while index_at:
        if index_at in seen or index_at >= size or raw[index_at:index_at + 1] != b"i":
            raise bad(f"missing index (no 'i' section at byte {index_at})")
        seen.add(index_at)
        n_entries = be(index_at + 1, 8, "an index")
        if n_entries > size:
            raise bad(f"truncated (an index announces {n_entries} sections)")
        end = index_at + 9 + 9 * n_entries + 8
        for i in range(n_entries):
            at = index_at + 9 + 9 * i
            rel = be(at + 1, 8, "an index")
            index.append((end + (rel - (1 << 64) if rel >> 63 else rel), raw[at:at + 1]))
        index_at = be(end - 8, 8, "an index")
    index.sort()
    for pos, typ in index:
        if pos < 0 or pos >= size or raw[pos:pos + 1] != typ:
            raise bad(f"the index is inconsistent with the file (no '{typ.decode('latin-1')}' section at byte {pos})")
    scopes = []  # [variables, [(data offset, n_recs)]]
    for pos, typ in index:
        if typ == b"i":
            continue
        if typ == b"v":
            if scopes and not scopes[-1][1]:
                scopes.pop()
            scopes.append([variables(pos, "a variable section"), []])
        elif typ == b"r":
            if not scopes:
                raise bad("a raw section without a variable section in front")
            for var in ("k", "max", "data_size"):
                if var not in scopes[-1][0]:
                    raise bad(f"`{var}` is not defined for a raw section")
            scopes[-1][1].append((pos + 9, be(pos + 1, 8, "a raw section")))
        elif typ == b"m":
            raise bad("a minimizer ('m') section: only raw sections are read, as by kmc_tools")
        else:
            raise bad(f"unsupported section type {typ!r}")
    scopes = [s for s in scopes if s[1]]
    if not scopes:
        raise bad("no scope with a data section was found (is the file fully indexed?)")
    ks = sorted({s[0]["k"] for s in scopes})
    if len(ks) != 1:
        raise bad(f"several k values ({', '.join(map(str, ks))}): only files with one k are read, as by kmc_tools")
    k = ks[0]
    if not 1 <= k <= KFF_MAX_K:
        raise bad(f"k = {k}: 1..{KFF_MAX_K} is read")
    for v, _ in scopes:
        if not v.get("ordered", 0):
            raise bad("ordered = 0: all sections must be ordered, as kmc_tools requires")
        if v["max"] != 1:
            raise bad(f"max = {v['max']}: only one k-mer per block is read")
    sizes = sorted({s[0]["data_size"] for s in scopes})
    if len(sizes) != 1:
        raise bad(f"scopes with different data_size ({', '.join(map(str, sizes))})")
    if not 1 <= sizes[0] <= 4:
        raise bad(f"data_size {sizes[0]}: counters of 1..4 bytes are read (kmc_tools refuses k-mers without counters)")
    rb = (k + 3) // 4 + sizes[0]
    sections = [sec for _, secs in scopes for sec in secs]
    for off, n in sections:
        if off + n * rb > size - 3:
            raise bad(f"truncated (the raw section at byte {off - 9} announces {n} records of {rb} bytes)")
    return KffFile(name, k, sizes[0], footer.get("min_count", 1), footer.get("max_count", 0xFFFFFFFF), bool(canonical), sections, b,
                   scopes=[(dict(v), list(secs)) for v, secs in scopes], encoding=encoding, all_unique=all_unique, footer=dict(footer))


def write_kff(path: str, kmer_len: int, data_size: int, both_strands: bool, min_count: int, max_count: int, sections) -> None:
    """The file CKFFWriter writes (kmc_core/kff_writer.cpp): 'KFF' 1 0 encoding all_unique = 1 canonical, an empty free block, the 'v' section (k, max = 1, data_size,
    ordered = 1), one 'r' section per element of `sections`, the index (offsets relative to its own end; its last entry the footer, next_index 0), the footer
    (first_index, min_count, max_count, counter_size, footer_size) and 'KFF'. An element of `sections` is the section's record bytes (bytes or a uint8 array), or an
    iterable of such pieces — the parts of a large export, written as they come; the section's record count is derived from the bytes and, as by InitSection /
    FinishSection (:92-127), written into its place afterwards. An output without records is ONE section of no records: the caller passes [b""]."""
    rb = (kmer_len + 3) // 4 + data_size
    be8 = lambda v: (int(v) & ((1 << 64) - 1)).to_bytes(8, "big")  # noqa: E731

    def variables(pairs):
        return b"v" + be8(len(pairs)) + b"".join(name.encode() + b"\0" + be8(val) for name, val in pairs)

    with open(path, "wb") as f:
        f.write(b"KFF" + bytes([1, 0, KFF_ENCODING, 1, 1 if both_strands else 0]) + (0).to_bytes(4, "big"))
        index = [f.tell()]
        f.write(variables([("k", kmer_len), ("max", 1), ("data_size", data_size), ("ordered", 1)]))
        for sec in sections:
            index.append(f.tell())
            f.write(b"r" + be8(0))
            n_bytes = 0
            for piece in ([sec] if isinstance(sec, (bytes, bytearray, memoryview, np.ndarray)) else sec):
                data = piece.tobytes() if isinstance(piece, np.ndarray) else bytes(piece)
                f.write(data)
                n_bytes += len(data)
            if n_bytes % rb:
                raise ValueError(f"write_kff: a section of {n_bytes} bytes is no whole number of records of {rb} bytes")
            if n_bytes:
                f.seek(index[-1] + 1)
                f.write(be8(n_bytes // rb))
                f.seek(0, os.SEEK_END)
        index_start = f.tell()
        index_end = index_start + 1 + 8 + (len(index) + 1) * 9 + 8
        f.write(b"i" + be8(len(index) + 1))
        for i, pos in enumerate(index):
            f.write((b"v" if i == 0 else b"r") + be8(pos - index_end))
        f.write(b"v" + be8(0) + be8(0))
        footer = [("first_index", index_start), ("min_count", min_count), ("max_count", max_count), ("counter_size", data_size)]
        footer.append(("footer_size", 1 + 8 + sum(len(n) + 1 + 8 for n, _ in footer) + len("footer_size") + 1 + 8))
        f.write(variables(footer) + b"KFF")


def read_database(path: str) -> Database:
    if is_kff(path) and not os.path.exists(path + ".kmc_pre"):
        raise DbFormatError(f"{path}: a KFF file; only KMC databases (.kmc_pre / .kmc_suf) are read")
    pre = np.fromfile(path + ".kmc_pre", dtype=np.uint8)
    suf = np.fromfile(path + ".kmc_suf", dtype=np.uint8)
    if pre.size < 16 or bytes(pre[:4]) != b"KMCP" or bytes(pre[-4:]) != b"KMCP":
        raise DbFormatError(f"{path}.kmc_pre: no KMCP markers")
    if suf.size < 8 or bytes(suf[:4]) != b"KMCS" or bytes(suf[-4:]) != b"KMCS":
        raise DbFormatError(f"{path}.kmc_suf: no KMCS markers")
    header_offset = int(pre[-8:-4].view(np.uint32)[0])
    kmc2 = int(pre[-12:-8].view(np.uint32)[0]) == 0x200
    h = pre[pre.size - 8 - header_offset: pre.size - 8]
    u32 = lambda o: int(h[o:o + 4].copy().view(np.uint32)[0])  # noqa: E731
    k, mode, cs, p = u32(0), u32(4), u32(8), u32(12)
    o = 16
    sig_len = 0
    if kmc2:
        sig_len = u32(o)
        o += 4
    min_count, max_lo = u32(o), u32(o + 4)
    total = int(h[o + 8:o + 16].copy().view(np.uint64)[0])
    both = int(h[o + 16]) != 1
    max_hi = u32(o + 20)
    db = Database(k, mode, cs, p, sig_len, min_count, (max_hi << 32) + max_lo, total, both, kmc2)
    n_entries = 1 << (2 * p)
    body = suf[4:-4]
    if not kmc2:
        db.lut = pre[4: 4 + 8 * n_entries].copy().view(np.uint64)
        db.recs = body.copy()
        if db.recs.size != total * db.rec_bytes:
            raise DbFormatError(f"{path}: {db.recs.size} bytes of records, the header says {total} records of {db.rec_bytes} bytes")
        return db
    lut_area = pre[4: pre.size - 8 - header_offset - ((1 << (2 * sig_len)) + 1) * 4].copy().view(np.uint64)
    n_bins = (lut_area.size - 1) // n_entries
    offs = np.concatenate([lut_area[: n_bins * n_entries], lut_area[-1:]])
    rb = db.rec_bytes
    db.raw_recs, db.raw_lut = body[: total * rb].copy(), offs.copy()
    for b in range(n_bins):
        ob = offs[b * n_entries: (b + 1) * n_entries + 1].astype(np.int64)
        db.bins.append((body[ob[0] * rb: ob[-1] * rb].copy(), np.diff(ob).astype(np.uint64)))
    return db


def best_lut_prefix_len(kmer_len: int, total_kmers: int) -> int:
    """CKMC1DbWriter::calc_lut_prefix_len for one input (kmc1_db_writer.h:432-452): the prefix length with the smallest suffixes + LUT"""
    best, best_mem = 0, 1 << 62
    for p in range(1, 16):
        if (kmer_len - p) % 4:
            continue
        mem = total_kmers * (kmer_len - p) // 4 + (8 << (2 * p))
        if mem < best_mem:
            best, best_mem = p, mem
    return best


def byte_log(x: int) -> int:
    return 1 if x < (1 << 8) else 2 if x < (1 << 16) else 3 if x < (1 << 24) else 4


def write_kmc1(path: str, kmer_len: int, counter_size: int, lut_prefix_len: int, cutoff_min: int, cutoff_max: int, both_strands: bool, lut: np.ndarray, recs: np.ndarray,
               mode: int = 0) -> None:
    """The database CKMC1DbWriter writes (kmc1_db_writer.h:296-372): 'KMCP' LUT header(64 B) uint32(64) 'KMCP' / 'KMCS' records 'KMCS'."""
    lut = np.ascontiguousarray(lut, dtype=np.uint64)
    recs = np.ascontiguousarray(recs, dtype=np.uint8)
    rb = (kmer_len - lut_prefix_len) // 4 + counter_size
    assert lut.size == 1 << (2 * lut_prefix_len) and recs.size % rb == 0
    n = recs.size // rb
    hdr = np.zeros(64, dtype=np.uint8)
    hdr[0:24].view(np.uint32)[:] = [kmer_len, mode, counter_size, lut_prefix_len, cutoff_min, cutoff_max & 0xFFFFFFFF]
    hdr[24:32].view(np.uint64)[0] = n
    hdr[32] = 0 if both_strands else 1
    hdr[36:40].view(np.uint32)[0] = cutoff_max >> 32
    with open(path + ".kmc_pre", "wb") as f:
        f.write(b"KMCP")
        f.write(lut.tobytes())
        f.write(hdr.tobytes())
        f.write(np.uint32(64).tobytes())
        f.write(b"KMCP")
    with open(path + ".kmc_suf", "wb") as f:
        f.write(b"KMCS")
        f.write(recs.tobytes())
        f.write(b"KMCS")
