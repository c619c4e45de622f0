"""KMC databases on disk <-> numpy: what `python -m kmc_amd.tools` reads and writes.

read_database() takes a database as `kmc` writes it (KMC2: records ordered inside every signature bin, kmc_core/kb_completer.cpp:287-320) or as `kmc_tools`
writes it (KMC1: one ascending sequence, kmc_tools/kmc1_db_writer.h:296-372); the header is parsed as kmc_tools/kmer_file_header.cpp:63-93 does.
write_kmc1() writes the KMC1 form: markers, LUT, header, records."""
from __future__ import annotations

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


def is_kff(path: str) -> bool:
    """kmc_tools' rule (kmer_file_header.cpp is_kff_file): the name itself, or name + '.kff', is a file that starts with 'KFF'"""
    for p in (path, path + ".kff"):
        if os.path.isfile(p):
            with open(p, "rb") as f:
                if f.read(3) == b"KFF":
                    return True
    return False


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
