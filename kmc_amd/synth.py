"""Deterministic synthetic inputs (SURVEY.md §8d "Synthetic inputs").

FASTQ shape: genome = i.i.d. uniform ACGT of length G; reads = L-bp windows at uniform random
starts, each base substituted with probability `err` by a different base, reverse-complemented
with probability 0.5; constant quality 'I'; no N. NumPy ``default_rng(seed)``.

Used by tests (to drive the reference binaries in oracle/_ref) and by bench.py's cpu_baseline
leg. The large device-side workloads of bench.py come from kmc_amd/csrc/synth_bins.cpp instead
(same read model, generated straight into super-k-mer bin images).
"""
from __future__ import annotations

import numpy as np

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_reads(seed: int, genome_len: int, n_reads: int, read_len: int = 150, err: float = 0.01) -> np.ndarray:
    """Return reads as a (n_reads, read_len) uint8 array of 2-bit symbols (A=0 C=1 G=2 T=3)."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, size=genome_len, dtype=np.uint8)
    starts = rng.integers(0, genome_len - read_len + 1, size=n_reads)
    out = np.empty((n_reads, read_len), dtype=np.uint8)
    step = 1 << 16
    ar = np.arange(read_len)
    for lo in range(0, n_reads, step):
        hi = min(n_reads, lo + step)
        r = genome[starts[lo:hi, None] + ar[None, :]]
        mask = rng.random(r.shape) < err
        sub = rng.integers(1, 4, size=r.shape, dtype=np.uint8)
        r = np.where(mask, (r + sub) & 3, r).astype(np.uint8)
        flip = rng.random(hi - lo) < 0.5
        r[flip] = (3 - r[flip])[:, ::-1]
        out[lo:hi] = r
    return out


def write_fastq(path: str, reads: np.ndarray) -> int:
    """Write reads as 4-line FASTQ records ("@r<9 digits>", sequence, "+", quality 'I'); returns bytes written."""
    n, L = reads.shape
    rec = 12 + L + 3 + L + 1
    total = 0
    with open(path, "wb") as f:
        step = 1 << 16
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            m = hi - lo
            buf = np.empty((m, rec), dtype=np.uint8)
            buf[:, 0] = ord("@")
            buf[:, 1] = ord("r")
            ids = np.arange(lo, hi, dtype=np.int64)
            for d in range(9):
                buf[:, 10 - d] = (ids // 10**d) % 10 + ord("0")
            buf[:, 11] = ord("\n")
            buf[:, 12 : 12 + L] = _ACGT[reads[lo:hi]]
            buf[:, 12 + L] = ord("\n")
            buf[:, 13 + L] = ord("+")
            buf[:, 14 + L] = ord("\n")
            buf[:, 15 + L : 15 + 2 * L] = ord("I")
            buf[:, 15 + 2 * L] = ord("\n")
            f.write(buf.tobytes())
            total += buf.size
    return total


def make_fastq(path: str, seed: int, genome_len: int, n_reads: int, read_len: int = 150, err: float = 0.01) -> int:
    return write_fastq(path, make_reads(seed, genome_len, n_reads, read_len, err))


def make_multiline_fasta(path: str, seed: int, contig_lens, line_width: int = 60, lower_frac: float = 0.0, n_run_per_mbp: float = 0.0,
                         n_run_len: int = 200, n_empty: int = 0, eol: bytes = b"\n") -> int:
    """Write an assembly-like multi-line FASTA (the input of -fm): one record per contig length in `contig_lens`, sequence wrapped at
    `line_width` columns, every line ended by `eol` (b"\n" or b"\r\n"). Sequence = i.i.d. uniform ACGT; a share `lower_frac` of it is
    soft-masked (lowercase runs of ~500 bp); `n_run_per_mbp` runs of `n_run_len` N per Mbp; `n_empty` records with a title and no sequence
    between the others. Returns bytes written."""
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in contig_lens]
    empty_before = np.bincount(rng.integers(0, len(lens) + 1, size=n_empty), minlength=len(lens) + 1)  # empty records in front of contig i
    eol_a = np.frombuffer(eol, dtype=np.uint8)
    chunk = line_width * (1 << 18)  # whole lines per chunk
    total = 0
    with open(path, "wb") as f:
        for i in range(len(lens) + 1):
            for j in range(int(empty_before[i])):
                title = b">empty_%d_%d no sequence" % (i, j) + eol
                f.write(title)
                total += len(title)
            if i == len(lens):
                break
            title = b">contig_%d synthetic assembly len=%d" % (i, lens[i]) + eol
            f.write(title)
            total += len(title)
            for lo in range(0, lens[i], chunk):
                m = min(chunk, lens[i] - lo)
                seq = _ACGT[rng.integers(0, 4, size=m, dtype=np.uint8)]
                if lower_frac > 0:
                    n = int(rng.poisson(lower_frac * m / 500))
                    d = np.zeros(m + 1, dtype=np.int32)
                    st = rng.integers(0, m, size=n)
                    np.add.at(d, st, 1)
                    np.add.at(d, np.minimum(st + rng.integers(100, 900, size=n), m), -1)
                    seq = np.where(np.cumsum(d[:m]) > 0, seq | 0x20, seq).astype(np.uint8)
                if n_run_per_mbp > 0:
                    for s0 in rng.integers(0, m, size=int(rng.poisson(n_run_per_mbp * m / 1e6))):
                        seq[s0:s0 + n_run_len] = ord("N")
                rows = (m + line_width - 1) // line_width
                buf = np.zeros((rows, line_width + eol_a.size), dtype=np.uint8)
                flat = np.zeros(rows * line_width, dtype=np.uint8)
                flat[:m] = seq
                buf[:, :line_width] = flat.reshape(rows, line_width)
                buf[:, line_width:] = eol_a
                out = buf.reshape(-1)
                if m % line_width:  # the last line of the contig is short
                    cut = (rows - 1) * (line_width + eol_a.size) + m % line_width
                    out = np.concatenate([out[:cut], eol_a])
                f.write(out.tobytes())
                total += out.size
    return total


def homopolymer_rich_sequence(rng, n: int, mean_run: float = 2.0, lower_frac: float = 0.0, n_run_per_mbp: float = 0.0, n_run_len: int = 50) -> np.ndarray:
    """`n` ASCII symbols whose homopolymer runs have geometric lengths of mean `mean_run` (successive runs differ in their symbol), a share
    `lower_frac` of the SYMBOLS in lower case (symbol by symbol, so that a run mixes cases: "aAaA" is one homopolymer to -hc), and
    `n_run_per_mbp` runs of `n_run_len` N per Mbp."""
    if n <= 0:
        return np.zeros(0, dtype=np.uint8)
    n_runs = int(n / mean_run * 1.2) + 16
    while True:
        lens = rng.geometric(1.0 / mean_run, size=n_runs)
        if int(lens.sum()) >= n:
            break
        n_runs *= 2
    sym = np.cumsum(rng.integers(1, 4, size=n_runs)) & 3  # never the symbol of the run before
    seq = _ACGT[np.repeat(sym, lens)[:n]].copy()
    if lower_frac > 0:
        seq = np.where(rng.random(n) < lower_frac, seq | 0x20, seq).astype(np.uint8)
    if n_run_per_mbp > 0:
        for s0 in rng.integers(0, n, size=int(rng.poisson(n_run_per_mbp * n / 1e6))):
            seq[s0:s0 + n_run_len] = ord("N")
    return seq


def make_long_reads(path: str, seed: int, read_lens, fmt: str = "fq", mean_run: float = 2.0, lower_frac: float = 0.1, n_run_per_mbp: float = 20.0,
                    n_run_len: int = 50, eol: bytes = b"\n") -> int:
    """Write homopolymer-rich long reads (the input -hc is meant for: ONT / PacBio): one record per length in `read_lens`, the sequence on ONE
    line, as FASTQ (`fmt` "fq": constant quality 'I') or FASTA ("fa"). Sequences come from homopolymer_rich_sequence. Returns bytes written."""
    rng = np.random.default_rng(seed)
    total = 0
    with open(path, "wb") as f:
        for i, n in enumerate(int(x) for x in read_lens):
            seq = homopolymer_rich_sequence(rng, n, mean_run, lower_frac, n_run_per_mbp, n_run_len).tobytes()
            rec = (b"@read_%d len=%d" % (i, n) + eol + seq + eol + b"+" + eol + b"I" * n + eol) if fmt == "fq" else (b">read_%d len=%d" % (i, n) + eol + seq + eol)
            f.write(rec)
            total += len(rec)
    return total


# ---- BAM (the input of -fbam), written with struct and zlib alone
_BAM_NIBBLE_OF = np.full(256, 255, dtype=np.uint8)
_BAM_NIBBLE_OF[np.frombuffer(b"=ACMGRSVTWYHKDBN", dtype=np.uint8)] = np.arange(16, dtype=np.uint8)
_TO_ACGTN = bytes(c if c in b"ACGT" else ord("N") for c in range(256))
_TO_COMPLEMENT = bytes({65: 84, 67: 71, 71: 67, 84: 65}.get(c, ord("N")) for c in range(256))
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bam_record(seq, flag: int = 0, name: bytes = b"r", n_cigar: int = 0, qual: bool = True, tags: bytes = b"", pad_to: int = 0) -> bytes:
    """One BAM alignment record (block_size included). `seq`: a str over "=ACMGRSVTWYHKDBN" as the record STORES it (an aligner stores a reversed read
    reverse-complemented and sets flag 0x10), or a sequence of nibble values 0..15; first base in the high nibble. `name` without its NUL (l_read_name = len + 1,
    at most 254 bytes); `n_cigar` operations "1M"; qualities 0xFF * l_seq (none with qual=False: not a legal record, a block_size the device refuses); `tags`
    raw bytes behind the qualities, grown with filler to make the whole record `pad_to` bytes when that is larger."""
    import struct

    nib = _BAM_NIBBLE_OF[np.frombuffer(seq.encode(), dtype=np.uint8)] if isinstance(seq, str) else np.asarray(seq, dtype=np.uint8) & 15
    assert int(nib.max(initial=0)) < 16, "a base outside =ACMGRSVTWYHKDBN"
    l_seq = int(nib.size)
    even = np.zeros(l_seq + (l_seq & 1), dtype=np.uint8)
    even[:l_seq] = nib
    packed = ((even[0::2] << 4) | even[1::2]).tobytes()
    body = name + b"\0" + struct.pack("<I", (1 << 4) | 0) * n_cigar + packed + (b"\xff" * l_seq if qual else b"")
    fixed = 36 + len(body) + len(tags)
    tags = tags + b"\x5a" * max(0, pad_to - fixed)
    block_size = 32 + len(body) + len(tags)
    head = struct.pack("<iiiIIiiii", block_size, -1, -1, (4680 << 16) | (len(name) + 1), ((flag & 0xFFFF) << 16) | n_cigar, l_seq, -1, -1, 0)
    return head + body + tags


def bam_part(records) -> bytes:
    """A part as the reference's BAM readers hand it to the splitter: whole records, one after the other, nothing else."""
    return b"".join(records)


def bgzf_blocks(data: bytes, block_bytes: int = 0xFF00, level: int = 6) -> bytes:
    """`data` as BGZF members of `block_bytes` uncompressed bytes each (gzip with the BC extra field that holds BSIZE, raw deflate, CRC32, ISIZE), without
    the EOF block."""
    import struct
    import zlib

    out = bytearray()
    for lo in range(0, len(data), block_bytes):
        chunk = data[lo:lo + block_bytes]
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = z.compress(chunk) + z.flush()
        bsize = 12 + 6 + len(comp) + 8
        assert bsize <= 0x10000
        out += struct.pack("<4BI2BH2BHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 0x42, 0x43, 2, bsize - 1) + comp + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk))
    return bytes(out)


def write_bam(path: str, records, block_bytes: int = 3000, text: bytes = b"@HD\tVN:1.6\tSO:unsorted\n", refs=()) -> int:
    """Write an (unaligned-style) BAM file: header (magic, l_text, text, n_ref, references as (name, length)) and `records` (bam_record) as one BGZF
    stream cut every `block_bytes` uncompressed bytes WITHOUT regard to record boundaries — records span blocks, as in files samtools writes — and the
    28-byte EOF block. Returns bytes written."""
    import struct

    head = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        head += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", length)
    blob = bgzf_blocks(head + b"".join(records), block_bytes) + BGZF_EOF
    with open(path, "wb") as f:
        f.write(blob)
    return len(blob)


def bam_reads_as_getseq(reads, both_strands: bool):
    """What CSplitter::GetSeq's BAM branch (splitter.cpp:326-419) returns for records given as (seq str, flag): the included sequences, in order, as ASCII with
    N for every base that is not A C G T, reversed and complemented where flag 0x10 is set and both_strands is off; and the number of included records."""
    out, n = [], 0
    for seq, flag in reads:
        if flag & 0x900:
            continue
        n += 1
        raw = seq.encode()
        out.append(raw[::-1].translate(_TO_COMPLEMENT) if not both_strands and flag & 0x10 else raw.translate(_TO_ACGTN))
    return out, n


# Named configurations of BASELINE.json / SURVEY.md §8d
CONFIGS = {
    "C1": dict(seed=12345, genome_len=400_000, n_reads=33_000),          # 10 MB FASTQ plumbing case
    "C2": dict(seed=2026, genome_len=66_000_000, n_reads=13_300_000),    # ~2 Gbp
    "C3": dict(seed=2026, genome_len=1_000_000_000, n_reads=200_000_000),  # ~30 Gbp
}

if __name__ == "__main__":
    import sys

    name, path = sys.argv[1], sys.argv[2]
    print(make_fastq(path, **CONFIGS[name]))
