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
