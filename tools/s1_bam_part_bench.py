"""Timing of kmc_hip_split_part (include/kmc_hip.h) on one 32 MB part of BAM alignment records (file_type 4: k_s1_bam_chain + k_s1_bam_decode) next to the
single-line FASTA part that holds the same sequences (file_type 0: k_s1_text_to_codes). A BAM part is what the reference's BAM readers hand the splitter:
BGZF inflated and the file header taken off on the host, whole records. Wall-clock of the synchronous C-ABI call (H2D of the part, the kernel chain of
kmc_amd/csrc/stage1_chain.h, D2H of the records): median, smallest and largest of --reps calls after one warm-up call; one JSON line per part. The two parts
hold the same bases, so the BAM part is the smaller one: compare seconds, not GB/s. --fasta-only times the FASTA part alone (for a library without file_type
4: set KMC_HIP_LIB). For the kernels alone run it under `rocprofv3 --kernel-trace --stats -- python tools/s1_bam_part_bench.py`. numpy + the C-ABI only."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmc_amd import capi  # noqa: E402


def make_parts(mbytes, read_len, seed):
    """(BAM part of about `mbytes` MB, its FASTA twin, records, included records): records of `read_len` bases, a 9-byte name, one cigar operation, qualities;
    half of them flagged reverse, 2 % secondary (not in the twin). The twin is what GetSeq returns with both_strands on (flag 0x10 is then ignored)."""
    rng = np.random.default_rng(seed)
    assert read_len % 2 == 0
    rec = 36 + 9 + 4 + read_len // 2 + read_len
    n = (mbytes << 20) // rec
    bases = rng.integers(0, 4, size=(n, read_len), dtype=np.uint8)
    flags = np.where(rng.random(n) < 0.5, 0x10, 0).astype(np.uint32) | np.where(rng.random(n) < 0.02, 0x100, 0).astype(np.uint32)
    head = np.zeros((n, 9), dtype="<u4")
    head[:, 0] = rec - 4
    head[:, 1] = head[:, 2] = head[:, 6] = head[:, 7] = 0xFFFFFFFF
    head[:, 3] = (4680 << 16) | 9
    head[:, 4] = (flags << 16) | 1
    head[:, 5] = read_len
    out = np.zeros((n, rec), dtype=np.uint8)
    out[:, :36] = head.view(np.uint8).reshape(n, 36)
    ids = np.arange(n)
    out[:, 36] = ord("r")
    for d in range(7):
        out[:, 43 - d] = (ids // 10**d) % 10 + ord("0")
    out[:, 45:49] = np.frombuffer(np.array([(read_len << 4) | 0], dtype="<u4").tobytes(), dtype=np.uint8)
    nib = np.array([1, 2, 4, 8], dtype=np.uint8)[bases]
    out[:, 49:49 + read_len // 2] = (nib[:, 0::2] << 4) | nib[:, 1::2]
    out[:, 49 + read_len // 2:] = 0xFF
    keep = (flags & 0x900) == 0
    fa = np.zeros((int(keep.sum()), read_len + 3), dtype=np.uint8)
    fa[:, 0] = ord(">")
    fa[:, 1] = fa[:, -1] = ord("\n")
    fa[:, 2:-1] = np.frombuffer(b"ACGT", dtype=np.uint8)[bases[keep]]
    return out.reshape(-1), fa.reshape(-1), n, int(keep.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbytes", type=int, default=32, help="size of the BAM part (the reference's reader cuts parts of up to 32 MB)")
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--m", type=int, default=9)
    ap.add_argument("--bins", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fasta-only", action="store_true")
    a = ap.parse_args()
    bam, fa, n_rec, n_incl = make_parts(a.mbytes, a.read_len, 1)
    smap = np.random.default_rng(2).integers(0, a.bins, size=(1 << (2 * a.m)) + 1).astype(np.int32)
    ctx = capi.Context((0,))
    L, h = ctx.L, ctx.h
    L.kmc_hip_split_set_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
    L.kmc_hip_split_part.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7
    ctx._chk(L.kmc_hip_split_set_map(h, 0, smap.ctypes.data, a.m))
    arr = np.zeros((5, a.bins), dtype=np.uint64)
    need, n_reads = C.c_uint64(0), C.c_uint64(0)
    sums = {}
    for name, text, ft in (("BAM", bam, capi.SPLIT_FILE_BAM), ("single-line FASTA", fa, 0)):
        if a.fasta_only and ft:
            continue
        p = capi.SplitParams(a.k, a.m, a.bins, 3, 1, ft, 524296, 0, 0)  # line_cap: KMC's mem_part_pmm_reads
        recs = np.zeros(2 * fa.size + 256 * (a.bins + 1), dtype=np.uint8)
        times = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            rc = L.kmc_hip_split_part(h, 0, 0, C.byref(p), text.ctypes.data, text.size, recs.ctypes.data, recs.size, C.byref(need), *[x.ctypes.data for x in arr],
                                      C.byref(n_reads))
            dt = time.perf_counter() - t0
            ctx._chk(rc)
            if rep:
                times.append(dt)
        sums[ft] = (int(n_reads.value), int(arr[2].sum()), int(arr[3].sum()), int(arr[1].sum()))
        print(json.dumps(dict(what="kmc_hip_split_part: one %s part, host bytes -> host records (%d calls)" % (name, a.reps), file_type=ft, part_bytes=int(text.size),
                              records=n_rec if ft else n_incl, reads=int(n_reads.value), k=a.k, bins=a.bins, kmers=int(arr[2].sum()), superkmers=int(arr[3].sum()),
                              median_ms=statistics.median(times) * 1e3, min_ms=min(times) * 1e3, max_ms=max(times) * 1e3)), flush=True)
    if len(sums) == 2:
        assert sums[capi.SPLIT_FILE_BAM] == sums[0], ("the two parts disagree", sums)
    ctx.close()


if __name__ == "__main__":
    main()
