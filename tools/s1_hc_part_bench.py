"""Timing of kmc_hip_split_part (include/kmc_hip.h) on one 32 MB FASTA part of homopolymer-rich long reads with KMC_HIP_SPLIT_HOMOPOLYMER off and on
(-hc: k_s1_hc_compact between text -> codes and the cut), the same text both times. Wall-clock of the synchronous C-ABI call (H2D of the text, the kernel
chain of kmc_amd/csrc/stage1_chain.h, D2H of the records), best of --reps and the spread over them; one JSON line per mode. The flag-off line is what
to compare between two builds of the library ($KMC_HIP_LIB picks the build). For the kernels alone run it under
`rocprofv3 --kernel-trace --stats -- python tools/s1_hc_part_bench.py`. numpy + the C-ABI only."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmc_amd import capi, synth  # noqa: E402


def make_part(mbytes, record_len, seed, mean_run):
    """one single-line FASTA part of about `mbytes` MB: homopolymer-rich records (geometric run lengths, mixed case, N runs)"""
    rng = np.random.default_rng(seed)
    out, size, i = [], 0, 0
    while size < (mbytes << 20):
        out.append(b">read_%d synthetic\n" % i + synth.homopolymer_rich_sequence(rng, record_len, mean_run, 0.1, 20, 50).tobytes() + b"\n")
        size += len(out[-1])
        i += 1
    return np.frombuffer(b"".join(out), dtype=np.uint8), i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbytes", type=int, default=32, help="size of the part (the reference's reader cuts parts of up to 32 MB)")
    ap.add_argument("--record", type=int, default=100_000, help="symbols per record")
    ap.add_argument("--mean-run", type=float, default=2.0, help="mean homopolymer run length of the text")
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--m", type=int, default=9)
    ap.add_argument("--bins", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--modes", default="off,on", help="comma-separated: off, on (a library from before the flag takes `off` only)")
    a = ap.parse_args()
    text, n_rec = make_part(a.mbytes, a.record, 1, a.mean_run)
    smap = np.random.default_rng(2).integers(0, a.bins, size=(1 << (2 * a.m)) + 1).astype(np.int32)
    ctx = capi.Context((0,))
    L, h = ctx.L, ctx.h
    L.kmc_hip_split_set_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
    L.kmc_hip_split_part.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7
    ctx._chk(L.kmc_hip_split_set_map(h, 0, smap.ctypes.data, a.m))
    covers = hasattr(L, "kmc_hip_split_covers") and L.kmc_hip_split_covers(capi.SPLIT_COVERS_HOMOPOLYMER) == 1
    arr = np.zeros((5, a.bins), dtype=np.uint64)
    need, n_reads = C.c_uint64(0), C.c_uint64(0)
    recs = np.zeros(2 * text.size + 256 * (a.bins + 1), dtype=np.uint8)
    for mode in a.modes.split(","):
        if mode == "on" and not covers:
            raise SystemExit("this library does not cover KMC_HIP_SPLIT_HOMOPOLYMER (kmc_hip_split_covers answers 0): it would ignore the flag")
        p = capi.SplitParams(a.k, a.m, a.bins, 3, 1, 0, 524296, 0, capi.SPLIT_HOMOPOLYMER if mode == "on" else 0)  # line_cap: KMC's mem_part_pmm_reads
        times = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            rc = L.kmc_hip_split_part(h, 0, 0, C.byref(p), text.ctypes.data, text.size, recs.ctypes.data, recs.size, C.byref(need), *[x.ctypes.data for x in arr],
                                      C.byref(n_reads))
            dt = time.perf_counter() - t0
            ctx._chk(rc)
            if rep:  # the first call grows the arena
                times.append(dt)
        print(json.dumps(dict(what="kmc_hip_split_part: one FASTA part, host text -> host records, homopolymer compression %s" % mode, hc=mode, text_bytes=int(text.size),
                              records=n_rec, reads=int(n_reads.value), k=a.k, bins=a.bins, kmers=int(arr[2].sum()), superkmers=int(arr[3].sum()),
                              seconds=min(times), seconds_median=float(np.median(times)), seconds_max=max(times), reps=a.reps, text_GBs=text.size / min(times) / 1e9)),
              flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
