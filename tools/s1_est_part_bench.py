"""Timing of kmc_hip_split_part (include/kmc_hip.h) on one 32 MB FASTA part of 100 kbp records with KMC_HIP_SPLIT_ESTIMATE off and on (--opt-out-size:
k_s1_nthash_estimate in front of the records' copy down, counters of kmc_hip_estimate_open at the reference's s = 7, r = 27), the same text both times, and
the same again with one 2 Mbp poly-A record inside (one k-mer with 2 M copies: if the filter accepts it, every window is an atomic add on ONE address;
largest_counter_per_call says whether it was accepted, and --poly picks another letter or a repeat unit such as AC). Wall-clock of the synchronous C-ABI call (H2D of the text, the kernel chain of
kmc_amd/csrc/stage1_chain.h, D2H of the records), best of --reps and the spread over them, and the time of draining the counters in 64 MB chunks; one JSON
line per mode. The flag-off line is what to compare between two builds of the library ($KMC_HIP_LIB picks the build; a library from before the flag takes
`--modes off` only). For the kernels alone run it under `rocprofv3 --kernel-trace --stats -- python tools/s1_est_part_bench.py`. numpy + the C-ABI only."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmc_amd import capi  # noqa: E402


def make_part(mbytes, record_len, seed, poly_len, poly_letter):
    """one single-line FASTA part of about `mbytes` MB: uniform random records; poly_len > 0 puts one homopolymer record in the middle"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out, size, i = [], 0, 0
    target, poly_done = (mbytes << 20) - poly_len, not poly_len
    while size < target:
        if not poly_done and size >= target // 2:
            out.append(b">poly\n" + (poly_letter * (poly_len // len(poly_letter) + 1))[:poly_len] + b"\n")
            poly_done = True
        out.append(b">read_%d synthetic\n" % i + acgt[rng.integers(0, 4, size=record_len)].tobytes() + b"\n")
        size += len(out[-1])
        i += 1
    return np.frombuffer(b"".join(out), dtype=np.uint8), len(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbytes", type=int, default=32, help="size of the part (the reference's reader cuts parts of up to 32 MB)")
    ap.add_argument("--record", type=int, default=100_000, help="symbols per record")
    ap.add_argument("--poly", default="A", help="letter (or repeat unit, e.g. AC) of the 2 Mbp low-complexity record of the `poly` modes")
    ap.add_argument("--poly-len", type=int, default=2_000_000)
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--m", type=int, default=9)
    ap.add_argument("--bins", type=int, default=512)
    ap.add_argument("--s", type=int, default=7)
    ap.add_argument("--r", type=int, default=27)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--modes", default="off,on,poly-off,poly-on", help="comma-separated: off, on, poly-off, poly-on")
    a = ap.parse_args()
    smap = np.random.default_rng(2).integers(0, a.bins, size=(1 << (2 * a.m)) + 1).astype(np.int32)
    ctx = capi.Context((0,))
    L, h = ctx.L, ctx.h
    L.kmc_hip_split_set_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
    L.kmc_hip_split_part.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7
    ctx._chk(L.kmc_hip_split_set_map(h, 0, smap.ctypes.data, a.m))
    covers = hasattr(L, "kmc_hip_split_covers") and hasattr(L, "kmc_hip_estimate_open") and L.kmc_hip_split_covers(capi.SPLIT_COVERS_ESTIMATE) == 1
    arr = np.zeros((5, a.bins), dtype=np.uint64)
    need, n_reads = C.c_uint64(0), C.c_uint64(0)
    texts = {}
    for mode in a.modes.split(","):
        poly, on = mode.startswith("poly"), mode.endswith("on")
        if on and not covers:
            raise SystemExit("this library does not cover KMC_HIP_SPLIT_ESTIMATE (kmc_hip_split_covers answers 0): it would ignore the flag")
        if poly not in texts:
            texts[poly] = make_part(a.mbytes, a.record, 1, a.poly_len if poly else 0, a.poly.encode())
        text, n_rec = texts[poly]
        recs = np.zeros(2 * text.size + 256 * (a.bins + 1), dtype=np.uint8)
        p = capi.SplitParams(a.k, a.m, a.bins, 3, 1, 0, 524296, 0, capi.SPLIT_ESTIMATE if on else 0)  # line_cap: KMC's mem_part_pmm_reads
        extra = {}
        if on:
            t0 = time.perf_counter()
            ctx._chk(L.kmc_hip_estimate_open(h, 0, a.k, a.s, a.r))
            extra["open_seconds"] = time.perf_counter() - t0
        times = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            rc = L.kmc_hip_split_part(h, 0, 0, C.byref(p), text.ctypes.data, text.size, recs.ctypes.data, recs.size, C.byref(need), *[x.ctypes.data for x in arr],
                                      C.byref(n_reads))
            dt = time.perf_counter() - t0
            ctx._chk(rc)
            if rep:  # the first call grows the arena
                times.append(dt)
        if on:
            chunk = np.zeros(1 << 24, dtype=np.uint32)
            t0, total, top = time.perf_counter(), 0, 0
            for first in range(0, 2 << a.r, chunk.size):
                cnt = min(chunk.size, (2 << a.r) - first)
                ctx._chk(L.kmc_hip_estimate_read(h, 0, first, cnt, chunk.ctypes.data))
                total += int(chunk[:cnt].sum(dtype=np.uint64))
                top = max(top, int(chunk[:cnt].max()))
            extra.update(drain_seconds=time.perf_counter() - t0, accepted_per_call=total // (a.reps + 1), largest_counter_per_call=top // (a.reps + 1))
            ctx._chk(L.kmc_hip_estimate_close(h, 0))
        print(json.dumps(dict(what="kmc_hip_split_part: one FASTA part, host text -> host records, histogram estimate %s%s" % ("on" if on else "off", ", with a homopolymer record" if poly else ""),
                              mode=mode, text_bytes=int(text.size), records=n_rec, reads=int(n_reads.value), k=a.k, bins=a.bins, s=a.s, r=a.r, kmers=int(arr[2].sum()),
                              seconds=min(times), seconds_median=float(np.median(times)), seconds_max=max(times), reps=a.reps, text_GBs=text.size / min(times) / 1e9, **extra)),
              flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
