"""Timing of kmc_hip_smallk_part (include/kmc_hip.h: small k, k <= 13, counted on the device by k_s1_smallk_count) on one 32 MB FASTA part of 100 kbp
records at several k, next to kmc_hip_split_part of the same part at k = 27 on the same build (mode `split`: the existing chain), and the same again with
one 2 Mbp homopolymer record inside (modes `poly-*`: every window of that record is one k-mer, the same-address case). Wall-clock of the synchronous C-ABI
call (H2D of the text, the front half of kmc_amd/csrc/stage1_chain.h, the counting kernel, D2H of one word), median, best and worst of --reps calls behind
one warm-up call; one JSON line per mode and k. $KMC_HIP_S1_SMALLK_LDS_K (0 = every k adds straight into the table in HBM) and $KMC_HIP_S1_SMALLK_WGS (the
number of persistent workgroups) are the library's measurement switches; $KMC_HIP_LIB picks the build, and `--modes split` runs on a library from before
small k. For the kernels alone run it under `rocprofv3 --kernel-trace --stats -- python tools/s1_smallk_part_bench.py`. numpy + the C-ABI only."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmc_amd import capi  # noqa: E402
from s1_est_part_bench import make_part  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbytes", type=int, default=32, help="size of the part (the reference's reader cuts parts of up to 32 MB)")
    ap.add_argument("--record", type=int, default=100_000, help="symbols per record")
    ap.add_argument("--poly", default="A", help="letter (or repeat unit, e.g. AC) of the 2 Mbp low-complexity record of the `poly` modes")
    ap.add_argument("--poly-len", type=int, default=2_000_000)
    ap.add_argument("--ks", default="5,7,8,11,13", help="comma-separated k of the smallk modes")
    ap.add_argument("--poly-ks", default="5,13", help="comma-separated k of the poly-smallk mode")
    ap.add_argument("--split-k", type=int, default=27)
    ap.add_argument("--m", type=int, default=9)
    ap.add_argument("--bins", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--modes", default="split,smallk,poly-smallk", help="comma-separated: split, smallk, poly-split, poly-smallk")
    a = ap.parse_args()
    ctx = capi.Context((0,))
    L, h = ctx.L, ctx.h
    L.kmc_hip_split_set_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
    L.kmc_hip_split_part.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7
    covers = hasattr(L, "kmc_hip_split_covers") and hasattr(L, "kmc_hip_smallk_open") and L.kmc_hip_split_covers(capi.SPLIT_COVERS_SMALLK) == 1
    env = {v: os.environ.get(v) for v in ("KMC_HIP_S1_SMALLK_LDS_K", "KMC_HIP_S1_SMALLK_WGS") if os.environ.get(v)}
    texts = {}

    def report(what, mode, k, text, n_rec, reads, kmers, times, **extra):
        print(json.dumps(dict(what=what, mode=mode, k=k, text_bytes=int(text.size), records=n_rec, reads=reads, kmers=kmers, seconds=min(times),
                              seconds_median=float(np.median(times)), seconds_max=max(times), reps=a.reps, text_GBs=text.size / float(np.median(times)) / 1e9, **env, **extra)),
              flush=True)

    for mode in a.modes.split(","):
        poly = mode.startswith("poly")
        if poly not in texts:
            texts[poly] = make_part(a.mbytes, a.record, 1, a.poly_len if poly else 0, a.poly.encode())
        text, n_rec = texts[poly]
        if mode.endswith("split"):
            smap = np.random.default_rng(2).integers(0, a.bins, size=(1 << (2 * a.m)) + 1).astype(np.int32)
            ctx._chk(L.kmc_hip_split_set_map(h, 0, smap.ctypes.data, a.m))
            arr = np.zeros((5, a.bins), dtype=np.uint64)
            need, n_reads = C.c_uint64(0), C.c_uint64(0)
            recs = np.zeros(2 * text.size + 256 * (a.bins + 1), dtype=np.uint8)
            p = capi.SplitParams(a.split_k, a.m, a.bins, 3, 1, 0, 524296, 0, 0)  # line_cap: KMC's mem_part_pmm_reads
            times = []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                rc = L.kmc_hip_split_part(h, 0, 0, C.byref(p), text.ctypes.data, text.size, recs.ctypes.data, recs.size, C.byref(need), *[x.ctypes.data for x in arr],
                                          C.byref(n_reads))
                dt = time.perf_counter() - t0
                ctx._chk(rc)
                if rep:  # the first call grows the arena
                    times.append(dt)
            report("kmc_hip_split_part: one FASTA part, host text -> host records" + (", with a homopolymer record" if poly else ""), mode, a.split_k, text, n_rec,
                   int(n_reads.value), int(arr[2].sum()), times, bins=a.bins)
            continue
        if not covers:
            raise SystemExit("this library does not count small k on the device (kmc_hip_split_covers(0x103) answers 0)")
        for k in [int(x) for x in (a.poly_ks if poly else a.ks).split(",")]:
            p = capi.SplitParams(k, 0, 0, 0, 1, 0, 524296, 0, 0)
            n_reads, n_kmers = C.c_uint64(0), C.c_uint64(0)
            t0 = time.perf_counter()
            ctx._chk(L.kmc_hip_smallk_open(h, 0, k, 1))
            open_seconds = time.perf_counter() - t0
            times = []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                rc = L.kmc_hip_smallk_part(h, 0, 0, C.byref(p), text.ctypes.data, text.size, C.byref(n_reads), C.byref(n_kmers))
                dt = time.perf_counter() - t0
                ctx._chk(rc)
                if rep:
                    times.append(dt)
            chunk = np.zeros(min(1 << 22, 1 << (2 * k)), dtype=np.uint64)
            t0, total, top = time.perf_counter(), 0, 0
            for first in range(0, 1 << (2 * k), chunk.size):
                ctx._chk(L.kmc_hip_smallk_read(h, 0, first, chunk.size, chunk.ctypes.data))
                total += int(chunk.sum(dtype=np.uint64))
                top = max(top, int(chunk.max()))
            drain_seconds = time.perf_counter() - t0
            ctx._chk(L.kmc_hip_smallk_close(h, 0))
            assert total == int(n_kmers.value) * (a.reps + 1), (total, n_kmers.value)
            report("kmc_hip_smallk_part: one FASTA part, host text -> the device's table" + (", with a homopolymer record" if poly else ""), mode, k, text, n_rec,
                   int(n_reads.value), int(n_kmers.value), times, open_seconds=open_seconds, drain_seconds=drain_seconds, largest_counter_per_call=top // (a.reps + 1))
    ctx.close()


if __name__ == "__main__":
    main()
