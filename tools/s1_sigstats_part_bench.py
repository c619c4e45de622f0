"""Timing of kmc_hip_sigstats_part (include/kmc_hip.h: stage 0, the signature statistics, k_s1_sig_stats) on one 32 MB FASTA part of 100 kbp records at
k = 27, m = 9, next to kmc_hip_split_part of the same part on the same build (mode `pair`: --rounds alternating runs, each the median of --reps calls), and
the same part with one 2 Mbp record of A inside (mode `poly`: every window of that record adds to the special entry) and with a satellite record whose windows
fall on two signatures (mode `sat`: a seeded random repeat unit, searched with the library itself). Mode `split` times kmc_hip_split_part alone and runs on a library
from before stage 0: that line, from this build and from the parent's ($KMC_HIP_LIB picks the build), shows that nothing new is launched on that road.
Wall-clock of the synchronous C-ABI call (H2D of the text, the front half of kmc_amd/csrc/stage1_chain.h, the kernel, D2H of one word); one JSON line per
mode and round. $KMC_HIP_S1_SIGSTATS_LDS_M (the largest m whose table is kept in LDS; 0 = adds straight into HBM) and $KMC_HIP_S1_SIGSTATS_WGS (persistent
workgroups) are the library's measurement switches. For the kernels alone run it under `rocprofv3 --kernel-trace --stats -- python
tools/s1_sigstats_part_bench.py`, as a run of its own. numpy + the C-ABI only."""
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

LINE_CAP = 524296  # KMC's mem_part_pmm_reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbytes", type=int, default=32, help="size of the part (the reference's reader cuts parts of up to 32 MB)")
    ap.add_argument("--record", type=int, default=100_000, help="symbols per record")
    ap.add_argument("--poly-len", type=int, default=2_000_000)
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--m", type=int, default=9)
    ap.add_argument("--bins", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--modes", default="pair,poly,sat", help="comma-separated: pair, poly, sat, split")
    a = ap.parse_args()
    ctx = capi.Context((0,))
    L, h = ctx.L, ctx.h
    L.kmc_hip_split_set_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
    L.kmc_hip_split_part.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7
    covers = hasattr(L, "kmc_hip_split_covers") and hasattr(L, "kmc_hip_sigstats_open") and L.kmc_hip_split_covers(capi.SPLIT_COVERS_SIGSTATS) == 1
    env = {v: os.environ.get(v) for v in ("KMC_HIP_S1_SIGSTATS_LDS_M", "KMC_HIP_S1_SIGSTATS_WGS", "KMC_HIP_LIB") if os.environ.get(v)}
    entries = (1 << (2 * a.m)) + 1
    smap = np.random.default_rng(2).integers(0, a.bins, size=entries).astype(np.int32)

    def report(what, mode, rnd, text, n_rec, reads, kmers, times, **extra):
        print(json.dumps(dict(what=what, mode=mode, round=rnd, k=a.k, m=a.m, text_bytes=int(text.size), records=n_rec, reads=reads, kmers=kmers, seconds=min(times),
                              seconds_median=float(np.median(times)), seconds_max=max(times), reps=a.reps, text_GBs=text.size / float(np.median(times)) / 1e9, **env, **extra)),
              flush=True)

    def time_split(text):
        ctx._chk(L.kmc_hip_split_set_map(h, 0, smap.ctypes.data, a.m))
        arr = np.zeros((5, a.bins), dtype=np.uint64)
        need, n_reads = C.c_uint64(0), C.c_uint64(0)
        recs = np.zeros(2 * text.size + 256 * (a.bins + 1), dtype=np.uint8)
        p = capi.SplitParams(a.k, a.m, a.bins, 3, 1, 0, LINE_CAP, 0, 0)
        times = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            rc = L.kmc_hip_split_part(h, 0, 0, C.byref(p), text.ctypes.data, text.size, recs.ctypes.data, recs.size, C.byref(need), *[x.ctypes.data for x in arr], C.byref(n_reads))
            dt = time.perf_counter() - t0
            ctx._chk(rc)
            if rep:  # the first call grows the arena
                times.append(dt)
        return times, int(n_reads.value), int(arr[2].sum())

    def time_stats(text):
        """-> (times, reads, k-mers, the statistics of ONE call)"""
        p = capi.SplitParams(a.k, a.m, 0, 0, 1, 0, LINE_CAP, 0, 0)
        n_reads, n_kmers = C.c_uint64(0), C.c_uint64(0)
        ctx._chk(L.kmc_hip_sigstats_open(h, 0, a.k, a.m))
        times = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            rc = L.kmc_hip_sigstats_part(h, 0, 0, C.byref(p), text.ctypes.data, text.size, C.byref(n_reads), C.byref(n_kmers))
            dt = time.perf_counter() - t0
            ctx._chk(rc)
            if rep:
                times.append(dt)
        stats = np.zeros(entries, dtype=np.uint32)
        ctx._chk(L.kmc_hip_sigstats_read(h, 0, 0, entries, stats.ctypes.data))
        ctx._chk(L.kmc_hip_sigstats_close(h, 0))
        assert int(stats.sum(dtype=np.uint64)) == int(n_kmers.value) * (a.reps + 1), (int(stats.sum(dtype=np.uint64)), n_kmers.value)
        return times, int(n_reads.value), int(n_kmers.value), stats // np.uint32(a.reps + 1)

    def satellite_unit():
        """a repeat unit whose 10 kbp repeat puts its windows on exactly two signatures, found with the library. A unit no longer than a window's k - m + 1 m-mers
        gives every window the same m-mers, so one signature: seeded random units of k - m + 2 .. 3k symbols are tried"""
        p = capi.SplitParams(a.k, a.m, 0, 0, 1, 0, LINE_CAP, 0, 0)
        rng = np.random.default_rng(3)
        for _ in range(400):
            unit = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=int(rng.integers(a.k - a.m + 2, 3 * a.k))))
            text = np.frombuffer(b">s\n" + (unit.encode() * 10_000)[:10_000] + b"\n", dtype=np.uint8)
            n_reads, n_kmers = C.c_uint64(0), C.c_uint64(0)
            ctx._chk(L.kmc_hip_sigstats_open(h, 0, a.k, a.m))
            ctx._chk(L.kmc_hip_sigstats_part(h, 0, 0, C.byref(p), text.ctypes.data, text.size, C.byref(n_reads), C.byref(n_kmers)))
            stats = np.zeros(entries, dtype=np.uint32)
            ctx._chk(L.kmc_hip_sigstats_read(h, 0, 0, entries, stats.ctypes.data))
            ctx._chk(L.kmc_hip_sigstats_close(h, 0))
            if np.count_nonzero(stats) == 2:
                return unit
        raise SystemExit("no repeat unit tried falls on exactly two signatures at this k and m")

    plain = None
    for mode in a.modes.split(","):
        if mode != "split" and not covers:
            raise SystemExit("this library does not compute the signature statistics on the device (kmc_hip_split_covers(0x107) answers 0)")
        if mode in ("pair", "split"):
            if plain is None:
                plain = make_part(a.mbytes, a.record, 1, 0, b"A")
            text, n_rec = plain
            for rnd in range(a.rounds):
                if mode == "pair":
                    times, reads, kmers, stats = time_stats(text)
                    report("kmc_hip_sigstats_part: one FASTA part, host text -> the device's statistics", "pair-sigstats", rnd, text, n_rec, reads, kmers, times,
                           signatures_hit=int(np.count_nonzero(stats)), largest_entry=int(stats.max()))
                times, reads, kmers = time_split(text)
                report("kmc_hip_split_part: one FASTA part, host text -> host records", "pair-split" if mode == "pair" else "split", rnd, text, n_rec, reads, kmers, times, bins=a.bins)
            continue
        unit = "A" if mode == "poly" else satellite_unit()
        text, n_rec = make_part(a.mbytes, a.record, 1, a.poly_len, unit.encode())
        for rnd in range(a.rounds):
            times, reads, kmers, stats = time_stats(text)
            report("kmc_hip_sigstats_part: the part with a %d bp record of (%s)n" % (a.poly_len, unit), mode, rnd, text, n_rec, reads, kmers, times, unit=unit,
                   signatures_hit=int(np.count_nonzero(stats)), largest_entry=int(stats.max()), special_entry=int(stats[entries - 1]))
    ctx.close()


if __name__ == "__main__":
    main()
