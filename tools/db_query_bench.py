"""Reads against an ordered database on the device (kmc_hip_db_query_reads_device): for k = 27, 55 and 127 a synthetic database — every canonical k-mer of a random
genome — and reads of 150 symbols already in HBM, half of them cut from the genome and half random, so that about half of the lookups hit. Device time by HIP events
around the call (medians of 5) for the lookups alone, with the per-read counts (`filter`), and with the masked copy (`filter -hm`), as G lookups/s of windows without an
invalid symbol. Where oracle/_ref/kmc_tools is present, the reference's `kmc_tools -t16 filter` is timed on the same data written to a temporary directory (wall time).

    python tools/db_query_bench.py [--n 2000000] [--out profiles/r07/db_query_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kmc_amd import capi, dbio  # noqa: E402

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
READ_LEN = 150


def canonical_windows(codes, k):
    """-> uint64[n_win, words] (word 0 least significant): min(k-mer, reverse complement) of every window"""
    n_win, words = codes.size - k + 1, (k + 31) // 32
    fw, rc = np.zeros((n_win, words), dtype=np.uint64), np.zeros((n_win, words), dtype=np.uint64)
    c = codes.astype(np.uint64)
    for j in range(k):
        s = c[j:j + n_win]
        b = 2 * (k - 1 - j)
        fw[:, b // 64] |= s << np.uint64(b % 64)
        b = 2 * j
        rc[:, b // 64] |= (np.uint64(3) - s) << np.uint64(b % 64)
    less, decided = np.zeros(n_win, dtype=bool), np.zeros(n_win, dtype=bool)
    for w in reversed(range(words)):
        less |= ~decided & (fw[:, w] < rc[:, w])
        decided |= fw[:, w] != rc[:, w]
    return np.where(less[:, None], fw, rc)


def body(kmers, k, p, counts):
    """ascending distinct k-mers -> (LUT, records) of a KMC1 body with one counter byte"""
    sbits = 2 * (k - p)
    w, r = sbits // 64, sbits % 64
    pref = kmers[:, w] >> np.uint64(r)
    if r and w + 1 < kmers.shape[1]:
        pref |= kmers[:, w + 1] << np.uint64(64 - r)
    pref &= np.uint64((1 << (2 * p)) - 1)
    be = np.ascontiguousarray(kmers[:, ::-1]).astype(">u8").view(np.uint8).reshape(kmers.shape[0], -1)
    recs = np.ascontiguousarray(np.concatenate([be[:, be.shape[1] - sbits // 8:], counts.astype(np.uint8)[:, None]], axis=1).reshape(-1))
    return np.searchsorted(pref, np.arange(1 << (2 * p), dtype=np.uint64), side="left").astype(np.uint64), recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2_000_000, help="database records (window starts: four times as many)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "db_query_bench.json"))
    a = ap.parse_args()
    import torch  # before libkmc_hip.so is loaded: the library then binds the HIP runtime torch brought, and the process holds one copy of it

    capi.require_gpu_backend()
    ctx = capi.Context((0,))
    ref = os.path.join(ROOT, "oracle", "_ref", "kmc_tools")
    res = dict(n_records=a.n, read_len=READ_LEN, k={})
    for k in (27, 55, 127):
        rng = np.random.default_rng(k)
        genome = rng.integers(0, 4, size=a.n + k - 1).astype(np.uint8)
        km = canonical_windows(genome, k)
        km = km[np.lexsort([km[:, w] for w in range(km.shape[1])])]
        km = km[np.concatenate([[True], (km[1:] != km[:-1]).any(axis=1)])]
        p = dbio.best_lut_prefix_len(k, km.shape[0])
        lut, recs = body(km, k, p, rng.integers(1, 200, size=km.shape[0]))
        n_reads = 4 * a.n // (READ_LEN + 1)
        text = np.empty((n_reads, READ_LEN + 1), dtype=np.uint8)
        starts = rng.integers(0, genome.size - READ_LEN, size=n_reads // 2)
        text[:n_reads // 2, :READ_LEN] = BASES[genome[starts[:, None] + np.arange(READ_LEN)[None, :]]]
        text[n_reads // 2:, :READ_LEN] = BASES[rng.integers(0, 4, size=(n_reads - n_reads // 2, READ_LEN))]
        text[:, READ_LEN] = ord("\n")
        text = text[rng.permutation(n_reads)]
        seq = text.reshape(-1)
        off = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(READ_LEN + 1)
        d = dict(recs=ctx.malloc(recs.nbytes + 256), lut=ctx.malloc(lut.nbytes), seq=ctx.malloc(seq.size + 256), off=ctx.malloc(off.nbytes), cnt=ctx.malloc(4 * seq.size),
                 nv=ctx.malloc(4 * n_reads), mk=ctx.malloc(seq.size + 256))
        ctx.h2d(d["recs"], recs)
        ctx.h2d(d["lut"], lut)
        ctx.h2d(d["seq"], seq)
        ctx.h2d(d["off"], off)
        view = capi.DbView(d["recs"], km.shape[0], d["lut"], p, 1, 1, 255)
        row = dict(records=int(km.shape[0]), lut_prefix_len=p, positions=int(seq.size), reads=n_reads, modes={})
        for mode, kw in (("lookup", dict(n_reads=0)), ("filter", dict(n_reads=n_reads, d_n_valid=d["nv"])), ("filter_hm", dict(n_reads=n_reads, d_masked=d["mk"]))):
            ms = []
            for it in range(6):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                st = ctx.db_query_reads_device(view, k, True, d["seq"], seq.size, d["off"], kw["n_reads"], 2, d["cnt"], kw.get("d_n_valid", 0), 0, kw.get("d_masked", 0))
                e1.record()
                e1.synchronize()
                if it:
                    ms.append(e0.elapsed_time(e1))
            t = statistics.median(ms) / 1e3
            row["modes"][mode] = dict(ms_median_of_5=t * 1e3, g_lookups_per_s=st["n_valid_windows"] / t / 1e9)
        row["tallies"] = st
        row["hit_rate"] = st["n_found"] / st["n_valid_windows"]
        for x in d.values():
            ctx.free(x)
        if os.path.exists(ref):
            with tempfile.TemporaryDirectory() as td:
                dbio.write_kmc1(os.path.join(td, "db"), k, 1, p, 1, 255, True, lut, recs)
                with open(os.path.join(td, "reads.fa"), "wb") as f:
                    f.write(b"".join(b">r\n" + text[i].tobytes() for i in range(n_reads)))
                t0 = time.perf_counter()
                subprocess.run([ref, "-t16", "-hp", "filter", os.path.join(td, "db"), os.path.join(td, "reads.fa"), "-ci2", "-fa", os.path.join(td, "out.fa")], check=True, capture_output=True)
                row["reference_kmc_tools_t16_filter_wall_s"] = time.perf_counter() - t0
        res["k"][str(k)] = row
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
