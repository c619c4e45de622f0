"""One database transformed on the device (kmc_hip_db_dump_device, kmc_hip_db_reduce_device, kmc_hip_db_histogram_device): for k = 27, 55 and 127 a synthetic ordered
database of 8 M random k-mers already in HBM, two counter bytes. Device time by HIP events around each call (medians of 5):
  dump       the whole database as text: G records/s and GB/s of text written
  reduce     -ci2 -cx200 -cs255: G records/s of input
  histogram  counters 1..255 (the bins in LDS): G records/s, once with counters drawn uniformly from 1..255 and once with a k-mer-spectrum-like draw (about 70 % ones
             and a geometric tail) — the skewed draw is what the combining of equal counters inside a wave is for
Where oracle/_ref/kmc_tools is present, the whole process `kmc_tools -t16 transform <db> dump|reduce|histogram` is timed on the same database from disk (wall time,
spectrum-like counters).

    python tools/db_transform_bench.py [--n 8000000] [--out profiles/r07/db_transform_bench.json]
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


def random_body(rng, k, p, n, counts):
    """n ascending distinct random k-mers -> (LUT, records with two counter bytes, n)"""
    words = (k + 31) // 32
    km = rng.integers(0, 1 << 63, size=(n, words), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, words), dtype=np.uint64)
    top = 2 * k - 64 * (words - 1)
    if top < 64:
        km[:, words - 1] &= np.uint64((1 << top) - 1)
    km = km[np.lexsort([km[:, w] for w in range(words)])]
    km = km[np.concatenate([[True], (km[1:] != km[:-1]).any(axis=1)])]
    n = km.shape[0]
    sbits = 2 * (k - p)
    w, r = sbits // 64, sbits % 64
    pref = km[:, w] >> np.uint64(r)
    if r and w + 1 < words:
        pref |= km[:, w + 1] << np.uint64(64 - r)
    pref &= np.uint64((1 << (2 * p)) - 1)
    be = np.ascontiguousarray(km[:, ::-1]).astype(">u8").view(np.uint8).reshape(n, -1)
    recs = np.ascontiguousarray(np.concatenate([be[:, be.shape[1] - sbits // 8:], counts[:n].astype("<u2").view(np.uint8).reshape(n, 2)], axis=1).reshape(-1))
    return np.searchsorted(pref, np.arange(1 << (2 * p), dtype=np.uint64), side="left").astype(np.uint64), recs, n


def timed(torch, fn):
    ms, res = [], None
    for it in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        if it:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms) / 1e3, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8_000_000, help="database records")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "db_transform_bench.json"))
    ap.add_argument("--no-reference", action="store_true", help="do not time oracle/_ref/kmc_tools")
    a = ap.parse_args()
    import torch  # before libkmc_hip.so is loaded: the library then binds the HIP runtime torch brought, and the process holds one copy of it

    capi.require_gpu_backend()
    ctx = capi.Context((0,))
    ref = os.path.join(ROOT, "oracle", "_ref", "kmc_tools")
    res = dict(n_records=a.n, counter_bytes=2, k={})
    for k in (27, 55, 127):
        rng = np.random.default_rng(k)
        draws = dict(uniform=rng.integers(1, 256, size=a.n).astype(np.uint32),
                     spectrum=np.where(rng.random(a.n) < 0.7, 1, 1 + rng.geometric(0.02, size=a.n)).astype(np.uint32))
        p = dbio.best_lut_prefix_len(k, a.n)
        lut, recs, n = random_body(rng, k, p, a.n, draws["spectrum"])
        rb = (k - p) // 4 + 2
        text_cap = n * (k + 12)
        d = dict(recs=ctx.malloc(recs.nbytes + 256), lut=ctx.malloc(lut.nbytes), text=ctx.malloc(text_cap + 256), out=ctx.malloc(n * rb + 256), lut_out=ctx.malloc(lut.nbytes),
                 hist=ctx.malloc(8 * 255))
        ctx.h2d(d["recs"], recs)
        ctx.h2d(d["lut"], lut)
        view = capi.DbView(d["recs"], n, d["lut"], p, 2, 1, 0xFFFFFFFF)
        row = dict(records=n, lut_prefix_len=p, record_bytes=rb)
        t, (n_bytes, st) = timed(torch, lambda: ctx.db_dump_device(k, view, 1, 0, n, 1, 0xFFFFFFFF, 0xFFFFFFFF, d["text"], text_cap))
        row["dump"] = dict(ms_median_of_5=t * 1e3, g_records_per_s=n / t / 1e9, text_gb_per_s=n_bytes / t / 1e9, text_bytes=n_bytes, tallies=st)
        t, (n_out, st) = timed(torch, lambda: ctx.db_reduce_device(k, view, 2, 200, 255, 0, p, d["out"], n * rb, d["lut_out"]))
        row["reduce"] = dict(ms_median_of_5=t * 1e3, g_records_per_s=n / t / 1e9, tallies=st)
        row["histogram"] = {}
        for name in ("spectrum", "uniform"):
            if name == "uniform":  # the same records, the other counters
                r2 = recs.reshape(n, rb).copy()
                r2[:, rb - 2:] = draws["uniform"][:n].astype("<u2").view(np.uint8).reshape(n, 2)
                ctx.h2d(d["recs"], r2.reshape(-1))
            t, st = timed(torch, lambda: ctx.db_histogram_device(k, view, 1, 1, 255, d["hist"]))
            hist = np.zeros(255, dtype=np.uint64)
            ctx.d2h(hist, d["hist"])
            assert np.array_equal(hist, np.bincount(draws[name][:n], minlength=256)[1:256].astype(np.uint64))
            row["histogram"][name] = dict(ms_median_of_5=t * 1e3, g_records_per_s=n / t / 1e9, share_of_ones=float(hist[0]) / n, tallies=st)
        row["histogram"]["spectrum_over_uniform"] = row["histogram"]["spectrum"]["g_records_per_s"] / row["histogram"]["uniform"]["g_records_per_s"]
        for x in d.values():
            ctx.free(x)
        if os.path.exists(ref) and not a.no_reference:
            with tempfile.TemporaryDirectory() as td:
                dbio.write_kmc1(os.path.join(td, "db"), k, 2, p, 1, 65535, True, lut, recs)
                row["reference_kmc_tools_t16_wall_s"] = {}
                for name, args in (("dump", ["dump", os.path.join(td, "o.txt")]), ("reduce", ["reduce", os.path.join(td, "o"), "-ci2", "-cx200", "-cs255"]),
                                   ("histogram", ["histogram", os.path.join(td, "h.txt"), "-cx255"])):
                    t0 = time.perf_counter()
                    subprocess.run([ref, "-t16", "-hp", "transform", os.path.join(td, "db"), *args], check=True, capture_output=True)
                    row["reference_kmc_tools_t16_wall_s"][name] = time.perf_counter() - t0
        res["k"][str(k)] = row
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
