"""Two ordered databases compared on the device (kmc_hip_db_compare_device): for k = 27, 55 and 127 two equal synthetic databases of 8 M random k-mers already in HBM,
two counter bytes. Device time by HIP events around the synchronous call (medians of 5 after a warm-up, min to max beside them):
  equal         the whole walk runs
  first, middle a counter changed at record 0 and at the middle record: what the tile skip buys
  thinned       every second record of B carries a counter its cutoffs remove, and A is B without those records: the compaction of one input, then the whole walk
Beside each the rate of a plain device-to-device copy (hipMemcpyAsync) of as many bytes as k_db_compare reads on equal inputs: both unpacked arrays. Where
oracle/_ref/kmc_tools is present, the whole process `kmc_tools -t16 compare` is timed on the equal pair from disk (wall time); the child processes run before the
device is opened.

    python tools/db_compare_bench.py [--n 8000000] [--k 27,55,127] [--out profiles/r13/db_compare_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from db_transform_bench import random_body  # noqa: E402
from kmc_amd import capi, dbio  # noqa: E402


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
    return dict(ms_median_of_5=statistics.median(ms), ms_min=min(ms), ms_max=max(ms)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8_000_000, help="database records")
    ap.add_argument("--k", default="27,55,127")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "db_compare_bench.json"))
    ap.add_argument("--no-reference", action="store_true", help="do not time oracle/_ref/kmc_tools")
    a = ap.parse_args()
    ks = [int(x) for x in a.k.split(",")]
    ref = os.path.join(ROOT, "oracle", "_ref", "kmc_tools")
    res = dict(n_records=a.n, counter_bytes=2, k={})
    data = {}
    for k in ks:  # the databases, and the reference on them, before the device is opened
        rng = np.random.default_rng(k)
        p = dbio.best_lut_prefix_len(k, a.n)
        counts = rng.integers(2, 60000, size=a.n).astype(np.uint32)  # 2 and more: the planted change (the low bit flipped) stays inside the cutoffs
        lut, recs, n = random_body(rng, k, p, a.n, counts)
        data[k] = (p, lut, recs, n)
        row = res["k"][str(k)] = dict(records=n, lut_prefix_len=p, record_bytes=(k - p) // 4 + 2, unpacked_words=(k + 31) // 32 + 1)
        if os.path.exists(ref) and not a.no_reference:
            with tempfile.TemporaryDirectory() as td:
                for name in "ab":
                    dbio.write_kmc1(os.path.join(td, name), k, 2, p, 1, 65535, True, lut, recs)
                t0 = time.perf_counter()
                r = subprocess.run([ref, "-t16", "-hp", "compare", os.path.join(td, "a"), os.path.join(td, "b")], capture_output=True, text=True)
                row["reference_kmc_tools_t16_wall_s"] = time.perf_counter() - t0
                assert r.returncode == 0 and r.stdout == "DB Equals\n", (r.returncode, r.stdout, r.stderr)
        else:
            row["reference_kmc_tools_t16_wall_s"] = "NOT MEASURED"
    import torch  # before libkmc_hip.so is loaded: the library then binds the HIP runtime torch brought, and the process holds one copy of it

    capi.require_gpu_backend()
    ctx = capi.Context((0,))
    for k in ks:
        p, lut, recs, n = data[k]
        row = res["k"][str(k)]
        rb = row["record_bytes"]
        d = dict(a=ctx.malloc(recs.nbytes + 256), b=ctx.malloc(recs.nbytes + 256), lut=ctx.malloc(lut.nbytes))
        ctx.h2d(d["a"], recs)
        ctx.h2d(d["b"], recs)
        ctx.h2d(d["lut"], lut)
        va, vb = (capi.DbView(d[q], n, d["lut"], p, 2, 1, 0xFFFFFFFF) for q in "ab")
        read_bytes = 2 * n * row["unpacked_words"] * 8

        def rate(t):
            return dict(t, g_records_per_s=n / t["ms_median_of_5"] / 1e6, gb_per_s_of_unpacked_words=read_bytes / t["ms_median_of_5"] / 1e6)

        t, r = timed(torch, lambda: ctx.db_compare_device(k, va, vb))
        assert r["kind"] == 0 and r["n_a"] == n
        row["equal"] = rate(t)
        r2 = recs.reshape(n, rb)
        for name, at in (("first", 0), ("middle", n // 2)):
            patch = r2[at].copy()
            patch[rb - 2] ^= 1
            ctx.h2d(d["b"] + at * rb, patch)
            t, r = timed(torch, lambda: ctx.db_compare_device(k, va, vb))
            assert (r["kind"], r["ordinal"], r["record_a"], r["record_b"]) == (1, at, at, at), r
            row[name] = dict(t, share_of_equal=t["ms_median_of_5"] / row["equal"]["ms_median_of_5"])
            ctx.h2d(d["b"] + at * rb, r2[at].copy())
        # thinned: B is the database with the counter of every second record set to 60001; its cutoffs end at 60000. A holds the other records only
        thin = r2.copy()
        thin[1::2, rb - 2:] = np.array([60001], dtype="<u2").view(np.uint8)
        ctx.h2d(d["b"], thin.reshape(-1))
        half = np.ascontiguousarray(r2[0::2]).reshape(-1)
        m = half.size // rb
        # A's LUT: records with a prefix below i — every second record of the full database, so ceil(lut / 2)
        lut_half = ((lut + np.uint64(1)) // np.uint64(2)).astype(np.uint64)
        d["lut_half"] = ctx.malloc(lut_half.nbytes)
        ctx.h2d(d["a"], half)
        ctx.h2d(d["lut_half"], lut_half)
        va_half, vb_cut = capi.DbView(d["a"], m, d["lut_half"], p, 2, 1, 0xFFFFFFFF), capi.DbView(d["b"], n, d["lut"], p, 2, 1, 60000)
        t, r = timed(torch, lambda: ctx.db_compare_device(k, va_half, vb_cut))
        assert r["kind"] == 0 and r["n_a"] == m and r["n_b"] == m, r
        row["thinned"] = dict(t, g_input_records_per_s=(n + m) / t["ms_median_of_5"] / 1e6)
        for x in d.values():
            ctx.free(x)
        src, dst = torch.empty(read_bytes, dtype=torch.uint8, device="cuda"), torch.empty(read_bytes, dtype=torch.uint8, device="cuda")
        t, _ = timed(torch, lambda: dst.copy_(src))
        row["memcpy_of_the_bytes_read"] = dict(t, bytes=read_bytes, gb_per_s_copied=read_bytes / t["ms_median_of_5"] / 1e6)
        del src, dst
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
