"""Set operations between two ordered databases on the device (kmc_hip_db_set_op_device): two synthetic ordered databases at k = 27 with a given share of
common k-mers, union and intersect. Device time by HIP events around the call (medians of 7), as Gk-mers/s of input records and as a fraction of 8 TB/s by the
bytes of DESIGN.md §9: both unpacked inputs read twice (the count and the write launches of k_so_tile), the kept records written, the pack read and written.
Where oracle/_ref/kmc_tools is present, the reference's `simple` is timed on the same databases (wall time, files in a temporary directory).

    python tools/db_setops_bench.py [--n 16000000] [--shared 0.5] [--out profiles/r07/db_setops_bench.json]
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

K, P, CB = 27, 3, 1


def body(kmers, counts):
    suf = (kmers & np.uint64((1 << 48) - 1)).astype(">u8").view(np.uint8).reshape(-1, 8)[:, 2:]
    recs = np.ascontiguousarray(np.concatenate([suf, counts.astype(np.uint8)[:, None]], axis=1).reshape(-1))
    lut = np.searchsorted(kmers >> np.uint64(48), np.arange(64, dtype=np.uint64), side="left").astype(np.uint64)
    return lut, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16_000_000, help="records per input")
    ap.add_argument("--shared", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "db_setops_bench.json"))
    a = ap.parse_args()
    capi.require_gpu_backend()
    import torch

    rng = np.random.default_rng(1)
    n_sh = int(a.n * a.shared)
    pool = np.unique(rng.integers(0, 1 << 54, size=int((2 * a.n - n_sh) * 1.02) + 1000, dtype=np.uint64))
    pool = pool[rng.permutation(pool.size)][: 2 * a.n - n_sh]
    ka, kb = np.sort(pool[: a.n]), np.sort(pool[a.n - n_sh:])
    ca, cb = rng.integers(1, 100, size=ka.size), rng.integers(1, 100, size=kb.size)
    bodies = [body(ka, ca), body(kb, cb)]
    ctx = capi.Context((0,))
    rb = (K - P) // 4 + CB
    dev = []
    for lut, recs in bodies:
        d_r, d_l = ctx.malloc(recs.nbytes + 256), ctx.malloc(lut.nbytes)
        ctx.h2d(d_r, recs)
        ctx.h2d(d_l, lut)
        dev.append((d_r, d_l))
    views = [capi.DbView(d[0], a.n, d[1], P, CB, 1, 255) for d in dev]
    d_out, d_lut = ctx.malloc(2 * a.n * rb + 256), ctx.malloc(8 << (2 * P))
    res = dict(k=K, n_per_input=a.n, shared=a.shared, ops={})
    for op, oc in (("union", "sum"), ("intersect", "min")):
        o = capi.DbOp(capi.DB_OPS[op], capi.DB_COUNTER_OPS[oc], 1, 255, 255, P)
        ms = []
        for it in range(8):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            n, st = ctx.db_set_op_device(K, views[0], views[1], o, d_out, 2 * a.n * rb, d_lut)
            e1.record()
            e1.synchronize()
            if it:
                ms.append(e0.elapsed_time(e1))
        t = statistics.median(ms) / 1e3
        unpacked = 16  # one k-mer word + one count word
        nbytes = 2 * a.n * rb + 2 * a.n * unpacked + 2 * (2 * a.n * unpacked) + n * unpacked + n * unpacked + n * rb
        res["ops"][op] = dict(ms_median_of_7=t * 1e3, written=n, tallies=st, gkmers_per_s_of_input=2 * a.n / t / 1e9, bytes=nbytes, fraction_of_8TBps=nbytes / t / 8e12)
    ref = os.path.join(ROOT, "oracle", "_ref", "kmc_tools")
    if os.path.exists(ref):
        with tempfile.TemporaryDirectory() as td:
            for name, (lut, recs) in zip("ab", bodies):
                dbio.write_kmc1(os.path.join(td, name), K, CB, P, 1, 255, True, lut, recs)
            for op in ("union", "intersect"):
                t0 = time.perf_counter()
                subprocess.run([ref, "simple", os.path.join(td, "a"), os.path.join(td, "b"), op, os.path.join(td, "o_" + op)], check=True, capture_output=True)
                res["ops"][op]["reference_kmc_tools_wall_s"] = time.perf_counter() - t0
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
