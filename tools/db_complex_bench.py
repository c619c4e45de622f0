"""A set expression over several ordered databases on the device (kmc_hip_db_expr_device): left-deep unions (sum) and intersections (min) of N = 2, 4 and 8 synthetic
ordered databases of 8 M random k-mers already in HBM, two counter bytes, at k = 27, 55 and 127. Every database is a random half of one pool of 16 M k-mers, so any two
share about half of their k-mers. Device time by HIP events around the whole synchronous call (medians of 5 after one warm-up call).
On the same data, what the call replaces:
  chain      N - 1 kmc_hip_db_set_op_device calls, every intermediate database written and read again. NOT equivalent in counters in general: every call of the chain
             applies the output's cutoffs and clamp, the expression only at its root. (On this data no counter reaches the clamp, and the outputs are compared.)
  set_op     for N = 2, the single kmc_hip_db_set_op_device call.
Where oracle/_ref/kmc_tools is present, the whole process `kmc_tools -t16 complex <file>` is timed on the same databases from disk (wall time).

    python tools/db_complex_bench.py [--n 8000000] [--out profiles/r08/db_complex_bench.json] [--no-reference]
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

NS = (2, 4, 8)
OPS = (("union", "sum", "+"), ("intersect", "min", "*"))
CB = 2
U16 = 65535


def random_pool(rng, k, n):
    """n ascending distinct random k-mers as rows of 64-bit words, word 0 least significant"""
    words = (k + 31) // 32
    km = rng.integers(0, 1 << 63, size=(n, words), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, words), dtype=np.uint64)
    top = 2 * k - 64 * (words - 1)
    if top < 64:
        km[:, words - 1] &= np.uint64((1 << top) - 1)
    km = km[np.lexsort([km[:, w] for w in range(words)])]
    return km[np.concatenate([[True], (km[1:] != km[:-1]).any(axis=1)])]


def body(km, k, p, counts):
    """ascending k-mers -> (LUT, records with two counter bytes)"""
    n, words = km.shape
    sbits = 2 * (k - p)
    w, r = sbits // 64, sbits % 64
    pref = km[:, w] >> np.uint64(r)
    if r and w + 1 < words:
        pref = pref | (km[:, w + 1] << np.uint64(64 - r))
    pref = pref & np.uint64((1 << (2 * p)) - 1)
    be = np.ascontiguousarray(km[:, ::-1]).astype(">u8").view(np.uint8).reshape(n, -1)
    recs = np.ascontiguousarray(np.concatenate([be[:, be.shape[1] - sbits // 8:], counts.astype("<u2").view(np.uint8).reshape(n, 2)], axis=1).reshape(-1))
    return np.searchsorted(pref, np.arange(1 << (2 * p), dtype=np.uint64), side="left").astype(np.uint64), recs


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
    ap.add_argument("--n", type=int, default=8_000_000, help="records per database")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "db_complex_bench.json"))
    ap.add_argument("--no-reference", action="store_true", help="do not time oracle/_ref/kmc_tools")
    a = ap.parse_args()
    import torch  # before libkmc_hip.so is loaded: the library then binds the HIP runtime torch brought, and the process holds one copy of it

    capi.require_gpu_backend()
    ctx = capi.Context((0,))
    ref = os.path.join(ROOT, "oracle", "_ref", "kmc_tools")
    res = dict(n_records_per_database=a.n, counter_bytes=CB, note="chain: N - 1 kmc_hip_db_set_op_device calls; not equivalent to the expression in counters in general "
               "(every call applies cutoffs and clamp); on this data the outputs are equal and are compared", k={})
    n_max = max(NS)
    for k in (27, 55, 127):
        rng = np.random.default_rng(k)
        pool = random_pool(rng, k, 2 * a.n)
        p = dbio.best_lut_prefix_len(k, a.n)
        rb = (k - p) // 4 + CB
        bodies, views, allocs = [], [], []
        for i in range(n_max):
            km = pool[rng.random(pool.shape[0]) < 0.5]
            lut, recs = body(km, k, p, rng.integers(1, 256, size=km.shape[0]).astype(np.uint32))
            d_r, d_l = ctx.malloc(recs.nbytes + 256), ctx.malloc(lut.nbytes)
            ctx.h2d(d_r, recs)
            ctx.h2d(d_l, lut)
            allocs += [d_r, d_l]
            bodies.append((lut, recs, km.shape[0]))
            views.append(capi.DbView(d_r, km.shape[0], d_l, p, CB, 1, U16))
        cap = sum(b[2] for b in bodies) * rb
        outs = [(ctx.malloc(cap + 256), ctx.malloc(8 << (2 * p))) for _ in range(3)]
        row = dict(lut_prefix_len=p, record_bytes=rb, records=[b[2] for b in bodies])
        for op, oc, sign in OPS:
            row[op] = {}
            for N in NS:
                n_in = sum(b[2] for b in bodies[:N])
                steps = [(capi.DB_EXPR_INPUT, 0)]
                for i in range(1, N):
                    steps += [(capi.DB_EXPR_INPUT, i), (capi.DB_OPS[op], capi.DB_COUNTER_OPS[oc])]
                out = capi.DbOp(0, 0, 1, U16, U16, p)
                t, (n_out, st) = timed(torch, lambda: ctx.db_expr_device(k, views[:N], steps, out, outs[0][0], cap, outs[0][1]))
                got = np.zeros(n_out * rb, dtype=np.uint8)
                ctx.d2h(got, outs[0][0])
                o = capi.DbOp(capi.DB_OPS[op], capi.DB_COUNTER_OPS[oc], 1, U16, U16, p)

                def chain():
                    acc, n_acc = views[0], 0
                    for i in range(1, N):
                        d_o, d_l = outs[1 + i % 2]
                        n_acc, _ = ctx.db_set_op_device(k, acc, views[i], o, d_o, cap, d_l)
                        acc = capi.DbView(d_o, n_acc, d_l, p, CB, 1, U16)
                    return n_acc, 1 + (N - 1) % 2

                tc, (n_chain, last) = timed(torch, chain)
                chained = np.zeros(n_chain * rb, dtype=np.uint8)
                ctx.d2h(chained, outs[last][0])
                assert n_chain == n_out and np.array_equal(got, chained), (k, op, N)
                row[op][str(N)] = dict(expr_ms_median_of_5=t * 1e3, g_input_records_per_s=n_in / t / 1e9, input_records=n_in, written=n_out, tallies=st,
                                       chain_ms_median_of_5=tc * 1e3, chain_over_expr=tc / t)
                if N == 2:
                    row[op]["2"]["set_op_ms_median_of_5"] = tc * 1e3  # the chain of one call is the set_op call
                    row[op]["2"]["expr_over_set_op"] = t / tc
            ts = [row[op][str(N)]["expr_ms_median_of_5"] for N in NS]
            tcs = [row[op][str(N)]["chain_ms_median_of_5"] for N in NS]
            row[op]["expr_time_8_over_2"], row[op]["chain_time_8_over_2"] = ts[-1] / ts[0], tcs[-1] / tcs[0]
        for d_o, d_l in outs:
            ctx.free(d_o)
            ctx.free(d_l)
        for d in allocs:
            ctx.free(d)
        if os.path.exists(ref) and not a.no_reference:
            with tempfile.TemporaryDirectory() as td:
                for i, (lut, recs, _) in enumerate(bodies):
                    dbio.write_kmc1(os.path.join(td, f"db{i}"), k, CB, p, 1, U16, True, lut, recs)
                for op, oc, sign in OPS:
                    for N in NS:
                        definition = os.path.join(td, "def.txt")
                        with open(definition, "w") as f:
                            f.write("INPUT:\n" + "".join(f"d{i} = {os.path.join(td, f'db{i}')}\n" for i in range(N)) + f"OUTPUT:\n{os.path.join(td, 'o')} = " +
                                    f" {sign} ".join(f"d{i}" for i in range(N)) + "\n")
                        t0 = time.perf_counter()
                        subprocess.run([ref, "-t16", "-hp", "complex", definition], check=True, capture_output=True)
                        row[op][str(N)]["reference_kmc_tools_t16_wall_s"] = time.perf_counter() - t0
        res["k"][str(k)] = row
        print(f"k={k}: " + json.dumps(row), flush=True)
        del pool, bodies
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
