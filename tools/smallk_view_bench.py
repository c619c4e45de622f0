"""The small-k table as a database on the device (kmc_hip_smallk_tally / kmc_hip_smallk_view_device: k_sk_tally, k_db_cumsum, k_sk_emit) on one MI355X: for k = 9, 11 and 13
a table of 4^k uint64 counters planted in HBM and handed over through d_table, at three densities:
  dense      every entry kept
  one_in_64  1 entry in 64 non-zero, all of them kept
  spectrum   a spectrum-like draw: half of the entries non-zero, 70 % of those ones, with -ci2 (the ones fall below the threshold)
Device time by HIP events around each synchronous call, medians of 5 after a warm-up, and the spread (min .. max) of those 5; -cx 1e9, -cs 255 (one counter byte), the
LUT prefix length tools.smallk_lut_prefix_len picks. In the same run, per k: a plain device-to-device copy of the table's bytes (the view call reads the table twice, once
per kernel, so its floor is two reads plus the body written) and the road this replaces, kmc_hip_smallk_read of the whole table into pageable host memory. The view's body is
checked against numpy before anything is timed. The table is 2 MB at k = 9 and 32 MB at k = 11: both sit in the 256 MiB last-level cache between the calls of a timing
loop, so those rates are cache rates, not HBM rates — only k = 13 (512 MB) streams from HBM. A figure that could not be taken is written as "NOT MEASURED" with the reason.

    python tools/smallk_view_bench.py [--k 9 11 13] [--out profiles/r15/smallk_view_bench.json]
For the split into tally / scan / emit run it under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/smallk_view_bench.py --only 13:spectrum`, a
profiler run of its own (6 view calls and nothing else timed), and collect the statistics file:
    python tools/smallk_view_bench.py --collect 13:spectrum:<stats.csv> ... [--trace-out profiles/r15/smallk_view_kernel_trace.json]
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DENSITIES = ("dense", "one_in_64", "spectrum")
CX, CS = 10**9, 255


def table_of(k, density):
    n = 1 << (2 * k)
    rng = np.random.default_rng([k, DENSITIES.index(density)])
    if density == "dense":
        return rng.integers(2, 200, size=n, dtype=np.uint64), 1
    if density == "one_in_64":
        t = np.zeros(n, dtype=np.uint64)
        at = rng.random(n) < 1 / 64
        t[at] = rng.integers(2, 200, size=int(at.sum()), dtype=np.uint64)
        return t, 1
    t = np.where(rng.random(n) < 0.7, 1, 1 + rng.geometric(0.02, size=n)).astype(np.uint64)
    t[rng.random(n) < 0.5] = 0
    return t, 2


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


def collect(a):
    res = dict(source="rocprofv3 --kernel-trace --stats over tools/smallk_view_bench.py --only <k>:<density>, one profiler run per entry below (one tally call and 6 view calls each: 7 "
                      "k_sk_tally launches — the view tallies before it writes —, 7 scans, 6 k_sk_emit); microseconds", runs={})
    for spec in a.collect:
        k, density, path = spec.split(":", 2)
        with open(path) as f:
            rows = {re.sub(r"\(.*", "", r["Name"]).replace("void ", ""): r for r in csv.DictReader(f)}
        run = {}
        for name, r in rows.items():
            if name.startswith(("k_sk_", "k_db_cumsum")):
                run[name] = dict(calls=int(r["Calls"]), total_us=int(r["TotalDurationNs"]) / 1e3, avg_us=float(r["AverageNs"]) / 1e3, min_us=int(r["MinNs"]) / 1e3, max_us=int(r["MaxNs"]) / 1e3)
        res["runs"].setdefault(k, {})[density] = run
    os.makedirs(os.path.dirname(a.trace_out), exist_ok=True)
    with open(a.trace_out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[9, 11, 13])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "smallk_view_bench.json"))
    ap.add_argument("--only", help="<k>:<density>: nothing but six view calls on that table (for a kernel trace); writes no file")
    ap.add_argument("--collect", nargs="*", help="k:density:stats.csv of --only runs under the profiler: writes --trace-out and leaves")
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "r15", "smallk_view_kernel_trace.json"))
    a = ap.parse_args()
    if a.collect is not None:
        return collect(a)
    import torch  # before libkmc_hip.so is loaded: the library then binds the HIP runtime torch brought, and the process holds one copy of it

    from kmc_amd import capi, tools

    capi.require_gpu_backend()
    ctx = capi.Context((0,))
    L, u64p = ctx.L, C.POINTER(C.c_uint64)
    only = tuple(a.only.split(":")) if a.only else None
    res = dict(cutoff_max=CX, counter_max=CS, counter_bytes=1,
               cache_note="the table is 2 MB at k = 9 and 32 MB at k = 11 and stays in the 256 MiB last-level cache between the timed calls: cache rates; k = 13 (512 MB) streams from HBM",
               per_kernel_split="kernel times come from a profiler run of its own: profiles/r15/smallk_view_kernel_trace.json (--collect), else NOT MEASURED", k={})
    for k in ([int(only[0])] if only else a.k):
        n = 1 << (2 * k)
        row = dict(entries=n, table_bytes=8 * n)
        d_table = ctx.malloc(8 * n)
        for density in ([only[1]] if only else DENSITIES):
            table, ci = table_of(k, density)
            ctx.h2d(d_table, table)
            st = np.zeros(4, dtype=np.uint64)

            def tally():
                ctx._chk(L.kmc_hip_smallk_tally(ctx.h, 0, d_table, k, ci, CX, st.ctypes.data_as(u64p)))

            tally()
            unique, kept = int(st[0]), int(st[3])
            p = tools.smallk_lut_prefix_len(k, unique, 1)
            rb = (k - p) // 4 + 1
            d_out, d_lut = ctx.malloc(kept * rb + 256), ctx.malloc(8 << (2 * p))
            v, nk = capi.DbView(), C.c_uint64(0)

            def view():
                ctx._chk(L.kmc_hip_smallk_view_device(ctx.h, 0, d_table, k, 1, ci, CX, CS, 0, p, 0, d_out, kept * rb, d_lut, C.byref(v), C.byref(nk), st.ctypes.data_as(u64p)))

            view()
            keep = (table >= ci) & (table != 0)
            idx = np.flatnonzero(keep).astype(np.uint64)
            sb = rb - 1
            want = np.stack([((idx >> np.uint64(8 * (sb - 1 - j))) & np.uint64(255)) for j in range(sb)] + [np.minimum(table[keep], np.uint64(CS))], axis=1).astype(np.uint8)
            got = np.zeros(kept * rb, dtype=np.uint8)
            ctx.d2h(got, d_out)
            assert nk.value == kept == idx.size and np.array_equal(got, want.reshape(-1)), f"k = {k}, {density}: the body differs from the restatement"
            del want, got, idx, keep
            if only:
                for _ in range(5):
                    view()
            else:
                t_tally, _ = timed(torch, tally)
                t_view, _ = timed(torch, view)
                moved = 2 * 8 * n + kept * rb + (8 << (2 * p))  # the table read by both kernels, the body and the LUT written
                row[density] = dict(cutoff_min=ci, unique=unique, kept=kept, lut_prefix_len=p, record_bytes=rb, tally=dict(t_tally, gb_per_s_read=8 * n / t_tally["ms_median_of_5"] / 1e6),
                                    view=dict(t_view, bytes_read_plus_written=moved, gb_per_s_read_plus_written=moved / t_view["ms_median_of_5"] / 1e6))
            ctx.free(d_out)
            ctx.free(d_lut)
        ctx.free(d_table)
        if only:
            continue
        src, dst = torch.empty(8 * n, dtype=torch.uint8, device="cuda"), torch.empty(8 * n, dtype=torch.uint8, device="cuda")
        t, _ = timed(torch, lambda: dst.copy_(src))
        row["memcpy_of_the_table"] = dict(t, gb_per_s_read_plus_written=2 * 8 * n / t["ms_median_of_5"] / 1e6)
        del src, dst
        sk = capi.SmallK(ctx, k, True)
        try:
            host = np.ones(n, dtype=np.uint64)  # touched: the page faults are not the link's
            t, _ = timed(torch, lambda: ctx._chk(L.kmc_hip_smallk_read(ctx.h, 0, 0, n, host.ctypes.data)))
            row["read_back_to_host"] = dict(t, gb_per_s=8 * n / t["ms_median_of_5"] / 1e6, note="kmc_hip_smallk_read of the whole table into a pageable numpy array")
        finally:
            sk.close()
        for density in DENSITIES:
            d = row[density]["view"]
            d["over_memcpy_time"] = d["ms_median_of_5"] / row["memcpy_of_the_table"]["ms_median_of_5"]
            d["read_back_over_view_time"] = row["read_back_to_host"]["ms_median_of_5"] / d["ms_median_of_5"]
        res["k"][str(k)] = row
        print(json.dumps({str(k): row}), flush=True)
    ctx.close()
    if only:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
