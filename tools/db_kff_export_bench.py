"""A database body framed as KFF records on the device (kmc_hip_db_kff_export_device, k_kff_frame): for k = 27, 55 and 127 a body of 8 M random k-mers already in HBM,
two counter bytes, data_size 2. Device time by HIP events around each synchronous call, medians of 5 after a warm-up, and the spread (min .. max) of those 5:
  one_segment    an ordered body under the LUT of the prefix length of its size
  512_segments   the same records dealt into 512 ascending bins in file order under the segmented LUT (the smallest valid prefix length), as a KMC2 body has it
GB/s are bytes read plus written (the body's records and the KFF records; the LUT is not counted), next to one plain device-to-device copy of the OUTPUT bytes (its
bytes read plus written) on the same box, and the ratio. The output of the one-segment leg is checked against the record restated in numpy before anything is timed.
A figure that could not be taken is written as "NOT MEASURED" with the reason.

    python tools/db_kff_export_bench.py [--n 8000000] [--k 27 55 127] [--out profiles/r14/db_kff_export_bench.json]
For the kernel alone run it under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/db_kff_export_bench.py --k <k> --only <shape>`, a profiler run of
its own per k and shape (6 calls: k_kff_frame's row is then one k and one shape), and collect the statistics files:
    python tools/db_kff_export_bench.py --collect 27:one_segment:<stats.csv> ... [--bench profiles/r14/db_kff_export_bench.json] [--trace-out profiles/r14/db_kff_export_kernel_trace.json]
With --bench the kernel's own rate and its ratio to the copy measured there are added.
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SEGMENTS = 512
SHAPES = ("one_segment", "512_segments")


def random_keys(rng, k, n):
    """n distinct ascending random k-mers as big-endian bytes uint8[n, ceil(k / 4)], padding bits zero: the leading (at most 8) bytes distinct and ascending"""
    kb = (k + 3) // 4
    tb = min(kb, 8)
    bits = 2 * k - 8 * (kb - tb)
    assert bits < 64
    top = np.unique(rng.integers(0, 1 << bits, size=n + n // 50, dtype=np.uint64))[:n]
    assert top.size == n
    return np.concatenate([top.astype(">u8").view(np.uint8).reshape(n, 8)[:, 8 - tb:], rng.integers(0, 256, size=(n, kb - tb), dtype=np.uint8)], axis=1)


def prefixes_of(key, k, p):
    pb = key.shape[1] - (k - p) // 4
    x = np.zeros(key.shape[0], dtype=np.uint64)
    for q in range(pb):
        x = (x << np.uint64(8)) | key[:, q].astype(np.uint64)
    return x


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
    bench = json.load(open(a.bench)) if a.bench and os.path.exists(a.bench) else None
    res = dict(source="rocprofv3 --kernel-trace --stats over tools/db_kff_export_bench.py --only <shape>, one profiler run per entry below (6 calls each); microseconds", k_kff_frame={})
    for spec in a.collect:
        k, shape, path = spec.split(":", 2)
        with open(path) as f:
            rows = {re.sub(r"\(.*", "", r["Name"]).replace("void ", ""): r for r in csv.DictReader(f)}
        r = rows["k_kff_frame"]
        row = dict(calls=int(r["Calls"]), total_us=int(r["TotalDurationNs"]) / 1e3, avg_us=float(r["AverageNs"]) / 1e3, min_us=int(r["MinNs"]) / 1e3, max_us=int(r["MaxNs"]) / 1e3)
        if bench and k in bench["k"]:
            b = bench["k"][k]
            row["gb_per_s_read_plus_written"] = b["bytes_read_plus_written"][shape] / row["avg_us"] / 1e3
            row["over_memcpy"] = row["gb_per_s_read_plus_written"] / b["memcpy_of_the_output"]["gb_per_s_read_plus_written"]
        res["k_kff_frame"].setdefault(k, {})[shape] = row
    os.makedirs(os.path.dirname(a.trace_out), exist_ok=True)
    with open(a.trace_out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8_000_000, help="records")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "db_kff_export_bench.json"))
    ap.add_argument("--k", type=int, nargs="+", default=[27, 55, 127], help="k-mer lengths")
    ap.add_argument("--only", choices=SHAPES, help="nothing but the export call on that shape (for a kernel trace that keeps the shapes apart); writes no file")
    ap.add_argument("--collect", nargs="*", help="k:shape:stats.csv of --only runs under the profiler: writes --trace-out and leaves")
    ap.add_argument("--bench", default=os.path.join(ROOT, "profiles", "r14", "db_kff_export_bench.json"), help="with --collect: the bench file whose copy the kernel is set against")
    ap.add_argument("--trace-out", default=os.path.join(ROOT, "profiles", "r14", "db_kff_export_kernel_trace.json"))
    a = ap.parse_args()
    if a.collect is not None:
        return collect(a)
    import torch  # before libkmc_hip.so is loaded: the library then binds the HIP runtime torch brought, and the process holds one copy of it

    from kmc_amd import capi, dbio

    capi.require_gpu_backend()
    ctx = capi.Context((0,))
    cs = ds = 2
    res = dict(n_records=a.n, counter_bytes=cs, data_size=ds, n_segments=N_SEGMENTS,
               per_kernel_split="kernel times come from a profiler run of its own: profiles/r14/db_kff_export_kernel_trace.json (--collect)", k={})
    for k in a.k:
        rng = np.random.default_rng(k)
        n = a.n
        key = random_keys(rng, k, n)
        counts = np.where(rng.random(n) < 0.7, 1, 1 + rng.geometric(0.02, size=n)).astype(np.uint16)
        le, be = counts.astype("<u2").view(np.uint8).reshape(n, 2), counts.astype(">u2").view(np.uint8).reshape(n, 2)
        kb = key.shape[1]
        want = np.concatenate([key, be], axis=1)
        sec = rng.integers(0, N_SEGMENTS, size=n)
        order = np.argsort(sec, kind="stable")
        starts = np.concatenate([[0], np.cumsum(np.bincount(sec, minlength=N_SEGMENTS))]).astype(np.int64)
        p1, p0 = dbio.best_lut_prefix_len(k, n), dbio.best_lut_prefix_len(k, 0)
        rb_out = kb + ds
        row = dict(records=n, kff_record_bytes=rb_out, bytes_read_plus_written={})
        d_kff = ctx.malloc(n * rb_out + 256)
        for shape, p, perm in (("one_segment", p1, None), ("512_segments", p0, order)):
            if a.only not in (None, shape):
                continue
            kk = key if perm is None else key[perm]
            sb = (k - p) // 4
            recs = np.ascontiguousarray(np.concatenate([kk[:, kb - sb:], le if perm is None else le[perm]], axis=1))
            pref = prefixes_of(kk, k, p)
            ent = np.arange(1 << (2 * p), dtype=np.uint64)
            if perm is None:
                lut, n_seg = np.searchsorted(pref, ent, side="left").astype(np.uint64), 1
            else:
                lut = np.concatenate([starts[s] + np.searchsorted(pref[starts[s]:starts[s + 1]], ent, side="left") for s in range(N_SEGMENTS)] + [[n]]).astype(np.uint64)
                n_seg = N_SEGMENTS
            d_recs, d_lut = ctx.malloc(recs.nbytes + 256), ctx.malloc(lut.nbytes + 256)
            ctx.h2d(d_recs, recs.reshape(-1))
            ctx.h2d(d_lut, lut)
            view = capi.DbView(d_recs, n, d_lut, p, cs, 1, 65535)
            t, got = timed(torch, lambda: ctx.db_kff_export_device(k, view, n_seg, 0, n, ds, d_kff, n * rb_out))
            assert got == n * rb_out
            out = np.zeros(n * rb_out, dtype=np.uint8)
            ctx.d2h(out, d_kff)
            assert np.array_equal(out.reshape(n, rb_out), want if perm is None else want[perm]), f"k = {k}, {shape}: the KFF records differ from the restatement"
            moved = n * (sb + cs + rb_out)
            row["bytes_read_plus_written"][shape] = moved
            row[shape] = dict(t, lut_prefix_len=p, record_bytes=sb + cs, lut_entries=int(lut.size), gb_per_s_read_plus_written=moved / t["ms_median_of_5"] / 1e6)
            ctx.free(d_recs)
            ctx.free(d_lut)
        ctx.free(d_kff)
        if a.only:
            print(json.dumps({str(k): row}), flush=True)
            continue
        src, dst = torch.empty(n * rb_out, dtype=torch.uint8, device="cuda"), torch.empty(n * rb_out, dtype=torch.uint8, device="cuda")
        t, _ = timed(torch, lambda: dst.copy_(src))
        row["memcpy_of_the_output"] = dict(t, gb_per_s_read_plus_written=2 * n * rb_out / t["ms_median_of_5"] / 1e6)
        del src, dst
        for shape in SHAPES:
            row[shape]["over_memcpy"] = row[shape]["gb_per_s_read_plus_written"] / row["memcpy_of_the_output"]["gb_per_s_read_plus_written"]
        res["k"][str(k)] = row
        print(json.dumps({str(k): row}), flush=True)
    ctx.close()
    if a.only:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
