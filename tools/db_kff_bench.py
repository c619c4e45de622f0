"""A KFF file's records imported as a database body on the device (kmc_hip_kff_import_device): for k = 27, 55 and 127 the KFF records of 8 M random k-mers already in
HBM, two counter bytes. Device time by HIP events around each synchronous call, medians of 5 after a warm-up, and the spread (min .. max) of those 5:
  repack     k_kff_repack alone (ordered = 0): the records as ONE section and the same records dealt into 512 ascending sections; GB/s read plus written, next to one
             plain device-to-device copy of the output bytes (its bytes read plus written) on the same box, and the ratio
  order      ordered = 1 on the 512 sections (unpack, the stable LSD sort, verify, pack) against kmc_hip_order_database_device on the same k-mers given as a KMC2
             database of 512 bins — the path the same job takes for a database `kmc` wrote; the two share the sort
Where oracle/_ref/kmc_tools is present, the whole process `kmc_tools -t16 transform <kff> sort <out>` is timed on the 512-section file from disk (wall time; context
only, a process against a call). A figure that could not be taken is written as "NOT MEASURED" with the reason.

    python tools/db_kff_bench.py [--n 8000000] [--k 27 55 127] [--out profiles/r11/db_kff_bench.json]
For the kernels alone run it under `rocprofv3 --kernel-trace --stats -- python tools/db_kff_bench.py --no-reference`, in a run of its own (with --k and --only-repack
one k and one section shape per run, so that k_kff_repack's rows are not mixed); tools/db_kff_trace.py collects the statistics files into profiles/r11/db_kff_kernel_trace.json.
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

N_SECTIONS = 512
P_BINS = 3  # lut_prefix_len of the KMC2 bins (k % 4 == 3 for every k measured)


def random_kmers(rng, k, n):
    """n distinct ascending random k-mers -> (words uint64[n, words] least significant first, big-endian bytes uint8[n, 8 x words])"""
    words = (k + 31) // 32
    km = rng.integers(0, 1 << 63, size=(n, words), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, words), dtype=np.uint64)
    top = 2 * k - 64 * (words - 1)
    if top < 64:
        km[:, words - 1] &= np.uint64((1 << top) - 1)
    km = km[np.lexsort([km[:, w] for w in range(words)])]
    km = km[np.concatenate([[True], (km[1:] != km[:-1]).any(axis=1)])]
    return km, np.ascontiguousarray(km[:, ::-1]).astype(">u8").view(np.uint8).reshape(km.shape[0], -1)


def prefix_of(km, k, p):
    sbits = 2 * (k - p)
    w, r = sbits // 64, sbits % 64
    pref = km[:, w] >> np.uint64(r)
    if r and w + 1 < km.shape[1]:
        pref |= km[:, w + 1] << np.uint64(64 - r)
    return pref & np.uint64((1 << (2 * p)) - 1)


def kff_container(k, sections) -> bytes:
    """the file CKFFWriter writes (kmc_core/kff_writer.cpp) around the given raw sections' record bytes; two counter bytes, canonical, cutoffs 1 .. 65535"""
    var = lambda pairs: b"v" + len(pairs).to_bytes(8, "big") + b"".join(n.encode() + b"\0" + v.to_bytes(8, "big") for n, v in pairs)  # noqa: E731
    rb = (k + 3) // 4 + 2
    out = [b"KFF\x01\x00\x1b\x01\x01" + bytes(4)]
    pos, index = 12, [12]
    out.append(var([("k", k), ("max", 1), ("data_size", 2), ("ordered", 1)]))
    pos += len(out[-1])
    for s in sections:
        index.append(pos)
        out += [b"r" + (len(s) // rb).to_bytes(8, "big"), s]
        pos += 9 + len(s)
    end = pos + 9 + 9 * (len(index) + 1) + 8
    out.append(b"i" + (len(index) + 1).to_bytes(8, "big") + b"".join((b"r" if i else b"v") + ((x - end) & ((1 << 64) - 1)).to_bytes(8, "big") for i, x in enumerate(index)) + b"v" + bytes(16))
    out.append(var([("first_index", pos), ("min_count", 1), ("max_count", 65535), ("counter_size", 2), ("footer_size", 1 + 8 + 20 + 18 + 18 + 21 + 20)]) + b"KFF")
    return b"".join(out)


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
    ap.add_argument("--n", type=int, default=8_000_000, help="records")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "db_kff_bench.json"))
    ap.add_argument("--k", type=int, nargs="+", default=[27, 55, 127], help="k-mer lengths (k % 4 == 3)")
    ap.add_argument("--only-repack", choices=("one_section", "512_sections"), help="nothing but the re-framing call on that shape (for a kernel trace that keeps the shapes apart); writes no file")
    ap.add_argument("--no-reference", action="store_true", help="do not time oracle/_ref/kmc_tools")
    ap.add_argument("--reference-timeout", type=float, default=120.0, help="seconds a kmc_tools run may take")
    a = ap.parse_args()
    import torch  # before libkmc_hip.so is loaded: the library then binds the HIP runtime torch brought, and the process holds one copy of it

    capi.require_gpu_backend()
    ctx = capi.Context((0,))
    ref = os.path.join(ROOT, "oracle", "_ref", "kmc_tools")
    res = dict(n_records=a.n, counter_bytes=2, n_sections=N_SECTIONS, per_kernel_split="kernel times come from a profiler run of its own: profiles/r11/db_kff_kernel_trace.json (tools/db_kff_trace.py)", k={})
    for k in a.k:
        rng = np.random.default_rng(k)
        km, be = random_kmers(rng, k, a.n)
        n = km.shape[0]
        counts = np.where(rng.random(n) < 0.7, 1, 1 + rng.geometric(0.02, size=n)).astype(np.uint16)
        kb = (k + 3) // 4
        kff = np.ascontiguousarray(np.concatenate([be[:, be.shape[1] - kb:], counts.astype(">u2").view(np.uint8).reshape(n, 2)], axis=1))
        sec = rng.integers(0, N_SECTIONS, size=n)
        order = np.argsort(sec, kind="stable")
        sec_n = np.bincount(sec, minlength=N_SECTIONS).tolist()
        kff512 = np.ascontiguousarray(kff[order])
        p0, p1 = dbio.best_lut_prefix_len(k, 0), dbio.best_lut_prefix_len(k, n)
        rb_in, rb0, rb1 = kb + 2, (k - p0) // 4 + 2, (k - p1) // 4 + 2
        d = dict(kff=ctx.malloc(kff.nbytes + 256), out=ctx.malloc(n * max(rb0, rb1) + 256), lut=ctx.malloc(8 * max((N_SECTIONS << (2 * p0)) + 1, 1 << (2 * p1))))
        row = dict(records=n, kff_record_bytes=rb_in, repack=dict(lut_prefix_len=p0, record_bytes=rb0), order=dict(lut_prefix_len=p1, record_bytes=rb1))
        moved = n * (rb_in + rb0)
        for name, data, secs in (("one_section", kff, [n]), ("512_sections", kff512, sec_n)):
            if a.only_repack not in (None, name):
                continue
            ctx.h2d(d["kff"], data.reshape(-1))
            t, got = timed(torch, lambda: ctx.kff_import_device(k, 2, d["kff"], secs, False, p0, d["out"], n * rb0, d["lut"]))
            assert got == n
            row["repack"][name] = dict(t, gb_per_s_read_plus_written=moved / t["ms_median_of_5"] / 1e6)
        if a.only_repack:
            for x in d.values():
                ctx.free(x)
            print(json.dumps({str(k): row}), flush=True)
            continue
        src, dst = torch.empty(n * rb0, dtype=torch.uint8, device="cuda"), torch.empty(n * rb0, dtype=torch.uint8, device="cuda")
        t, _ = timed(torch, lambda: dst.copy_(src))
        row["repack"]["memcpy_of_the_output"] = dict(t, gb_per_s_read_plus_written=2 * n * rb0 / t["ms_median_of_5"] / 1e6)
        del src, dst
        for name in ("one_section", "512_sections"):
            row["repack"][name]["over_memcpy"] = row["repack"][name]["gb_per_s_read_plus_written"] / row["repack"]["memcpy_of_the_output"]["gb_per_s_read_plus_written"]
        row["repack"]["512_over_one_section"] = row["repack"]["512_sections"]["gb_per_s_read_plus_written"] / row["repack"]["one_section"]["gb_per_s_read_plus_written"]
        # ordered = 1 on the 512 sections (they are in HBM from the loop above) ...
        t, got = timed(torch, lambda: ctx.kff_import_device(k, 2, d["kff"], sec_n, True, p1, d["out"], n * rb1, d["lut"]))
        imported = np.zeros(n * rb1, dtype=np.uint8)
        ctx.d2h(imported, d["out"])
        row["order"]["kff_import_512_sections"] = dict(t, g_records_per_s=n / t["ms_median_of_5"] / 1e6)
        # ... against the same k-mers as a KMC2 database of 512 bins through kmc_hip_order_database_device
        sb = (k - P_BINS) // 4
        bins = np.ascontiguousarray(np.concatenate([be[order, be.shape[1] - sb:], counts[order].astype("<u2").view(np.uint8).reshape(n, 2)], axis=1))
        starts = np.concatenate([[0], np.cumsum(sec_n)]).astype(np.int64)
        pref = prefix_of(km, k, P_BINS)[order].astype(np.int64)
        luts = np.stack([np.bincount(pref[starts[b]:starts[b + 1]], minlength=1 << (2 * P_BINS)) for b in range(N_SECTIONS)]).astype(np.uint64)
        small = np.zeros((N_SECTIONS, 8), dtype=np.uint64)
        small[:, 4] = np.array(sec_n, dtype=np.uint64) * np.uint64(sb + 2)
        e = dict(bins=ctx.malloc(bins.nbytes + 256), luts=ctx.malloc(luts.nbytes), small=ctx.malloc(small.nbytes))
        ctx.h2d(e["bins"], bins.reshape(-1))
        ctx.h2d(e["luts"], luts.reshape(-1))
        ctx.h2d(e["small"], small.reshape(-1))
        descs = (capi.BinDesc * N_SECTIONS)(*[capi.BinDesc(0, 0, 0, 0, 0, e["bins"] + int(starts[b]) * (sb + 2), sec_n[b] * (sb + 2), e["small"] + 64 * b + 32, e["luts"] + 8 * b * (1 << (2 * P_BINS)),
                                                           e["small"] + 64 * b) for b in range(N_SECTIONS)])
        p_in = capi.make_params(k, cutoff_min=1, cutoff_max=65535, counter_max=65535, lut_prefix_len=P_BINS)
        t, got = timed(torch, lambda: ctx.order_database_device(p_in, descs, p1, d["out"], n * rb1, d["lut"]))
        assert got == n
        ordered = np.zeros(n * rb1, dtype=np.uint8)
        ctx.d2h(ordered, d["out"])
        assert np.array_equal(ordered, imported), "the two paths disagree"
        row["order"]["order_database_512_bins"] = dict(t, g_records_per_s=n / t["ms_median_of_5"] / 1e6)
        row["order"]["import_over_order_database"] = row["order"]["kff_import_512_sections"]["ms_median_of_5"] / t["ms_median_of_5"]
        for x in list(d.values()) + list(e.values()):
            ctx.free(x)
        if os.path.exists(ref) and not a.no_reference:
            with tempfile.TemporaryDirectory() as td:
                flat = kff512.reshape(-1)
                with open(os.path.join(td, "in.kff"), "wb") as f:
                    f.write(kff_container(k, [flat[int(starts[b]) * rb_in:int(starts[b + 1]) * rb_in].tobytes() for b in range(N_SECTIONS)]))
                t0 = time.perf_counter()
                try:
                    subprocess.run([ref, "-t16", "-hp", "transform", os.path.join(td, "in.kff"), "sort", os.path.join(td, "o")], check=True, capture_output=True, timeout=a.reference_timeout)
                    row["reference_kmc_tools_t16_transform_sort_wall_s"] = time.perf_counter() - t0
                except (subprocess.TimeoutExpired, subprocess.CalledProcessError) as err:
                    row["reference_kmc_tools_t16_transform_sort_wall_s"] = f"NOT MEASURED: {type(err).__name__} after {time.perf_counter() - t0:.0f} s"
        else:
            row["reference_kmc_tools_t16_transform_sort_wall_s"] = "NOT MEASURED: no oracle/_ref/kmc_tools"
        res["k"][str(k)] = row
        print(json.dumps({str(k): row}), flush=True)
    ctx.close()
    if a.only_repack:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
