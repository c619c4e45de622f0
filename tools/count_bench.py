"""The counting session (kmc_hip_count_*: reads -> one ordered database body, the bin records never leave the device) measured on a synthetic FASTQ from the read model
of kmc_amd/synth.py (libkmc_synth writes the same reads), read into host memory and cut into parts of whole records first. Inside one run (after one whole warm-up run):
  parts    the sum of the kmc_hip_count_part calls (wall clock around the synchronous calls: upload, stage-1 chain, device-to-device copy into the store)
  gather   k_cnt_gather alone (HIP events around the launch, kmc_hip_count_timings)
  stage2   kmc_hip_process_bins_device over the gathered bins with the copies into the tight store (wall clock inside kmc_hip_count_finish)
  order    kmc_hip_count_order (wall clock)
and, as the yardstick of the gather, ONE device-to-device hipMemcpyAsync (torch's copy_ of a contiguous uint8 tensor) of the number of bytes the gather moved.
Every figure is the median of --runs sessions after one warm-up session, with the smallest and the largest beside it. The session's figures are calls on text
already in host memory: they hold neither the file reading nor the database writing. The whole processes the session stands against (kmc_amd/bin/kmc_hip_s1 or
oracle/_ref/kmc, followed by kmc_tools transform sort) are not timed here.
The body is checked as far as it can be without a second counter (check_body): every session gives the same bytes; the records ascend strictly under their LUT;
the k-mers that entered stage 2 are the windows of the reads (the model plants no invalid symbol); records = unique - below - above; every counter lies in [2, 255].
That it is the reference's database is what tests/test_gpu_count.py holds, on a file a numpy oracle can count.

    python tools/count_bench.py [--reads 2000000] [--genome 20000000] [--k 27] [--runs 5] [--out profiles/r10/count_bench.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kmc_amd import capi, dbio, readsio, tools  # noqa: E402


def cut_parts(text: np.ndarray, part_bytes: int) -> list:
    """views of `text`: whole FASTQ records, about part_bytes each"""
    parts, at = [], 0
    while at < text.size:
        end = min(at + part_bytes, text.size)
        n = readsio.whole_records(text[at:end], True) if end < text.size else text.size - at
        assert n > 0, "a record longer than a part"
        parts.append(text[at:at + n])
        at += n
    return parts


def run_session(ctx, parts, k, n_bins=512, m=9):
    ses = capi.CountSession(ctx, k, m, n_bins, True, tools.count_signature_map(m, n_bins))
    try:
        p = ses.split_params(file_type=1)
        t0 = time.perf_counter()
        for i, part in enumerate(parts):
            ses.part(part, p)
            if i == 0:
                say("first part:", time.perf_counter() - t0, "s")
        t_parts = time.perf_counter() - t0
        say("parts:", t_parts, "s")
        bp = capi.make_params(k, lut_prefix_len=next(q for q in range(1, 5) if (k - q) % 4 == 0))
        t0 = time.perf_counter()
        st, tot, n_records = ses.finish(bp)
        t_finish = time.perf_counter() - t0
        say("finish:", t_finish, "s", ses.timings())
        p_out = dbio.best_lut_prefix_len(k, n_records)
        view = ses.order(p_out)
        lib = ses.timings()
        info = ses.info()
        rb = (k - p_out) // 4 + view.counter_size
        recs, lut = np.zeros(n_records * rb, dtype=np.uint8), np.zeros(1 << (2 * p_out), dtype=np.uint64)
        t0 = time.perf_counter()
        ctx.d2h(recs, view.d_recs)
        ctx.d2h(lut, view.d_lut)
        t_down = time.perf_counter() - t0
        res = dict(parts_s=t_parts, finish_s=t_finish, layout_s=lib["layout"], gather_s=lib["gather"], stage2_s=lib["stage2"], order_s=lib["order"], copy_down_s=t_down,
                   n_parts=len(parts), n_segments=info["n_segments"], n_batches=info["n_batches"], n_records=int(n_records), n_kmers=int(tot[2]), bin_bytes=int(tot[3]),
                   largest_over_mean_bin=info["largest_bin"] * n_bins / max(int(tot[2]), 1), stats=[int(x) for x in st])
        return res, (view.counter_size, p_out, lut, recs)
    finally:
        ses.close()


def plain_copy_seconds(nbytes: int) -> float:
    """one device-to-device copy of nbytes (the median of 5 after a warm-up), by HIP events"""
    import torch

    a = torch.randint(0, 255, (max(nbytes, 1),), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    ts = []
    for it in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if it:
            ts.append(e0.elapsed_time(e1) / 1e3)
    return sorted(ts)[len(ts) // 2]


def check_body(k, cs, p_out, lut, recs, res, reads, read_len=150, ci=2, counter_max=255):
    """what can be said about the body without counting again; raises AssertionError"""
    sb = (k - p_out) // 4
    r = recs.reshape(-1, sb + cs)
    n = r.shape[0]
    assert n == res["n_records"] == res["stats"][0] - res["stats"][1] - res["stats"][2], "records != unique - below - above"
    assert res["n_kmers"] == res["stats"][3] == reads * (read_len - k + 1), "k-mers entering stage 2 != windows of the reads"
    assert lut[0] == 0 and np.all(np.diff(lut.astype(np.int64)) >= 0) and int(lut[-1]) <= n, "LUT does not ascend"
    prefix = np.repeat(np.arange(lut.size, dtype=np.uint32), np.diff(np.concatenate([lut, [n]]).astype(np.int64)))
    key = np.concatenate([prefix.astype(">u4").view(np.uint8).reshape(n, 4), r[:, :sb]], axis=1)
    differ = key[1:] != key[:-1]
    first = np.argmax(differ, axis=1)
    rows = np.arange(n - 1)
    assert bool(np.all(differ.any(axis=1))) and bool(np.all(key[1:][rows, first] > key[:-1][rows, first])), "records do not ascend strictly"
    cnt = np.zeros(n, dtype=np.uint32)
    for j in range(cs):
        cnt |= r[:, sb + j].astype(np.uint32) << (8 * j)
    assert int(cnt.min()) >= ci and int(cnt.max()) <= counter_max, "a counter outside [ci, cs]"


def say(*what):
    print("[count_bench]", *what, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--genome", type=int, default=20_000_000)
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--part-mb", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "count_bench.json"))
    a = ap.parse_args()
    import torch  # noqa: F401 — before libkmc_hip.so is loaded: the library then binds the HIP runtime torch brought, and the process holds one copy of it
    capi.require_gpu_backend()
    with tempfile.TemporaryDirectory() as td:
        fq = os.path.join(td, "reads.fq")
        size = capi.synth_fastq(fq, seed=7, genome_len=a.genome, n_reads=a.reads)
        text = np.fromfile(fq, dtype=np.uint8)
        parts = cut_parts(text, a.part_mb << 20)
        say("input:", size, "bytes,", len(parts), "parts")
        ctx = capi.Context((0,))
        try:
            cold, _ = run_session(ctx, parts, a.k)
            say("warm-up run:", json.dumps(cold))
            runs, body = [], None
            for i in range(a.runs):
                res, (cs, p_out, lut, recs) = run_session(ctx, parts, a.k)
                say("run", i, json.dumps(res))
                runs.append(res)
                if body is None:
                    body = (cs, p_out, lut, recs)
                else:
                    assert (cs, p_out) == body[:2] and np.array_equal(lut, body[2]) and np.array_equal(recs, body[3]), "two sessions gave different bodies"
        finally:
            ctx.close()
        cs, p_out, lut, recs = body
        check_body(a.k, cs, p_out, lut, recs, runs[0], a.reads)
        say("body checked:", runs[0]["n_records"], "records")
        timed = ("parts_s", "finish_s", "layout_s", "gather_s", "stage2_s", "order_s", "copy_down_s")
        warm = dict(runs[0], **{key: sorted(r[key] for r in runs)[len(runs) // 2] for key in timed})
        spread = {key: [min(r[key] for r in runs), max(r[key] for r in runs)] for key in timed}
        t0 = time.perf_counter()
        dbio.write_kmc1(os.path.join(td, "ours"), a.k, cs, p_out, 2, 10**9, True, lut, recs)
        write_s = time.perf_counter() - t0
        copy_s = plain_copy_seconds(warm["bin_bytes"])
        say("plain copy of", warm["bin_bytes"], "bytes:", copy_s, "s")
        seg = warm["bin_bytes"] / max(warm["n_segments"], 1)
        out = dict(input=dict(fastq_bytes=int(size), reads=a.reads, genome=a.genome, k=a.k, part_mb=a.part_mb, n_bins=512), runs=a.runs, session=warm, session_min_max=spread, session_first_run=cold, body_checked=True,
                   gather=dict(bytes=warm["bin_bytes"], mean_segment_bytes=seg, gb_per_s=2 * warm["bin_bytes"] / max(warm["gather_s"], 1e-9) / 1e9, plain_copy_s=copy_s,
                               plain_copy_gb_per_s=2 * warm["bin_bytes"] / max(copy_s, 1e-9) / 1e9, gather_over_plain_copy=copy_s / max(warm["gather_s"], 1e-9)),
                   session_gkmers_per_s=warm["n_kmers"] / (warm["parts_s"] + warm["finish_s"] + warm["order_s"]) / 1e9,
                   database_write_s=write_s, note="medians of `runs` sessions after one warm-up session; gb_per_s counts bytes read + bytes written; the session's figures are calls on text already in host memory")
    write(out, a.out)
    print(json.dumps(out))


def write(out, path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
