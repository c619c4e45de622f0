"""BGZF members inflated on the device (kmc_hip_bgzf_inflate_device / kmc_hip_bgzf_inflate, k_bgzf_inflate): a synthetic BAM stream and a synthetic FASTQ of about
--mb (256) MB inflated each, members of 0xFF00 bytes at level 6 — what samtools and bgzip write.
  device        HIP events around k_bgzf_inflate inside kmc_hip_bgzf_inflate_device: compressed bytes and output already in device memory, all members in one call
  host_to_host  wall clock around kmc_hip_bgzf_inflate: upload, the kernel, download — what `count` pays today
Medians of 5 after a warm-up with min .. max, GB/s of INFLATED output. Beside them, on the same machine in the same run:
  zlib_one_thread  zlib.decompressobj(-15) over the same members on one host thread with the CRC check: what the front end did before, and what the reference does
  device_copy      one plain device-to-device copy of the output bytes (GB/s of bytes written, as the other rates count output)
The output of the warm-up call is checked against zlib's before anything is timed. A figure that could not be taken is written as "NOT MEASURED" with the reason.

    python tools/bgzf_bench.py [--mb 256] [--out profiles/r16/bgzf_bench.json]
For the kernel alone run it under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/bgzf_bench.py`, a profiler run of its own."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kmc_amd import capi, synth  # noqa: E402

BLOCK = 0xFF00


def fastq_bytes(n_bytes: int) -> bytes:
    """the 4-line FASTQ of synth.write_fastq (150-base reads from a random genome, 1 % substitutions, constant quality)"""
    import tempfile

    n_reads = n_bytes // (12 + 150 + 3 + 150 + 1)
    with tempfile.NamedTemporaryFile() as f:
        synth.write_fastq(f.name, synth.make_reads(7, 50_000_000, n_reads))
        return f.read()


def bam_bytes(n_bytes: int) -> bytes:
    """an unaligned BAM stream: the header and records of 150 bases (name r<9 digits>, no CIGAR, qualities 0xFF), as synth.bam_record lays them out"""
    one = np.frombuffer(synth.bam_record("A" * 150, name=b"r000000000"), dtype=np.uint8)
    n = n_bytes // one.size
    recs = np.tile(one, (n, 1))
    ids = np.arange(n, dtype=np.int64)
    for d in range(9):
        recs[:, 36 + 9 - d] = (ids // 10**d) % 10 + ord("0")
    reads = synth.make_reads(8, 50_000_000, n)
    nib = np.array([1, 2, 4, 8], dtype=np.uint8)[reads]
    recs[:, 36 + 11:36 + 11 + 75] = (nib[:, 0::2] << 4) | nib[:, 1::2]
    assert recs[0, :4].view("<i4")[0] == one.size - 4
    head = b"BAM\1" + (25).to_bytes(4, "little") + b"@HD\tVN:1.6\tSO:unsorted\n\0\0" + (0).to_bytes(4, "little")
    return head + recs.tobytes()


def bgzf(data: bytes) -> bytes:
    """synth.bgzf_blocks over 16 threads (zlib releases the interpreter lock)"""
    step = BLOCK * 64
    with ThreadPoolExecutor(16) as ex:
        return b"".join(ex.map(lambda lo: synth.bgzf_blocks(data[lo:lo + step], BLOCK, 6), range(0, len(data), step))) + synth.BGZF_EOF


def summary(ms, out_bytes):
    med = statistics.median(ms)
    return dict(median_ms=round(med, 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), gb_per_s=round(out_bytes / med / 1e6, 2))


def bench_one(ctx, torch, name, data):
    L = ctx.L
    blob = np.frombuffer(bgzf(data), dtype=np.uint8)
    members, used, total = capi.bgzf_scan(blob)
    assert used == blob.size and total == len(data)
    res = dict(inflated_bytes=total, compressed_bytes=int(blob.size), members=int(members.size))
    # one host thread, as the front end did it
    t0 = time.perf_counter()
    for m in members:
        d = zlib.decompressobj(-15)
        out = d.decompress(blob[int(m["src_off"]):int(m["src_off"]) + int(m["comp_len"])])
        assert zlib.crc32(out) == int(m["crc"])
    res["zlib_one_thread"] = summary([(time.perf_counter() - t0) * 1e3], total)
    d_src, d_dst = ctx.malloc(blob.size + 16), ctx.malloc(total + 16)
    try:
        ctx.h2d(d_src, blob)
        capi.bgzf_inflate_device(ctx, d_src, blob.size, members, d_dst, total)  # warm-up, checked
        got = np.zeros(total, dtype=np.uint8)
        ctx.d2h(got, d_dst)
        assert got.tobytes() == data, "the device's bytes are not zlib's"
        res["device"] = summary([capi.bgzf_inflate_device(ctx, d_src, blob.size, members, d_dst, total) for _ in range(5)], total)
        out, bad = np.zeros(total, dtype=np.uint8), C.c_uint32(0)
        wall = []
        for it in range(6):
            t0 = time.perf_counter()
            rc = L.kmc_hip_bgzf_inflate(ctx.h, 0, 0, blob.ctypes.data_as(C.c_void_p), blob.size, members.ctypes.data_as(C.c_void_p), members.size, out.ctypes.data_as(C.c_void_p), total,
                                        C.byref(bad), None)
            assert rc == 0
            if it:
                wall.append((time.perf_counter() - t0) * 1e3)
        assert out.tobytes() == data
        res["host_to_host"] = summary(wall, total)
        try:
            if torch is None:
                raise RuntimeError("torch could not be imported")
            a, b = torch.empty(total, dtype=torch.uint8, device="cuda"), torch.empty(total, dtype=torch.uint8, device="cuda")
            a.random_(0, 256)
            ms = []
            for it in range(6):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                b.copy_(a)
                e1.record()
                e1.synchronize()
                if it:
                    ms.append(e0.elapsed_time(e1))
            res["device_copy"] = summary(ms, total)
        except Exception as e:  # noqa: BLE001
            res["device_copy"] = f"NOT MEASURED ({type(e).__name__}: {e})"
    finally:
        ctx.free(d_src)
        ctx.free(d_dst)
    if isinstance(res["device_copy"], dict):
        res["device_over_zlib"] = round(res["device"]["gb_per_s"] / res["zlib_one_thread"]["gb_per_s"], 1)
        res["host_to_host_over_zlib"] = round(res["host_to_host"]["gb_per_s"] / res["zlib_one_thread"]["gb_per_s"], 1)
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "bgzf_bench.json"))
    a = ap.parse_args()
    try:
        import torch  # before libkmc_hip.so is loaded: the library then binds the HIP runtime torch brought, and the process holds one copy of it
    except ImportError:
        torch = None
    capi.require_gpu_backend()
    ctx = capi.Context((0,))
    try:
        res = dict(window="the member's whole output in LDS (64 KiB + 16): one 64-thread workgroup per member, two workgroups a CU", member_bytes=BLOCK, level=6,
                   ring_32k="NOT MEASURED (the 32 KiB ring was not built)", kernel_trace="NOT MEASURED (no profiler run was taken)")
        res["fastq"] = bench_one(ctx, torch, "fastq", fastq_bytes(a.mb << 20))
        res["bam"] = bench_one(ctx, torch, "bam", bam_bytes(a.mb << 20))
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
