"""Timing of kmc_hip_split_part (include/kmc_hip.h) on 32 MB multi-line FASTA parts (file_type 2: k_s1_ml_text_to_codes) next to single-line FASTA
parts of the same size and the same sequences (file_type 0: k_s1_text_to_codes). A multi-line part is what CFastqReader::GetPartFromMultilneFasta hands
the splitter: titles with their end of line, sequence text without line ends. Wall-clock of the synchronous C-ABI call (H2D of the text, the kernel
chain of kmc_amd/csrc/stage1_chain.h, D2H of the records), best of --reps; one JSON line per mode. For the kernels alone run it under
`rocprofv3 --kernel-trace --stats -- python tools/s1_ml_part_bench.py`. numpy + the C-ABI only."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmc_amd import capi  # noqa: E402


class SplitParams(C.Structure):
    _fields_ = [("kmer_len", C.c_uint32), ("signature_len", C.c_uint32), ("n_bins", C.c_uint32), ("max_x", C.c_uint32), ("both_strands", C.c_uint32),
                ("file_type", C.c_uint32), ("line_cap", C.c_uint64), ("part_kind", C.c_uint32), ("reserved", C.c_uint32)]


def make_parts(mbytes, contig_len, seed):
    """(multi-line part, single-line part) of the same contigs, each about `mbytes` MB"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGTacgtACGTACGT", dtype=np.uint8)
    ml, sl, size = [], [], 0
    i = 0
    while size < (mbytes << 20):
        seq = acgt[rng.integers(0, acgt.size, size=contig_len)].tobytes()
        title = b">contig_%d synthetic" % i
        ml.append(title + b"\n" + seq)
        sl.append(title + b"\n" + seq + b"\n")
        size += len(sl[-1])
        i += 1
    return np.frombuffer(b"".join(ml), dtype=np.uint8), np.frombuffer(b"".join(sl), dtype=np.uint8), i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mbytes", type=int, default=32, help="size of a part (the reference's reader cuts parts of up to 32 MB)")
    ap.add_argument("--contig", type=int, default=100_000, help="symbols per record")
    ap.add_argument("--k", type=int, default=27)
    ap.add_argument("--m", type=int, default=9)
    ap.add_argument("--bins", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ml, sl, n_rec = make_parts(a.mbytes, a.contig, 1)
    smap = np.random.default_rng(2).integers(0, a.bins, size=(1 << (2 * a.m)) + 1).astype(np.int32)
    ctx = capi.Context((0,))
    L, h = ctx.L, ctx.h
    L.kmc_hip_split_set_map.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
    L.kmc_hip_split_part.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7
    ctx._chk(L.kmc_hip_split_set_map(h, 0, smap.ctypes.data, a.m))
    arr = np.zeros((5, a.bins), dtype=np.uint64)
    need, n_reads = C.c_uint64(0), C.c_uint64(0)
    for name, text, ft in (("multi-line FASTA", ml, 2), ("single-line FASTA", sl, 0)):
        p = SplitParams(a.k, a.m, a.bins, 3, 1, ft, 524296, 0, 0)  # line_cap: KMC's mem_part_pmm_reads
        recs = np.zeros(2 * text.size + 256 * (a.bins + 1), dtype=np.uint8)
        best = None
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            rc = L.kmc_hip_split_part(h, 0, 0, C.byref(p), text.ctypes.data, text.size, recs.ctypes.data, recs.size, C.byref(need), *[x.ctypes.data for x in arr],
                                      C.byref(n_reads))
            dt = time.perf_counter() - t0
            ctx._chk(rc)
            if rep and (best is None or dt < best):
                best = dt
        print(json.dumps(dict(what="kmc_hip_split_part: one %s part, host text -> host records (best of %d)" % (name, a.reps), file_type=ft, text_bytes=int(text.size),
                              records=n_rec, reads=int(n_reads.value), k=a.k, bins=a.bins, kmers=int(arr[2].sum()), superkmers=int(arr[3].sum()), seconds=best,
                              text_GBs=text.size / best / 1e9)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
