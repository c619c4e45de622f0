"""Makes tests/golden/setops_*: three pairs (k = 27, k = 55, k = 33) of small ordered KMC1 databases and, for every command line of setops_cases.LINES_OF[k], the
database `kmc_tools simple` writes from them. The k = 33 pair is large enough for kmc_tools to choose lut_prefix_len 5 (the prefix across a 64-bit word boundary of
the k-mer); the KMC2 database `kmc` wrote for its input a is kept as well (setops_k33_raw_a). Runs the reference's binaries from oracle/_ref and keeps only the data
they write.

    python tests/make_setops_golden.py [k ...]
"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import setops_cases as S  # noqa: E402
from kmc_amd import dbio, synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
# per k: (genome length, reads of a, reads of the other genome in b, further options of kmc). k = 33: 64 bins and signatures of 5 symbols keep the KMC2 .kmc_pre
# (a LUT of 4^p entries per bin, the signature map) small enough to commit
SHAPES = {27: (4000, 50, 25, []), 55: (4000, 50, 25, []), 33: (9500, 118, 45, ["-n64", "-p5"])}


def run(*cmd):
    subprocess.run(list(cmd), check=True, capture_output=True)


def main(ks):
    os.makedirs(S.GOLDEN, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        for k in ks:
            # low coverage of a genome of a few thousand bases, every read written 1..8 times: a few thousand k-mers with counts up to a few tens. b: half of a's reads
            # (written another number of times) plus reads of another genome — about half of the k-mers are shared, with different counts
            rng = np.random.default_rng(k)
            glen, n_reads, n_others, kmc_opts = SHAPES[k]
            reads, others = synth.make_reads(100 + k, glen, n_reads, 150, 0.004), synth.make_reads(200 + k, glen, n_others, 150, 0.004)
            rep = lambda r: np.repeat(r, rng.integers(1, 9, size=r.shape[0]), axis=0)  # noqa: E731
            for name, sub in (("a", rep(reads)), ("b", np.concatenate([rep(reads[n_reads // 2:]), rep(others)]))):
                fq = os.path.join(td, f"{name}{k}.fq")
                synth.write_fastq(fq, sub)
                tmp = os.path.join(td, f"t_{name}{k}")
                os.makedirs(tmp)
                run(os.path.join(REF, "kmc"), f"-k{k}", "-ci1", "-t2", *kmc_opts, fq, os.path.join(td, f"raw_{name}{k}"), tmp)
                run(os.path.join(REF, "kmc_tools"), "transform", os.path.join(td, f"raw_{name}{k}"), "sort", S.golden_path(k, name))
                if name == "a" and k in S.RAW_A:
                    for ext in (".kmc_pre", ".kmc_suf"):
                        shutil.copyfile(os.path.join(td, f"raw_{name}{k}") + ext, S.golden_path(k, S.RAW_A[k]) + ext)
            a, b = (dbio.read_database(S.golden_path(k, n)) for n in "ab")
            if k == 33:
                raw = dbio.read_database(S.golden_path(k, S.RAW_A[k]))
                assert raw.kmc2 and raw.total_kmers == a.total_kmers and S.straddles(k, raw.lut_prefix_len), "the raw database's prefix does not lie across the word boundary"
                assert a.lut_prefix_len == b.lut_prefix_len == 5 and S.straddles(k, 5), "kmc_tools did not choose lut_prefix_len 5"
            da, db_ = (S.decode_body(k, d.lut_prefix_len, d.counter_size, d.lut, d.recs) for d in (a, b))
            shared = len(set(da[0]) & set(db_[0]))
            print(f"k={k}: a {a.total_kmers} k-mers (p {a.lut_prefix_len}, counter {a.counter_size} B), b {b.total_kmers}, shared {shared}")
            assert 0.3 < shared / a.total_kmers < 0.8
            hdr = [dict(counter_size=d.counter_size, min_count=d.min_count, max_count=d.max_count, total_kmers=d.total_kmers, kmer_len=k) for d in (a, b)]
            for line in S.LINES_OF[k]:
                out = S.golden_path(k, line[0])
                run(os.path.join(REF, "kmc_tools"), *S.command_line(line, S.golden_path(k, "a"), S.golden_path(k, "b"), out))
                o = dbio.read_database(out)
                r = S.resolve_line(line, *hdr)
                _, wc, st = S.restate(da, db_, r["a_cut"], r["b_cut"], r["op"], r["oc"], r["ci"], r["cx"], r["cs"])
                print(f"  {line[0]}: {o.total_kmers} k-mers, counter {o.counter_size} B, tallies {st}")
                assert o.total_kmers > 0, line
                if line[0] in ("counters_subtract", "counters_subtract_ocdiff", "reverse_counters_subtract"):
                    assert st["n_below_min"] > 0, "no difference of 0"
                if line[0] == "union_ci3_cx20_cs10":
                    assert st["n_below_min"] > 0 and st["n_above_max"] > 0 and wc.count(10) > 1 and max(wc) == 10, "nothing cut or clamped"
                if line[0] == "union_a_ci2_b_cx5":
                    assert sum(c < 2 for c in da[1]) > 0 and sum(c > 5 for c in db_[1]) > 0, "the input cutoffs cut nothing"
                if line[0] == "intersect_ocsum_cs65535":
                    assert o.counter_size == 2
                if k == 33:
                    assert o.lut_prefix_len == 5
            sizes = [os.path.getsize(os.path.join(S.GOLDEN, f)) for f in os.listdir(S.GOLDEN) if f.startswith(f"setops_k{k}_")]
            print(f"k={k}: {len(sizes)} files, {sum(sizes)} bytes, largest {max(sizes)}")


if __name__ == "__main__":
    main([int(x) for x in sys.argv[1:]] or S.PAIRS)
