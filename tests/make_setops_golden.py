"""Makes tests/golden/setops_*: two pairs (k = 27, k = 55) of small ordered KMC1 databases and, for every command line of setops_cases.LINES, the database
`kmc_tools simple` writes from them. Runs the reference's binaries from oracle/_ref and keeps only the data they write.

    python tests/make_setops_golden.py
"""
import os
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


def run(*cmd):
    subprocess.run(list(cmd), check=True, capture_output=True)


def main():
    os.makedirs(S.GOLDEN, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        for k in S.PAIRS:
            # low coverage of a 4 000-base genome, every read written 1..8 times: a few thousand k-mers with counts up to a few tens. b: half of a's reads
            # (written another number of times) plus reads of another genome — about half of the k-mers are shared, with different counts
            rng = np.random.default_rng(k)
            reads, others = synth.make_reads(100 + k, 4000, 50, 150, 0.004), synth.make_reads(200 + k, 4000, 25, 150, 0.004)
            rep = lambda r: np.repeat(r, rng.integers(1, 9, size=r.shape[0]), axis=0)  # noqa: E731
            for name, sub in (("a", rep(reads)), ("b", np.concatenate([rep(reads[25:]), rep(others)]))):
                fq = os.path.join(td, f"{name}{k}.fq")
                synth.write_fastq(fq, sub)
                tmp = os.path.join(td, f"t_{name}{k}")
                os.makedirs(tmp)
                run(os.path.join(REF, "kmc"), f"-k{k}", "-ci1", "-t2", fq, os.path.join(td, f"raw_{name}{k}"), tmp)
                run(os.path.join(REF, "kmc_tools"), "transform", os.path.join(td, f"raw_{name}{k}"), "sort", S.golden_path(k, name))
            a, b = (dbio.read_database(S.golden_path(k, n)) for n in "ab")
            da, db_ = (S.decode_body(k, d.lut_prefix_len, d.counter_size, d.lut, d.recs) for d in (a, b))
            shared = len(set(da[0]) & set(db_[0]))
            print(f"k={k}: a {a.total_kmers} k-mers (p {a.lut_prefix_len}, counter {a.counter_size} B), b {b.total_kmers}, shared {shared}")
            assert 0.3 < shared / a.total_kmers < 0.8
            hdr = [dict(counter_size=d.counter_size, min_count=d.min_count, max_count=d.max_count, total_kmers=d.total_kmers, kmer_len=k) for d in (a, b)]
            for line in S.LINES:
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
            sizes = [os.path.getsize(os.path.join(S.GOLDEN, f)) for f in os.listdir(S.GOLDEN) if f.startswith(f"setops_k{k}_")]
            print(f"k={k}: {len(sizes)} files, {sum(sizes)} bytes, largest {max(sizes)}")


if __name__ == "__main__":
    main()
