"""Makes tests/golden/filter_*: two reads fixtures of about 200 records (FASTQ and the FASTA twin of each; the *_k pair has no read shorter than k = 33, for -t and
the fraction bounds, where kmc_tools' behaviour on shorter reads is undefined) and, for every command line of query_cases.LINES, the file `kmc_tools -t1 filter` writes.
The reads are stitched from walks over the k-mers of tests/golden/setops_k27_a and setops_k33_a (every window of a walk is in the database) and random bases, with 'N',
lower case, '\\r\\n' line ends, text behind the '+', reads of exactly 27 and 33 symbols and reads of several hundred. Runs the reference's binary from oracle/_ref and keeps
only the data it writes, gzipped (the quality lines are a pattern of the read's number and the position, not noise, so that they compress).

    python tests/make_filter_golden.py
"""
import gzip
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import query_cases as Q  # noqa: E402
import setops_cases as S  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def walks(k, rng):
    """-> function(length) -> bytes: a walk over the database's k-mers, every window of which is in the database (either strand)"""
    d = S.golden_db(k, "a")
    kmers = set(S.decode_body(k, d.lut_prefix_len, d.counter_size, d.lut, d.recs)[0])
    order = sorted(kmers)
    mask = (1 << (2 * k)) - 1

    def canon(x):
        return min(x, Q.kmer_int(Q.revcomp(Q.kmer_text(x, k))))

    def walk(length):
        for _ in range(5000):
            x = order[int(rng.integers(0, len(order)))]
            if rng.integers(0, 2):
                x = Q.kmer_int(Q.revcomp(Q.kmer_text(x, k)))
            text = bytearray(Q.kmer_text(x, k))
            while len(text) < length:
                nxt = [((x << 2) | int(b)) & mask for b in rng.permutation(4)]
                nxt = [y for y in nxt if canon(y) in kmers]
                if not nxt:
                    break
                x = nxt[0]
                text.append(b"ACGT"[x & 3])
            if len(text) >= length:
                return bytes(text)
        raise AssertionError("no walk of that length")

    return walk


def make_reads(rng, n, min_len):
    w27, w33 = walks(27, rng), walks(33, rng)
    rnd = lambda m: Q.BASES[rng.integers(0, 4, size=m)].tobytes()  # noqa: E731
    reads = []
    for i in range(n):
        kind = i % 10
        if kind == 0:
            s = rnd(int(rng.integers(max(min_len, 5), 60)))  # random: nothing found
        elif kind == 1:
            w = w27 if i % 20 == 1 else w33  # several hundred bases: three walks, everything found but the windows over the two joints
            s = b"".join(w(int(rng.integers(100, 180))) for _ in range(3))
        elif kind == 2:
            s = w27(27) if i % 20 == 2 else w33(33)  # exactly k
        elif kind in (3, 4):
            s = w27(int(rng.integers(30, 70))) + rnd(int(rng.integers(5, 30))) + w33(int(rng.integers(36, 70)))
        elif kind == 5:
            s = rnd(int(rng.integers(3, 30))) + w27(int(rng.integers(40, 90)))  # the first window is absent
        else:
            s = (w27 if rng.integers(0, 2) else w33)(int(rng.integers(max(min_len, 20), 100)))
        s = bytearray(s)
        if i % 7 == 3:
            s[int(rng.integers(0, len(s)))] = ord("N")
        if i % 11 == 5:
            a = int(rng.integers(0, len(s)))
            s[a:a + 30] = bytes(s[a:a + 30]).lower()
        if i % 13 == 6:  # a substitution in the middle of a walk: k windows drop out
            a = len(s) // 2
            s[a] = b"ACGT"[(b"ACGTacgtNn".index(s[a]) + 1) % 4]
        if len(s) < min_len:
            s += rnd(min_len - len(s))
        reads.append(bytes(s))
    return reads


def write_pair(reads, rng, fq, fa):
    with open(fq, "wb") as q, open(fa, "wb") as a:
        for i, s in enumerate(reads):
            eol = b"\r\n" if i % 40 == 9 else b"\n"
            qual = bytes(33 + (7 * i + j) % 41 for j in range(len(s)))
            plus = b"+" + (b"read%d again" % i if i % 3 == 0 else b"")
            q.write(b"@read%d len=%d" % (i, len(s)) + eol + s + eol + plus + eol + qual + eol)
            a.write(b">read%d len=%d" % (i, len(s)) + eol + s + eol)


def keep(path, data):
    with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0, filename="") as z:
        z.write(data)


def main():
    rng = np.random.default_rng(2027)
    with tempfile.TemporaryDirectory() as td:
        plain = lambda n: os.path.join(td, n)  # noqa: E731 — kmc_tools reads and writes plain files
        write_pair(make_reads(rng, 200, 0), rng, plain(Q.FQ[:-3]), plain(Q.FA[:-3]))
        write_pair(make_reads(rng, 200, 33), rng, plain(Q.FQ_LONG[:-3]), plain(Q.FA_LONG[:-3]))
        for n in (Q.FQ, Q.FA, Q.FQ_LONG, Q.FA_LONG):
            keep(os.path.join(Q.GOLDEN, n), open(plain(n[:-3]), "rb").read())
        for line in Q.LINES:
            subprocess.run([os.path.join(REF, "kmc_tools"), "-t1", "-hp", *Q.command_line(line, plain("out"), plain_dir=td)], check=True, capture_output=True)
            data = open(plain("out"), "rb").read()
            keep(os.path.join(Q.GOLDEN, "filter_out_" + line[0] + ".gz"), data)
            lead = b">" if ("-fa" in line[6] or "-fa" in line[7]) else b"@"
            n_out = sum(1 for ln in data.split(b"\n")[0::(2 if lead == b">" else 4)] if ln.startswith(lead))
            print(f"{line[0]}: {n_out} of 200 reads, {len(data)} bytes, {data.count(b'N')} N")
            assert 0 < n_out and (n_out < 200 or line[3] == ["-hm"]), line[0]
    sizes = [os.path.getsize(os.path.join(Q.GOLDEN, f)) for f in os.listdir(Q.GOLDEN) if f.startswith("filter_")]
    print(f"{len(sizes)} files, {sum(sizes)} bytes, largest {max(sizes)}")


if __name__ == "__main__":
    main()
