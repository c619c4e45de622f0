"""Writes tests/golden/smallk_input.fa and tests/golden/smallk_counts.json: the k-mer / count pairs kmc_dump gives for the reference's own `kmc -k5` and
`kmc -k9 -b` databases of the tiny input (both runs print "Small k optimization on!"). tests/test_stage1_smallk_emulated.py holds its numpy restatement
of CSplitter::ProcessReadsSmallK to them. Needs oracle/_ref/kmc and oracle/_ref/kmc_dump (built where the reference's source tree is present).

    python tests/make_smallk_golden.py"""
import json
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden")
RUNS = {"k5": ["-k5"], "k9b": ["-k9", "-b"]}


def tiny_input():
    """reads of 1 .. 120 symbols with N and lower case, reads of k - 1 and k symbols for both runs, a homopolymer, a palindrome, \\r\\n on some records"""
    rng = np.random.default_rng(20261018)
    letters = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)
    reads = [b"ACGT", b"ACGTA", b"ACGTACGT", b"ACGTACGTA", b"A" * 40, b"ACGTTGCATGCAACGT", b"NACGTACGTACGTN", b"ACGTANACGTACGTAC", b"N" * 12, b""]
    for _ in range(60):
        p = np.array([5, 5, 5, 5, 1, 1, 1, 1, 1], dtype=float)
        reads.append(letters[rng.choice(letters.size, size=int(rng.integers(1, 121)), p=p / p.sum())].tobytes())
    return b"".join(b">r%d\n" % i + r + (b"\r\n" if i % 7 == 3 else b"\n") for i, r in enumerate(reads) if r)


def main():
    text = tiny_input()
    with open(os.path.join(GOLDEN, "smallk_input.fa"), "wb") as f:
        f.write(text)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        inp = os.path.join(tmp, "in.fa")
        with open(inp, "wb") as f:
            f.write(text)
        for name, flags in RUNS.items():
            db, dump = os.path.join(tmp, name), os.path.join(tmp, name + ".txt")
            r = subprocess.run([os.path.join(REF, "kmc"), *flags, "-fa", "-ci1", "-cs1000000", "-v", "-m2", "-sf1", "-sp1", "-sr1", inp, db, tmp], capture_output=True, text=True, check=True)
            assert "Small k optimization on!" in r.stdout + r.stderr
            subprocess.run([os.path.join(REF, "kmc_dump"), "-ci1", "-cx1000000", db, dump], check=True, capture_output=True)
            with open(dump) as f:
                out[name] = [[a, int(b)] for a, b in (ln.split() for ln in f if ln.strip())]
    with open(os.path.join(GOLDEN, "smallk_counts.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print({k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
