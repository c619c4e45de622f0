"""Makes tests/golden/complex_*: for every definition of complex_cases.DEFS the database `kmc_tools -t1 -hp complex <file>` writes from databases that are already under
tests/golden (setops_*). The operations-definition files hold paths, so they are written from complex_cases into a temporary directory; only the .kmc_pre / .kmc_suf
pairs the reference writes are kept. Runs the reference's kmc_tools from oracle/_ref.

    python tests/make_complex_golden.py [k ...]
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import complex_cases as X  # noqa: E402
import setops_cases as S  # noqa: E402
from kmc_amd import dbio  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def main(ks):
    limit = max(os.path.getsize(os.path.join(S.GOLDEN, f)) for f in os.listdir(S.GOLDEN) if f.startswith("setops_"))
    with tempfile.TemporaryDirectory() as td:
        for k in ks:
            for line in X.DEFS[k]:
                out = X.golden_out(k, line[0])
                definition = os.path.join(td, f"{k}_{line[0]}.txt")
                with open(definition, "w") as f:
                    f.write(X.definition_text(line, out))
                subprocess.run([os.path.join(REF, "kmc_tools"), "-t1", "-hp", "complex", definition], check=True, capture_output=True)
                o = dbio.read_database(out)
                dbs = [dbio.read_database(X.fixture_path(fx)) for _, fx, _ in line[1]]
                r = X.resolve_line(line, [S.header_of(d) for d in dbs])
                tree = X.tree_of(line)
                lists = [X.ordered_lists(d) for d in dbs]
                _, wc, st = X.restate(tree, lists, r["cuts"], r["ci"], r["cx"], r["cs"])
                print(f"  k={k} {line[0]}: {o.total_kmers} k-mers, p {o.lut_prefix_len}, counter {o.counter_size} B, tallies {st}")
                assert o.total_kmers > 0, line
                assert all(os.path.getsize(out + e) <= limit for e in (".kmc_pre", ".kmc_suf")), "larger than the setops goldens"
                if line[0] == "inner_sum_beyond_cs":
                    inner = X.evaluate(tree[2], {i: X._leaf(*lists[i], *r["cuts"][i]) for i in range(len(lists))})
                    print(f"    inner sums beyond 255: {sum(c > 255 for _, c in inner)}")
                    assert sum(c > 255 for _, c in inner) > 10 and max(wc) <= 255 and o.counter_size == 1, "no inner sum beyond 255"
                if line[0] == "cutoffs":
                    assert st["n_below_min"] > 0 and st["n_above_max"] > 0 and wc.count(10) > 1 and max(wc) == 10, "nothing cut or clamped"
                if line[0] == "unused_wide_input":
                    assert o.counter_size == 2 and o.max_count == max(d.max_count for d in dbs), "the unused input does not show in the defaults"
                if line[0] in ("union_diff", "modes"):
                    assert st["n_result"] < st["n_keys"]
            sizes = [os.path.getsize(os.path.join(S.GOLDEN, f)) for f in os.listdir(S.GOLDEN) if f.startswith(f"complex_k{k}_")]
            print(f"k={k}: {len(sizes)} files, {sum(sizes)} bytes, largest {max(sizes)}")


if __name__ == "__main__":
    main([int(x) for x in sys.argv[1:]] or sorted(X.DEFS))
