"""Makes tests/golden/toolsline_*.json: what the reference's `kmc_tools -t1 -hp` prints for every command line of compare_cases.LINES (`compare`, `check`, `info`) over
fixtures that are committed already — stdout, stderr and the exit status, one small file per line. -hp hides the progress bar, which `compare` would otherwise write
into stdout. Runs oracle/_ref/kmc_tools (made by build() where the reference tree is present) with tests/golden as the working directory, so that no path of the
machine gets into a message; keeps nothing else.

    python tests/make_compare_golden.py
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import compare_cases as CC  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def main():
    for f in os.listdir(CC.GOLDEN):
        if f.startswith("toolsline_"):
            os.remove(os.path.join(CC.GOLDEN, f))
    seen = {}
    for line in CC.LINES:
        argv = [a.format(g=".") for a in line[1]]
        r = subprocess.run([os.path.join(REF, "kmc_tools"), "-t1", "-hp", *argv], cwd=CC.GOLDEN, capture_output=True, text=True, timeout=600)
        assert CC.GOLDEN not in r.stdout + r.stderr and ROOT not in r.stdout + r.stderr, line[0]
        rec = dict(stdout=r.stdout, stderr=r.stderr, status=r.returncode)
        with open(CC.golden_file(line), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        seen[line[0]] = rec
        print(f"{line[0]}: status {r.returncode}, stdout {r.stdout[:60]!r}{'...' if len(r.stdout) > 60 else ''}, stderr {r.stderr[:60]!r}")
    # what the lines are for
    assert seen["cmp_k33_kmc1_kmc2"]["stdout"] == "DB Equals\n" and seen["cmp_k33_kmc1_kmc2"]["status"] == 0
    assert seen["cmp_k27_a_b"]["stdout"] == "DB Differs\n" and seen["cmp_k27_a_b"]["status"] == 1
    for name in ("cmp_k27_kff", "cmp_k33_kff", "cmp_k55_kff", "cmp_k33_kmc2_kff", "cmp_k27_kff_cs2", "cmp_k27_multi_self", "cmp_k27_self_ci2_both", "cmp_k27_both_empty"):
        assert seen[name]["stdout"] == "DB Equals\n", name
    for name in ("cmp_k27_a_ends_first", "cmp_k27_b_ends_first"):
        assert seen[name]["stdout"] == "one of input is not finished\nDB Differs\n" and seen[name]["status"] == 1, name
    assert seen["chk_k27_at_cx"]["stdout"] == "0\n" and seen["chk_k27_below_cx"]["stdout"] == "5\n", "the cutoff_max rule of check"
    assert seen["chk_k27_present"]["stdout"] == "4\n" and seen["chk_k27_lower_case"]["stdout"] == "4\n" and seen["chk_k27_rc_only"]["stdout"] == "0\n"
    assert seen["chk_k27_kff_absent"]["stdout"] == "" and seen["chk_k27_kff_absent"]["status"] == 0, "a KFF file that does not hold the k-mer prints nothing"
    assert seen["chk_k27_too_short"] == dict(stdout="", stderr="Error: invalid k-mer length\n", status=1)
    assert seen["chk_k27_with_n"] == dict(stdout="", stderr="Error: invalid k-mer format\n", status=1)
    assert seen["info_k27_kff_multi"]["stdout"].count("nb_blocks") == 58 + 1 and "footer values:" in seen["info_k27_kff_multi"]["stderr"]
    sizes = [os.path.getsize(os.path.join(CC.GOLDEN, f)) for f in os.listdir(CC.GOLDEN) if f.startswith("toolsline_")]
    print(f"{len(sizes)} files, {sum(sizes)} bytes, largest {max(sizes)}")
    assert sum(sizes) < 100_000


if __name__ == "__main__":
    main()
