"""Records the reference for tests/test_smallk_db_emulated.py and tests/test_gpu_smallk_db.py: for every case of tests/smallk_db_cases.py the input files, what
`oracle/_ref/kmc -v -m2 -sf1 -sp2 -sr2 <flags> <in> db tmp` wrote — the log must say "Small k optimization on!" — and the statistics lines it printed, into
tests/golden/smallkdb_*. A KFF case is `kmc -okff` followed by `kmc_tools -t1 -hp transform db.kff reduce out -okff`, what `count` promises for KFF. Needs the reference
binaries (oracle/_ref, built by build()); the tests need only the recorded files. `python tests/make_smallk_db_golden.py`."""
import gzip
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import smallk_db_cases as K  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def main():
    kmc, kmc_tools = os.path.join(REF, "kmc"), os.path.join(REF, "kmc_tools")
    for exe in (kmc, kmc_tools):
        if not os.path.exists(exe):
            sys.exit(f"{exe} is missing: build() makes it where the reference tree is present")
    for name, (flags, files, fmt) in K.CASES.items():
        for fname, _, data in files:
            with open(os.path.join(K.GOLDEN, fname), "wb") as f:
                f.write(gzip.compress(data, 6, mtime=0) if fname.endswith(".gz") else data)
        with tempfile.TemporaryDirectory() as td:
            os.mkdir(os.path.join(td, "tmp"))
            db = os.path.join(td, "db")
            r = subprocess.run([kmc, *K.REF_FLAGS, *flags, *(["-okff"] if fmt == "kff" else []), K.input_argument(name, td), db, os.path.join(td, "tmp")], capture_output=True,
                               text=True, timeout=300)
            assert r.returncode == 0, (name, r.stdout[-800:], r.stderr[-800:])
            assert "Small k optimization on!" in r.stdout + r.stderr, (name, (r.stdout + r.stderr)[-800:])
            lines = K.report_lines(r.stdout)
            assert len(lines) == 7, (name, lines)
            with open(K.golden_report(name), "w") as f:
                f.write("".join("%s: %d\n" % ln for ln in lines))
            if fmt == "kff":
                r = subprocess.run([kmc_tools, "-t1", "-hp", "transform", db + ".kff", "reduce", os.path.join(td, "out"), "-okff"], capture_output=True, text=True, timeout=300)
                assert r.returncode == 0, (name, r.stdout[-800:], r.stderr[-800:])
                shutil.copyfile(os.path.join(td, "out.kff"), K.golden_out(name) + ".kff")
                sizes = [os.path.getsize(K.golden_out(name) + ".kff")]
            else:
                for ext in (".kmc_pre", ".kmc_suf"):
                    shutil.copyfile(db + ext, K.golden_out(name) + ext)
                sizes = [os.path.getsize(K.golden_out(name) + e) for e in (".kmc_pre", ".kmc_suf")]
        print(name, sizes, lines[:5])


if __name__ == "__main__":
    main()
