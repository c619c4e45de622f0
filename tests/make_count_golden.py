"""Records the reference for tests/test_count_emulated.py and tests/test_gpu_count.py: for every case of tests/count_cases.py the input files and what
`oracle/_ref/kmc <flags> <in> db tmp && oracle/_ref/kmc_tools transform db sort out` wrote, into tests/golden/count_*. Needs the reference binaries
(oracle/_ref, built by build()); the tests need only the recorded files. `python tests/make_count_golden.py`."""
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

import count_cases as CC  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def main():
    kmc, kmc_tools = os.path.join(REF, "kmc"), os.path.join(REF, "kmc_tools")
    for exe in (kmc, kmc_tools):
        if not os.path.exists(exe):
            sys.exit(f"{exe} is missing: build() makes it where the reference tree is present")
    for name, (flags, _, files) in CC.CASES.items():
        for fname, _, data in files:
            with open(os.path.join(CC.GOLDEN, fname), "wb") as f:
                f.write(gzip.compress(data, 6, mtime=0) if fname.endswith(".gz") else data)
        with tempfile.TemporaryDirectory() as td:
            os.mkdir(os.path.join(td, "tmp"))
            db = os.path.join(td, "db")
            subprocess.run([kmc, *flags, CC.input_argument(name, td), db, os.path.join(td, "tmp")], check=True, capture_output=True, timeout=300)
            subprocess.run([kmc_tools, "transform", db, "sort", os.path.join(td, "out")], check=True, capture_output=True, timeout=300)
            for ext in (".kmc_pre", ".kmc_suf"):
                shutil.copyfile(os.path.join(td, "out" + ext), CC.golden_out(name) + ext)
        print(name, [os.path.getsize(CC.golden_out(name) + e) for e in (".kmc_pre", ".kmc_suf")])


if __name__ == "__main__":
    main()
