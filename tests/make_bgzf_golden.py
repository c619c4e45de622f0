"""Records the reference for tests/test_bgzf_emulated.py and tests/test_gpu_bgzf.py: for every case of bgzf_cases.BAM_CASES the BAM file (synth.write_bam) and what
`oracle/_ref/kmc <flags> -fbam <in> db tmp && oracle/_ref/kmc_tools transform db sort out` wrote — plain `kmc -k9 -fbam` for the small-k case, whose database is ordered
as it is —, into tests/golden/bgzf_*. Needs the reference binaries (oracle/_ref, built by build()); the tests need only the recorded files.
`python tests/make_bgzf_golden.py`."""
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

import bgzf_cases as B  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def main():
    kmc, kmc_tools = os.path.join(REF, "kmc"), os.path.join(REF, "kmc_tools")
    for exe in (kmc, kmc_tools):
        if not os.path.exists(exe):
            sys.exit(f"{exe} is missing: build() makes it where the reference tree is present")
    for name, (flags, (k, *_), _) in B.BAM_CASES.items():
        size = B.write_case_bam(name, B.bam_path(name))
        with tempfile.TemporaryDirectory() as td:
            os.mkdir(os.path.join(td, "tmp"))
            db = os.path.join(td, "db")
            subprocess.run([kmc, *flags, "-fbam", B.bam_path(name), db, os.path.join(td, "tmp")], check=True, capture_output=True, timeout=300)
            if k > 13:
                subprocess.run([kmc_tools, "transform", db, "sort", os.path.join(td, "out")], check=True, capture_output=True, timeout=300)
            for ext in (".kmc_pre", ".kmc_suf"):
                shutil.copyfile(os.path.join(td, ("out" if k > 13 else "db") + ext), B.bam_out(name) + ext)
        print(name, size, [os.path.getsize(B.bam_out(name) + e) for e in (".kmc_pre", ".kmc_suf")])


if __name__ == "__main__":
    main()
