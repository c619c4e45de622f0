"""Makes tests/golden/kffout_*.kff: what the reference's `kmc_tools -t1 -hp transform <db> [-ci -cx] reduce <out> [-ci -cx -cs] -okff` writes for every line of
kffout_cases.FILES — output bounds, input bounds, counters wider than the input's, a KMC2 input, a KFF input of 58 sections, and an output without records. Runs
kmc_tools from oracle/_ref and keeps only the data files it wrote. Every file is held to the restatement of container and record (kff_cases) before it is kept, and the
"58 sections to one" file to a second reference run: `kmc -okff` of the committed count input followed by the same reduce.

Every line of kffout_cases.FILES ran in the reference; none had to be left out.

    python tests/make_kffout_golden.py
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import kff_cases as K  # noqa: E402
import kffout_cases as X  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def main():
    for f in os.listdir(X.GOLDEN):
        if f.startswith("kffout_"):
            os.remove(os.path.join(X.GOLDEN, f))
    with tempfile.TemporaryDirectory() as td:
        for name in X.FILES:
            out = os.path.join(td, name)
            subprocess.run([os.path.join(REF, "kmc_tools"), "-t1", "-hp", *X.reference_argv(name, out)], check=True, capture_output=True)
            raw = open(out + ".kff", "rb").read()
            h, sections = K.file_sections(raw)
            k, ds, n, ci, cx = X.FILE_SHAPES[name]
            got = (h["k"], h["cs"], sum(len(s[0]) for s in sections), h["min_count"], h["max_count"])
            assert len(sections) == 1, (name, len(sections))  # an output without records included: one section of 0 records
            assert all(w is None or w == g for w, g in zip((k, ds, n, ci, cx), got)), (name, got)
            assert all(ks == sorted(set(ks)) for ks, _ in sections), "a section is not strictly ascending"
            assert K.encode_container(h["k"], h["cs"], h["canonical"], h["min_count"], h["max_count"], [K.encode_records(h["k"], h["cs"], *s) for s in sections]) == raw, name
            with open(X.kff_file(name), "wb") as f:
                f.write(raw)
            print(f"{name}: k {got[0]}, data_size {got[1]}, {got[2]} records, min_count {got[3]}, max_count {got[4]}, {len(raw)} bytes")
        # the twin of `count ... output_format="kff"`: kmc -okff, then the reduce
        os.makedirs(os.path.join(td, "tmp"))
        counted = os.path.join(td, "counted")
        subprocess.run([os.path.join(REF, "kmc"), "-t4", *X.COUNT_ARGV, "-okff", os.path.join(X.GOLDEN, "count_k27_fq.fq"), counted, os.path.join(td, "tmp")], check=True, capture_output=True)
        subprocess.run([os.path.join(REF, "kmc_tools"), "-t1", "-hp", "transform", counted + ".kff", "reduce", os.path.join(td, "again"), "-okff"], check=True, capture_output=True)
        assert open(os.path.join(td, "again.kff"), "rb").read() == open(X.kff_file("kffout_k27_multi"), "rb").read(), "kmc -okff + reduce differs from the recorded file"
    sizes = [os.path.getsize(os.path.join(X.GOLDEN, f)) for f in os.listdir(X.GOLDEN) if f.startswith("kffout_")]
    print(f"{len(sizes)} files, {sum(sizes)} bytes, largest {max(sizes)}")
    assert max(sizes) < 110_000


if __name__ == "__main__":
    main()
