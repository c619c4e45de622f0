"""Makes tests/golden/kff_*.kff and tests/golden/kffline_*: KFF files as the reference writes them (kff_cases.FILES: `kmc_tools transform <db> reduce <out> -okff` of
the set-operation fixtures — one section each —, one of them with -cs65535 so that data_size is 2, and `kmc -okff` of a committed count input — one section per bin
pack), and what `kmc_tools -t1 -hp` writes for every command line of kff_cases.LINES over them. Runs the reference's kmc and kmc_tools from oracle/_ref and keeps only
the data files: databases as they are, text and reads gzipped with mtime 0.

The multi-section file: with kmc's default signature length the few reads of a count_* input all fall into ONE bin, hence one section; -p5 spreads them over 58 bin
packs (58 sections, none of them empty — empty sections are covered by the planted cases). Dropped: `transform <multi-section kff> histogram <out>` alone — the
reference's counters-only reader ends in a segmentation fault on that file; the histogram is recorded next to a dump on one line instead (the sequential reader).
Every other line ran in the reference, the KFF random access of `filter` included.

    python tests/make_kff_golden.py
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
from kmc_amd import dbio  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def main():
    for f in os.listdir(K.GOLDEN):
        if f.startswith(("kff_", "kffline_")):
            os.remove(os.path.join(K.GOLDEN, f))
    with tempfile.TemporaryDirectory() as td:
        for name, (tool, args) in K.FILES.items():
            out = os.path.join(td, name)
            argv = [a.format(g=K.GOLDEN, out=out) for a in args]
            if tool == "kmc":
                os.makedirs(os.path.join(td, "tmp_" + name))
                subprocess.run([os.path.join(REF, "kmc"), "-t4", *argv, os.path.join(td, "tmp_" + name)], check=True, capture_output=True)
            else:
                subprocess.run([os.path.join(REF, "kmc_tools"), "-t1", "-hp", *argv], check=True, capture_output=True)
            raw = open(out + ".kff", "rb").read()
            h, sections = K.file_sections(raw)
            assert (h["k"], h["cs"], len(sections), sum(len(s[0]) for s in sections)) == K.FILE_SHAPES[name], (name, h["k"], h["cs"], len(sections), sum(len(s[0]) for s in sections))
            assert all(ks == sorted(set(ks)) for ks, _ in sections), "a section is not strictly ascending"
            # the restatement writes the same file
            assert K.encode_container(h["k"], h["cs"], h["canonical"], h["min_count"], h["max_count"], [K.encode_records(h["k"], h["cs"], *s) for s in sections]) == raw, name
            with open(K.kff_file(name), "wb") as f:
                f.write(raw)
            print(f"{name}: k {h['k']}, data_size {h['cs']}, {len(sections)} sections, {sum(len(s[0]) for s in sections)} records, {len(raw)} bytes")
        _, multi = K.file_sections(open(K.kff_file("kff_k27_multi"), "rb").read())
        flat = [x for ks, _ in multi for x in ks]
        assert flat != sorted(flat), "the sections' ranges do not interleave: the sort would have nothing to do"
        for line in K.LINES:
            argv, outs = K.command_line(line, td)
            subprocess.run([os.path.join(REF, "kmc_tools"), "-t1", "-hp", *argv], check=True, capture_output=True)
            for i, (path, kind) in enumerate(zip(outs, line[3])):
                data = K.output_bytes(path, kind)
                assert all(len(d) > 0 for d in data), (line[0], i)
                K.write_golden(line, i, kind, data)
            print(line[0], [len(d) for path, kind in zip(outs, line[3]) for d in K.output_bytes(path, kind)])
        # what the lines are for
        by = {ln[0]: ln for ln in K.LINES}
        assert K.read_golden(by["multi_dump"], 0, "txt") != K.read_golden(by["multi_dump_s"], 0, "txt"), "file order is the sorted order"
        assert sorted(K.read_golden(by["multi_dump"], 0, "txt")[0].split(b"\n")) == sorted(K.read_golden(by["multi_dump_s"], 0, "txt")[0].split(b"\n"))
        for name, twin in K.TWINS.items():  # the twin KMC runs already recorded: the same records under another lut_prefix_len
            got, want = dbio.read_database(K.golden_out(by[name], 0)), dbio.read_database(os.path.join(K.GOLDEN, twin))
            import setops_cases as S

            assert S.decode_body(got.kmer_len, got.lut_prefix_len, got.counter_size, got.lut, got.recs) == S.decode_body(want.kmer_len, want.lut_prefix_len, want.counter_size, want.lut, want.recs), name
            if by[name][1] == "transform":  # one KFF input: total_kmers 0, the smallest valid prefix length
                assert got.lut_prefix_len == K.smallest_p(got.kmer_len), (name, got.lut_prefix_len)
            print(f"{name}: lut_prefix_len {got.lut_prefix_len}, its KMC twin {want.lut_prefix_len}")
        import gzip

        with gzip.open(os.path.join(K.GOLDEN, "filter_out_k27_normal_defaults.gz"), "rb") as f:
            assert f.read() == K.read_golden(by["k27_filter"], 0, "fq")[0], "filter over the KFF twin differs from filter over the KMC database"
        assert dbio.read_database(K.golden_out(by["k27_cs2_reduce_hist"], 0)).counter_size == 2
        assert dbio.read_database(K.golden_out(by["k33_reduce"], 0)).lut_prefix_len == 1 and dbio.read_database(os.path.join(K.GOLDEN, K.TWINS["k33_reduce"])).lut_prefix_len == 5
    sizes = [os.path.getsize(os.path.join(K.GOLDEN, f)) for f in os.listdir(K.GOLDEN) if f.startswith(("kff_", "kffline_"))]
    print(f"{len(sizes)} files, {sum(sizes)} bytes, largest {max(sizes)}")
    assert sum(sizes) < 1_000_000 and max(sizes) < 1 << 20


if __name__ == "__main__":
    main()
