"""Makes tests/golden/transform_*: what `kmc_tools -t1 -hp transform` writes for every command line of transform_cases.LINES, from the databases already under
tests/golden (setops_k27_a, setops_k33_a, setops_k33_raw_a — the KMC2 database `kmc` wrote —, setops_k55_a). Runs the reference's kmc_tools from oracle/_ref and keeps
only the data it writes: text outputs gzipped with mtime 0 (transform_<line>_<output>.txt.gz), databases as they are (.kmc_pre / .kmc_suf).

    python tests/make_transform_golden.py
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import setops_cases as S  # noqa: E402
import transform_cases as T  # noqa: E402
from kmc_amd import dbio  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")


def main():
    for f in os.listdir(T.GOLDEN):
        if f.startswith("transform_"):
            os.remove(os.path.join(T.GOLDEN, f))
    with tempfile.TemporaryDirectory() as td:
        for line in T.LINES:
            name, fixture, _, outs = line
            db = dbio.read_database(T.fixture_path(fixture))
            if db.kmc2:
                assert int(db.raw_lut[-1]) == db.total_kmers and db.raw_lut.size == len(db.bins) * (1 << (2 * db.lut_prefix_len)) + 1
            paths = [os.path.join(td, T.out_name(line, i)) for i in range(len(outs))]
            # Two dump outputs on one command line are beyond the reference: its vector of dump writers grows by copying a writer whose symbol table the copy's source
            # then frees (kmc_tools.cpp:47,63; dump_writer.h:104-107) — the first dump is written from freed memory and the run ends in abort(). Every output is
            # computed from the same walk over the input, whatever else is on the line, so such a line is recorded in one run per dump, each without the other dumps
            # (the database outputs stay, and with them the order of the walk); what the runs share must agree.
            dumps = [i for i, (op, _) in enumerate(outs) if op[0] == "dump"]
            seen = {}
            for keep in (dumps if len(dumps) >= 2 else [None]):
                idxs = [i for i in range(len(outs)) if keep is None or i == keep or i not in dumps]
                sub = (name, fixture, line[2], [outs[i] for i in idxs])
                assert T.resolve_line(sub, dict(S.header_of(db), kmc2=db.kmc2))[1] == T.resolve_line(line, dict(S.header_of(db), kmc2=db.kmc2))[1]
                for i in idxs:
                    for ext in ("", ".kmc_pre", ".kmc_suf"):
                        if os.path.exists(paths[i] + ext):
                            os.remove(paths[i] + ext)
                subprocess.run([os.path.join(REF, "kmc_tools"), "-t1", "-hp", *T.command_line(sub, T.fixture_path(fixture), [paths[i] for i in idxs])], check=True, capture_output=True)
                for i in idxs:
                    got = tuple(open(paths[i] + ext, "rb").read() for ext in ("", ".kmc_pre", ".kmc_suf") if os.path.exists(paths[i] + ext))
                    assert seen.setdefault(i, got) == got, (name, i)
            in_cut, need_order, res = T.resolve_line(line, dict(S.header_of(db), kmc2=db.kmc2))
            written = {r["index"] for r in res}
            tallies = {}
            for idx, kind, want, st in T.restate_line(line, db):
                tallies[idx] = st
            for i, (op, _) in enumerate(outs):
                if i not in written:
                    assert not os.path.exists(paths[i] + ".kmc_pre"), "a sort of an ordered database was written"
                    continue
                if T.is_text(op):
                    with open(paths[i], "rb") as f:
                        T.write_golden_text(line, i, f.read())
                else:
                    for ext in (".kmc_pre", ".kmc_suf"):
                        with open(paths[i] + ext, "rb") as f, open(T.golden_out(line, i) + ext, "wb") as g:
                            g.write(f.read())
            print(f"{name}: order {need_order}, " + "; ".join(f"{outs[i][0][0]} {st}" for i, st in sorted(tallies.items())))
            # every line does what it is for
            st0 = tallies.get(0)
            if name in ("k27_reduce", "k27_dump_cut"):
                assert st0["n_below_min"] > 0 and st0["n_above_max"] > 0, "nothing cut at both ends"
                kept = T.restate_reduce(*T.file_order(db), in_cut, 3 if name == "k27_reduce" else 2, 20, 10)[1]
                assert kept.count(10) > 1 and max(kept) == 10, "nothing clamped"
            if name == "k27_set300":
                assert dbio.read_database(T.golden_out(line, 0)).counter_size == 2
            if name == "k27_set0":
                o = dbio.read_database(T.golden_out(line, 0))
                assert o.counter_size == 4 and o.total_kmers == db.total_kmers and o.max_count == S.U32
            if name == "k27_compact":
                assert dbio.read_database(T.golden_out(line, 0)).counter_size == 1 and set(dbio.read_database(T.golden_out(line, 0)).recs.reshape(-1, 7)[:, 6]) == {1}
            if name == "k27_multi":
                assert all(tallies[i]["n_cut_in"] > 0 for i in range(4)) and tallies[0]["n_above_max"] > 0 and tallies[3]["n_below_min"] > 0
            if name == "k33raw_dump":
                raw_dump = T.read_golden_text(line, 0)
            if name == "k33raw_dump_s":
                assert T.read_golden_text(line, 0) != raw_dump and sorted(T.read_golden_text(line, 0).split(b"\n")) == sorted(raw_dump.split(b"\n")), "bin order is the sorted order"
            if name == "k33raw_sort":
                assert T.golden_database_files(line, 0) == tuple(open(T.fixture_path("setops_k33_a") + e, "rb").read() for e in (".kmc_pre", ".kmc_suf"))
            if name == "k33raw_reduce_dump":
                assert tallies[0]["n_below_min"] > 0 and T.read_golden_text(line, 1).split(b"\n") == sorted(T.read_golden_text(line, 1).split(b"\n"))[1:] + [b""], "the dump next to a database output is not ordered"
            if name == "k33_sort_hist":
                assert written == {1}
            if name == "k55_reduce":
                assert st0["n_above_max"] > 0
    sizes = [os.path.getsize(os.path.join(T.GOLDEN, f)) for f in os.listdir(T.GOLDEN) if f.startswith("transform_")]
    print(f"{len(sizes)} files, {sum(sizes)} bytes, largest {max(sizes)}")
    assert sum(sizes) < 1_000_000 and max(sizes) < 1 << 20


if __name__ == "__main__":
    main()
