"""Kernel times of the KFF import from rocprofv3 kernel statistics (`--kernel-trace --stats --output-format csv`) of tools/db_kff_bench.py runs, each a profiler run
of its own: per (k, section shape) one run with --only-repack — k_kff_repack's row is then one k and one shape, 6 calls — and per k one full run with --no-reference for the
split of the two ordering paths (6 calls of each entry; the sort's kernels are shared by the two paths and halved, as is k_db_cumsum's row).

    python tools/db_kff_trace.py --repack 27:one_section:<stats.csv> 27:512_sections:<stats.csv> ... --order 27:<stats.csv> 127:<stats.csv> [--out profiles/r11/db_kff_kernel_trace.json]
"""
import argparse
import csv
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows_of(path):
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            name = re.sub(r"\(.*", "", r["Name"]).replace("void ", "")
            out[name] = dict(calls=int(r["Calls"]), total_us=int(r["TotalDurationNs"]) / 1e3, avg_us=float(r["AverageNs"]) / 1e3, min_us=int(r["MinNs"]) / 1e3, max_us=int(r["MaxNs"]) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repack", nargs="*", default=[], help="k:shape:stats.csv of an --only-repack run")
    ap.add_argument("--order", nargs="*", default=[], help="k:stats.csv of a full run of one k")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "db_kff_kernel_trace.json"))
    a = ap.parse_args()
    res = dict(source="rocprofv3 --kernel-trace --stats over tools/db_kff_bench.py, one profiler run per entry below; microseconds", k_kff_repack={}, ordering={})
    for spec in a.repack:
        k, shape, path = spec.split(":", 2)
        res["k_kff_repack"].setdefault(k, {})[shape] = rows_of(path)["k_kff_repack"]
    for spec in a.order:
        k, path = spec.split(":", 1)
        rows = rows_of(path)
        size = (int(k) + 31) // 32

        def per_call(name, calls):
            return rows[name]["total_us"] / calls

        sort = dict(k_hist=per_call(f"k_hist<{size + 1}>", 12), k_onesweep=per_call(f"k_onesweep<{size + 1}>", 12))
        imp = dict(k_kff_unpack=per_call(f"k_kff_unpack<{size}>", 6), **sort, k_kff_verify=per_call(f"k_kff_verify<{size}>", 6), k_db_pack=per_call(f"k_db_pack<{size}>", 12))
        odb = dict(k_db_cumsum_x512=per_call("k_db_cumsum", 6), k_db_unpack_x512=per_call(f"k_db_unpack<{size}>", 6), **sort, k_db_pack=imp["k_db_pack"])
        res["ordering"][k] = dict(kff_import_512_sections=imp, order_database_512_bins=odb, kernels_sum=dict(kff_import=sum(imp.values()), order_database=sum(odb.values())))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
