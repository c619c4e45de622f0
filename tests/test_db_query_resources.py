"""The query kernels in tools/resource_usage.py's table of the gfx950 code object: k_dbq_lookup present for every record width, the three phases of k_dbq_reads present,
no spill and no scratch in k_dbq_lookup for SIZE 1 and 2 (the lookups of k <= 64) nor in k_dbq_reads."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_kernels_are_there_and_use_no_scratch_for_one_and_two_word_kmers():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py")], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.match(r"(k_dbq_\w+<[^>]*>)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", ln)
        if m:
            rows[m.group(1).replace(" ", "")] = dict(zip(("vgprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch", "waves"), (int(x) for x in m.groups()[1:])))
    names = [f"k_dbq_lookup<{size}>" for size in range(1, 8)] + [f"k_dbq_reads<{phase}>" for phase in range(3)]
    for name in names:
        assert name in rows, (name, sorted(rows))
    for name in names[:2] + names[7:]:
        assert rows[name]["scratch"] == 0 and rows[name]["vgpr_spill"] == 0, (name, rows[name])
