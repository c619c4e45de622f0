"""The compare kernels in tools/resource_usage.py's table of the gfx950 code object: k_db_compare and k_db_compare_finish present for every record width, no scratch and
no spill at any of them, and no LDS in k_db_compare (its wave reduction goes through registers)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compare_kernels_use_no_scratch_at_any_width():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py")], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.match(r"(k_db_compare\w*<[^>]*>)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", ln)
        if m:
            rows[m.group(1).replace(" ", "")] = dict(zip(("vgprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch", "waves", "lds"), (int(x) for x in m.groups()[1:])))
    for size in range(1, 8):
        for name in (f"k_db_compare<{size}>", f"k_db_compare_finish<{size}>"):
            assert name in rows, (name, sorted(rows))
            assert rows[name]["scratch"] == 0 and rows[name]["vgpr_spill"] == 0 and rows[name]["sgpr_spill"] == 0, (name, rows[name])
        assert rows[f"k_db_compare<{size}>"]["lds"] == 0, rows[f"k_db_compare<{size}>"]
