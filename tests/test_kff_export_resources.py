"""The KFF export kernel in tools/resource_usage.py's table of the gfx950 code object: k_kff_frame is there, without spill and without scratch — its records are framed
byte by byte in LDS, and the prefix search keeps two indices and no array."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kff_frame_is_there_and_uses_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py")], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.match(r"(k_kff_\w+(?:<[^>]*>)?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", ln)
        if m:
            rows[m.group(1).replace(" ", "")] = dict(zip(("vgprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch", "waves"), (int(x) for x in m.groups()[1:])))
    assert "k_kff_frame" in rows, sorted(rows)
    row = rows["k_kff_frame"]
    assert row["scratch"] == 0 and row["vgpr_spill"] == 0 and row["sgpr_spill"] == 0, row
