"""k_cnt_gather, the segmented copy of the counting session, in tools/resource_usage.py's table of the gfx950 code object: no scratch and no spill (every byte of bin
records goes through it once)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_gather_kernel_uses_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py")], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.match(r"(k_cnt_\w+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = dict(zip(("vgprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch", "waves"), (int(x) for x in m.groups()[1:])))
    assert "k_cnt_gather" in rows, sorted(rows)
    g = rows["k_cnt_gather"]
    assert g["scratch"] == 0 and g["vgpr_spill"] == 0 and g["sgpr_spill"] == 0, g
    assert g["waves"] >= 4, g  # 256-thread workgroups, 8 per CU: two waves per SIMD from the launch alone; registers must not be what limits it
