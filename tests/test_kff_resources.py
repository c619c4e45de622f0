"""The KFF import kernels in tools/resource_usage.py's table of the gfx950 code object: k_kff_repack, and k_kff_unpack and k_kff_verify for every record width; no spill
and no scratch in k_kff_repack, whose records are re-framed byte by byte in LDS."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kff_kernels_are_there_and_repack_uses_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py")], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.match(r"(k_kff_\w+(?:<[^>]*>)?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", ln)
        if m:
            rows[m.group(1).replace(" ", "")] = dict(zip(("vgprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch", "waves"), (int(x) for x in m.groups()[1:])))
    for name in ["k_kff_repack"] + [f"k_kff_{w}<{size}>" for w in ("unpack", "verify") for size in range(1, 8)]:
        assert name in rows, (name, sorted(rows))
    row = rows["k_kff_repack"]
    assert row["scratch"] == 0 and row["vgpr_spill"] == 0 and row["sgpr_spill"] == 0, row
