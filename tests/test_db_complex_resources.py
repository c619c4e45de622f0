"""The expression kernels in tools/resource_usage.py's table of the gfx950 code object: k_cx_partition for every record width, k_cx_tile for every width in both passes;
no spill and no scratch — the value stack of k_cx_tile is indexed statically (it is shifted on every push and pop), so it lies in registers."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expression_kernels_are_there_and_use_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py")], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.match(r"(k_cx_\w+<[^>]*>)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", ln)
        if m:
            rows[m.group(1).replace(" ", "")] = dict(zip(("vgprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch", "waves"), (int(x) for x in m.groups()[1:])))
    names = [f"k_cx_partition<{size}>" for size in range(1, 8)] + [f"k_cx_tile<{size},{w}>" for size in range(1, 8) for w in ("false", "true")]
    for name in names:
        assert name in rows, (name, sorted(rows))
        assert rows[name]["scratch"] == 0 and rows[name]["vgpr_spill"] == 0 and rows[name]["sgpr_spill"] == 0, (name, rows[name])
