"""The transform kernels in tools/resource_usage.py's table of the gfx950 code object: k_tr_compact present for every record width in both passes, k_tr_hist with its bins
in LDS and in HBM, k_tr_dump in both passes; no spill and no scratch in the dump and histogram kernels."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_transform_kernels_are_there_and_dump_and_histogram_use_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py")], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.match(r"(k_tr_\w+<[^>]*>)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", ln)
        if m:
            rows[m.group(1).replace(" ", "")] = dict(zip(("vgprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch", "waves"), (int(x) for x in m.groups()[1:])))
    flat = [f"k_tr_dump<{w}>" for w in ("false", "true")] + [f"k_tr_hist<{w}>" for w in ("false", "true")]
    names = flat + [f"k_tr_compact<{size},{w}>" for size in range(1, 8) for w in ("false", "true")]
    for name in names:
        assert name in rows, (name, sorted(rows))
    for name in flat:
        assert rows[name]["scratch"] == 0 and rows[name]["vgpr_spill"] == 0 and rows[name]["sgpr_spill"] == 0, (name, rows[name])
