"""The BGZF kernel in tools/resource_usage.py's table of the gfx950 code object: k_bgzf_inflate is there, without VGPR spill and without scratch — its decode tables and
its window live in LDS, and the arrays the table builder keeps (codes per length, first codes, offsets) are indexed by unrolled constants only."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bgzf_inflate_is_there_and_uses_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py")], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.match(r"(k_bgzf_\w+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = dict(zip(("vgprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch", "waves", "lds"), (int(x) for x in m.groups()[1:])))
    assert "k_bgzf_inflate" in rows, sorted(rows)
    for name, row in rows.items():
        assert row["scratch"] == 0 and row["vgpr_spill"] == 0, (name, row)
    assert 65536 + 16 <= rows["k_bgzf_inflate"]["lds"] <= 80 * 1024, rows  # the whole window, and two workgroups a CU (160 KiB)
