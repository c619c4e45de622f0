"""The set-operation kernels in tools/resource_usage.py's table of the gfx950 code object: present for every record width, no scratch for SIZE 1 and 2."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_setop_kernels_use_no_scratch_for_one_and_two_word_records():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py")], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.match(r"(k_so_\w+<[^>]*>)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", ln)
        if m:
            rows[m.group(1).replace(" ", "")] = [int(x) for x in m.groups()[1:]]
    for size in range(1, 8):
        for name in (f"k_so_partition<{size}>", f"k_so_tile<{size},false>", f"k_so_tile<{size},true>"):
            assert name in rows, (name, sorted(rows))
    for size in (1, 2):
        for name in (f"k_so_partition<{size}>", f"k_so_tile<{size},false>", f"k_so_tile<{size},true>"):
            assert rows[name][2] == 0, (name, rows[name])  # scratch bytes
