"""The small-k database kernels in tools/resource_usage.py's table of the gfx950 code object: k_sk_tally and k_sk_emit are there, in both instantiations (16-byte and
8-byte loads), without spill and without scratch — a thread's up to eight counters and their ranks stay in registers because every loop over them is unrolled."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_smallk_db_kernels_are_there_and_use_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py")], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.match(r"(k_sk_\w+(?:<[^>]*>)?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", ln)
        if m:
            rows[m.group(1).replace(" ", "")] = dict(zip(("vgprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch", "waves"), (int(x) for x in m.groups()[1:])))
    for name in ("k_sk_tally<true>", "k_sk_tally<false>", "k_sk_emit<true>", "k_sk_emit<false>"):
        assert name in rows, sorted(rows)
        row = rows[name]
        assert row["scratch"] == 0 and row["vgpr_spill"] == 0 and row["sgpr_spill"] == 0, (name, row)
