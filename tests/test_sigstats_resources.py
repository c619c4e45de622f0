"""k_s1_sig_stats, the stage-0 histogram, in tools/resource_usage.py's table of the gfx950 code object: no scratch, no spill, no spin loop, and the occupancy class
DESIGN.md 9 documents for its two instantiations — derived here from the VGPR count and the LDS size of the table itself (profiles/r12/resource_usage.txt is the
table of the committed tree), not from a number picked in advance:
  <0> (adds straight into HBM): bound by LDS — the tile's signatures and the span of s1_signatures_to_lds — at 160 KB / LDS workgroups of 4 waves per CU, below the
      8 the registers and the launch allow;
  <7> (the workgroup-private table of 4^7 + 1 counters): one workgroup per CU."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU, VGPRS_PER_SIMD, MAX_WAVES_PER_SIMD, WAVES_PER_WG, SIMDS = 160 * 1024, 512, 8, 4, 4  # gfx950; 256-thread workgroups


def _rows(text):
    rows = {}
    for ln in text.splitlines():
        m = re.match(r"(k_s1_sig_stats<\d+>)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", ln)
        if m:
            rows[m.group(1)] = dict(zip(("vgprs", "sgprs", "vgpr_spill", "sgpr_spill", "scratch", "waves", "lds"), (int(x) for x in m.groups()[1:])))
    return rows


def test_the_statistics_kernel_uses_no_scratch_and_has_the_documented_occupancy():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "resource_usage.py")], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-1500:]
    rows = _rows(r.stdout)
    assert sorted(rows) == ["k_s1_sig_stats<0>", "k_s1_sig_stats<7>"], sorted(rows)
    with open(os.path.join(ROOT, "profiles", "r12", "resource_usage.txt")) as f:
        recorded = _rows(f.read())
    for name, g in rows.items():
        assert g["scratch"] == 0 and g["vgpr_spill"] == 0 and g["sgpr_spill"] == 0, (name, g)
        assert recorded[name]["vgprs"] == g["vgprs"] and recorded[name]["lds"] == g["lds"], (name, g, recorded[name])  # the recorded table is this tree's
        by_regs = min(MAX_WAVES_PER_SIMD, VGPRS_PER_SIMD // (-(-g["vgprs"] // 8) * 8))
        by_lds = (LDS_PER_CU // g["lds"]) * WAVES_PER_WG // SIMDS
        assert g["waves"] == min(by_regs, by_lds), (name, g, by_regs, by_lds)
    g0, g7 = rows["k_s1_sig_stats<0>"], rows["k_s1_sig_stats<7>"]
    assert LDS_PER_CU // g0["lds"] < 8 and g0["waves"] == LDS_PER_CU // g0["lds"] >= 6  # <0>: LDS-bound, six workgroups per CU at least; registers would allow 8
    assert g7["lds"] > 4 * (4**7 + 1) and g7["waves"] == 1  # <7>: the table alone is 64 KB: one workgroup per CU


def test_the_statistics_kernel_has_no_spin_loop():
    """no look-back, no ticket, no wait on another workgroup: nothing in the kernel's text polls memory or sleeps (the look-back kernels of this file do both)"""
    with open(os.path.join(ROOT, "kmc_amd", "csrc", "stage1_kernels.hip.h")) as f:
        src = f.read()
    at = src.index("k_s1_sig_stats(const int8_t")
    body = src[at:src.index("\n}\n", at)]
    assert "s1_signatures_to_lds(" in body and "s1_smallk_add<" in body  # the shared m-mer / norm / window-minimum code, the shared wave aggregation
    for word in ("s_sleep", "ld_agent", "st_agent", "lookback", "LbWatch", "lb_blocked", "while (true)", "ticket", "atomicCAS", "atomicExch"):
        assert word not in body, word
