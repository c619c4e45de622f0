"""GPU: BGZF input on the device — the kernel cases and corruptions of tests/bgzf_cases.py through libkmc_hip.so (the corruptions are tests of error returns on bounded
code: they passed under the CPU emulation, tests/test_bgzf_emulated.py, before their first device run), a batch of more waves than the chip holds at once, and `count` /
`count-small` on a recorded BAM file and on a bgzipped twin of a recorded FASTQ. The oracle is zlib; the expected databases are reference outputs under tests/golden."""
import numpy as np
import pytest

import bgzf_cases as B
import count_cases as CC
from kmc_amd import capi, tools

pytestmark = pytest.mark.gpu


def test_block_types_match_geometry_and_sizes(ctx):
    B.check_kernel_cases(ctx)
    B.check_kernel_cases(ctx, device=True)


def test_many_members_odd_offsets_and_an_odd_source_address(ctx):
    B.check_placements(ctx)


def test_every_corruption_is_refused_as_zlib_refuses_it(ctx):
    assert B.check_corruptions(ctx) == B.CORRUPTION_REASONS
    assert B.check_corruptions(ctx, device=True) == B.CORRUPTION_REASONS


def test_more_members_than_the_chip_holds_at_once(ctx):
    """2000 members of 4 KB, about 8 MB of output; one of them damaged in a second run: every other member is still right"""
    kinds = [B.member(B.text(300 + i, 4096), (1, 6, 9)[i % 3]) for i in range(12)] + [B.member(B.noise(7, 4096), 0), B.member(B.text(8, 4096), 6, B.zlib.Z_FIXED)]
    members = [kinds[(i * 5) % len(kinds)] for i in range(2000)]
    blob = b"".join(members)
    got, _ = B.check(ctx, blob, expect_bad=[], device=True)
    assert got.size == 2000 * 4096
    bad = 1234
    at = sum(len(m) for m in members[:bad]) + len(members[bad]) - 8
    blob = blob[:at] + bytes([blob[at] ^ 1]) + blob[at + 1:]
    _, errs = B.check(ctx, blob, expect_bad=[bad])
    assert capi.BGZF_REASONS[int(errs[bad])] == "crc"


def test_count_bam_writes_what_the_reference_wrote(ctx, tmp_path):
    out = str(tmp_path / "out")
    res = tools.count(B.BAM_CASES["k27_b"][0] + ["-n8", B.bam_path("k27_b"), out], ctx=ctx, part_bytes=4096, input_format="bam")
    assert B.database_bytes(out) == B.database_bytes(B.bam_out("k27_b")) and res["n_parts"] > 5


def test_count_on_a_bgzipped_fastq_writes_the_recorded_database(ctx, tmp_path):
    fname, _, data = CC.CASES["k27_fq"][2][0]
    path, out = str(tmp_path / (fname + ".gz")), str(tmp_path / "out")
    with open(path, "wb") as f:
        f.write(B.bgzipped(data, 900))
    tools.count(CC.CASES["k27_fq"][0] + ["-n8", path, out], ctx=ctx, part_bytes=2048)
    assert CC.database_bytes(out) == CC.database_bytes(CC.golden_out("k27_fq"))


def test_count_small_bam(ctx, tmp_path):
    out = str(tmp_path / "out")
    tools.count_small(B.BAM_CASES["k9"][0] + [B.bam_path("k9"), out], ctx=ctx, part_bytes=4096, input_format="bam")
    assert B.database_bytes(out) == B.database_bytes(B.bam_out("k9"))
