"""Small k (k <= 13) from the table of counters to a database — kmc_hip_smallk_tally / kmc_hip_smallk_view_device (kernels k_sk_tally, k_sk_emit), capi.SmallK and
`python -m kmc_amd.tools count-small` — in the PRODUCT'S host library compiled over the emulated HIP runtime (tests/emu.py build_hostlib, small geometry), against the
numpy restatement of CSmallKCompleter and the bytes `kmc` itself wrote (tests/smallk_db_cases.py, tests/golden/smallkdb_*). k <= 9 here: the emulation runs one OS thread
per GPU thread. tests/test_gpu_smallk_db.py runs the same cases, and k = 11 .. 13, on libkmc_hip.so."""
import pytest

import emu
import smallk_db_cases as K


@pytest.fixture(scope="module")
def lib():
    c = K.SkContext(emu.build_hostlib("small"))
    yield c
    c.close()


# k = 1, 2, 4: span 1, far below a tile; k = 5: under one tile, span 256; k = 6: exactly two default tiles; k = 8: p = 4 and p = 8. One entry per thread from k = 6 on, so
# that tables of a few thousand entries cross many tile seams (16 tiles at k = 6, 256 at k = 8)
@pytest.mark.parametrize("k", [1, 2, 4, 5, 6, 8])
@pytest.mark.parametrize("fill", K.FILLS)
def test_planted_tables_against_the_restatement(lib, k, fill, monkeypatch):
    K.with_ipt(monkeypatch, 1 if k >= 6 else None)
    cs = 1 + (K.FILLS.index(fill) + k) % 4
    K.check_planted(lib, k, fill, cs, data_sizes=range(cs, 5) if fill in ("drawn", "half") and k != 8 else None)


@pytest.mark.parametrize("cs", [1, 2, 3, 4])
def test_every_counter_size_on_the_drawn_counters(lib, cs, monkeypatch):
    K.with_ipt(monkeypatch, 1)
    K.check_planted(lib, 6, "drawn", cs, data_sizes=range(cs, 5))


# k = 9 with the default tile: under p = 1 one span covers 32 tiles, under p = 5 a tile covers 8 spans, under p = 9 every entry writes a LUT word
@pytest.mark.parametrize("fill,cs", [("drawn", 4), ("seam_end", 2), ("sparse64", 1)])
def test_k9_at_every_prefix_length(lib, fill, cs, monkeypatch):
    K.with_ipt(monkeypatch, None)
    K.check_planted(lib, 9, fill, cs)


@pytest.mark.parametrize("wgs", [1, 3])
def test_a_tally_workgroup_walks_many_tiles(lib, wgs, monkeypatch):
    """16 tiles of 256 entries under 1 and 3 workgroups: an even and an odd number of tiles per workgroup, and workgroups with different numbers of them"""
    K.with_ipt(monkeypatch, 1)
    monkeypatch.setenv("KMC_HIP_SMALLK_TALLY_WGS", str(wgs))
    K.check_planted(lib, 6, "drawn", 3)
    K.check_planted(lib, 6, "seam_end", 1)


def test_k9_one_entry_per_thread(lib, monkeypatch):
    K.with_ipt(monkeypatch, 1)
    K.check_planted(lib, 9, "half", 3, prefixes=[5], data_sizes=[3])


@pytest.mark.parametrize("ipt,offset", [(1, 0), (3, 0), (None, 0), (None, 8), (2, 8), (5, 0), (99, 0)])
def test_the_bytes_do_not_depend_on_the_tile(lib, ipt, offset, monkeypatch):
    """entries per thread 1, 3 and the default give the restatement's bytes, also from a table that is not 16-byte aligned (8-byte loads) and with a value above the most"""
    K.with_ipt(monkeypatch, ipt)
    K.check_planted(lib, 6, "drawn", 2, offset=offset)
    K.check_planted(lib, 6, "seam_start", 1, offset=offset)


@pytest.mark.parametrize("name", K.OPEN_IDS)
def test_the_open_table(lib, name, monkeypatch):
    K.with_ipt(monkeypatch, 1)
    K.check_open_table(lib, name)


@pytest.mark.parametrize("name", [n for n in K.CASE_IDS if int(K.CASES[n][0][0][2:]) <= 9])
def test_count_small_writes_what_kmc_wrote(lib, name, tmp_path, monkeypatch):
    K.with_ipt(monkeypatch, None)
    K.check_golden(lib, name, tmp_path)


def test_going_on_on_the_device(lib, tmp_path, monkeypatch):
    K.with_ipt(monkeypatch, None)
    K.check_going_on(lib, tmp_path)


def test_refusals(lib, monkeypatch):
    K.with_ipt(monkeypatch, 1)
    K.check_refusals(lib)


def test_the_parser_and_the_prefix_length():
    K.check_parser()


@pytest.mark.parametrize("name", ["k4", "k5"])
def test_a_large_body_comes_down_in_parts(lib, name, tmp_path, monkeypatch):
    """the same bytes when the body is copied to the host 100 bytes at a time"""
    from kmc_amd import tools

    K.with_ipt(monkeypatch, None)
    monkeypatch.setattr(tools, "SMALLK_BODY_PART_BYTES", 100)
    K.check_golden(lib, name, tmp_path)
