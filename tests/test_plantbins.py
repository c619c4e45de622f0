"""CPU: tests/plantbins.py itself — the bins the planted-bucket sweep is made of must be what the sweep says they are, whatever library reads them."""
import numpy as np
import pytest

import oracle_py as O
import plantbins


def _geometries():
    yield plantbins.geometry_of(0), True
    for name in ("small", "small_tight"):
        yield plantbins.geometry_of(1, f"libkmc_hip_emu_{name}.so", env={}), False


def test_geometry_comes_from_the_header_and_the_emulated_flags():
    g = plantbins.geometry_of(0)
    assert (g.MID + 1, g.CAP, g.S) == (2 * g.DS, g.THREADS * 8, g.CAP - g.CAP // 12), g  # the product's inequality is tight
    t = plantbins.geometry_of(1, "/x/libkmc_hip_emu_small_tight.so", env={})
    assert (t.MID, t.DS, t.CAP) == (175, 88, 1024)
    assert plantbins.geometry_of(1, "", env={"KMC_PLANT_GEOMETRY": "small"}).MID == 192
    with pytest.raises(AssertionError):
        plantbins.geometry_of(1, "libsomething.so", env={})
    with pytest.raises(AssertionError):
        plantbins.geometry_of(2)


@pytest.mark.parametrize("case", plantbins.CASES)
def test_every_case_is_what_it_says_in_every_geometry(case):
    """the builder's own assertions (whole buckets, every residue, every named placement, no planted bucket in arrival order) hold, and the ordered records it reasons about
    are the oracle's expansion of the image it wrote — k-mer packing, pack sizes and both strands included"""
    for geo, device in _geometries():
        if device and case == "sweep-k27":
            continue  # 4 M records: built (and its assertions run) by the -m gpu test
        k, kw, bins, planted, ordered, rbits = plantbins.make_case(geo, case, device)
        op = O.make_params(k, kw.get("both_strands", 1))
        for (img, n, packs, _), o in zip(bins, ordered):
            assert int(packs.sum()) == img.size and packs.size == -(-n // plantbins.PACK_SUPERKMERS)
            assert np.array_equal(np.sort(O.expand(op, img)[:, 0]), o)
        g_n, g_rec = plantbins.n_giant(geo, planted)
        assert (g_n > 0) == (case in ("sweep-k27", "edges-k27", "giant-run-k27"))


def test_sweep_lengths_hold_what_the_sweep_promises():
    for geo, device in _geometries():
        ls = plantbins.sweep_lengths(geo, device)
        assert {geo.DS, geo.MID, geo.MID + 1, geo.MID + 2, 2 * geo.DS - 1, 2 * geo.DS, geo.CAP, geo.CAP + 1} <= set(ls) and len(ls) == len(set(ls))
        if device:
            assert set(range(geo.MID - 11, geo.MID + 15)) | {geo.DS + 1} <= set(ls)
