"""CPU: tests/plantbins.py itself — the bins the planted-bucket sweep is made of must be what the sweep says they are, whatever library reads them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emu
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


# ------------------------------------------------------------------------------------------------ records of two words and more
def _small():
    return plantbins.geometry_of(1, "libkmc_hip_emu_small.so", env={})


def test_wide_geometry_and_plans():
    d, s = plantbins.geometry_of(0), _small()
    assert [(d.wide(z).CAP, d.wide(z).S, d.wide(z).GT_CHUNK) for z in (2, 3, 8)] == [(3072, 2816, 4096), (1536, 1408, 2048), (1536, 1408, 2048)]
    assert (d.GT_MAX, d.BIG, s.GT_MAX, s.BIG) == (1 << 20, 128, 2048, 128)
    assert [(s.wide(z).CAP, s.wide(z).S, s.wide(z).GT_CHUNK) for z in (2, 3)] == [(512, 470, 1024), (256, 235, 512)]
    assert plantbins.plan_for(55, 1, 10**5, d, env={}) == plantbins.plan_for(55, 4, 10**5, d, env={}) == (80, 4, True)
    assert plantbins.plan_for(55, 4, 10**5, d, env={"KMC_HIP_INDIRECT": "0"}) == (80, 4, False)
    assert plantbins.plan_for(64, 1, 10**5, d, env={}) == (80, 6, False) and plantbins.plan_for(40, 3, 10**5, d, env={}) == (48, 5, False)
    assert plantbins.plan_for(200, 1, 10**5, d, env={}) == (368, 4, True) and plantbins.plan_for(200, 2, 10**5, d, env={}) == (368, 5, False)
    # the plan leaves whole bytes below the passes: around 64 the reachable values are 56, 64 and 72
    assert {plantbins.plan_for(k, n, 10**5, d, env={})[0] for k in range(33, 57) for n in (1, 2, 3, 5, 9)} == {32, 40, 48, 56, 64, 72, 80}
    assert plantbins.giant_passes(72) % 2 == 1 and plantbins.giant_passes(80) % 2 == 0
    for bad in (lambda: plantbins.plan_for(55, 1, 100, d, env={}), lambda: plantbins.plan_for(127, 1, 10**5, d, 33, env={}), lambda: plantbins.plan_for(27, 1, 10**5, d, env={})):
        with pytest.raises(AssertionError):
            bad()
    assert plantbins.group_sizes(55, 4) == [4] and plantbins.group_sizes(64, 2) == [1, 1] and plantbins.group_sizes(127, 6) == [4, 2] and plantbins.group_sizes(200, 18) == [16, 2]


@pytest.mark.parametrize("k,both", [(55, 0), (55, 1), (70, 0), (96, 1), (127, 1), (200, 0), (256, 0)])
def test_wide_image_round_trips_through_the_oracle(k, both):
    """image_of_wide / revcomp_wide / the both-strands trick: the oracle's expansion of the image is the records the helper ordered, and its counts are numpy's"""
    geo = _small()
    size = plantbins.words_of(k)
    rb, _, _ = plantbins.plan_for(k, 1, 10**4, geo, env={})
    b = plantbins.WideBin(geo.wide(size), k, rb, np.random.default_rng(k + both), both, plantbins.lows_generators(rb, size))
    b.fill(300)
    for L in (30, 200):
        b.plant_named(None, L, "x")
        b.fill(17)
    (img, n, packs, _), planted, ordered = b.build()
    op = O.make_params(k, both, cutoff_min=2, cutoff_max=20, lut_prefix_len=0, output_type=1)
    assert int(packs.sum()) == img.size and n == b.pos
    exp = O.expand(op, img)
    assert np.array_equal(exp[plantbins.order_of(exp)], ordered)
    out, lut, stats = O.process_bin(op, img, n)
    distinct, below, above, total, counted = plantbins.independent_counts(ordered, 2, 20)
    assert [int(x) for x in stats] == [distinct, below, above, total] and above >= 1 and out.size == counted * ((k + 3) // 4 + 1)
    ints = plantbins.to_ints(ordered)
    assert ints == sorted(ints) and np.array_equal(plantbins.to_words(ints, size), ordered)
    r = plantbins.revcomp_wide(ordered[:50], k)
    assert np.array_equal(plantbins.revcomp_wide(r, k), ordered[:50])
    comp = {0: 3, 1: 2, 2: 1, 3: 0}
    v = ints[7]
    want = sum(comp[(v >> (2 * j)) & 3] << (2 * (k - 1 - j)) for j in range(k))
    assert plantbins.to_ints(r[7:8]) == [want]


@pytest.mark.parametrize("rbits,size", [(56, 2), (64, 2), (72, 2), (80, 2), (112, 3), (224, 4), (480, 8)])
def test_lows_generators_produce_what_their_names_say(rbits, size):
    rng = np.random.default_rng(rbits)
    gens = plantbins.lows_generators(rbits, size)
    nd = (rbits + 31) // 32
    dw = lambda v: [(v >> (32 * d)) & 0xFFFFFFFF for d in range(nd + 1)]
    assert sum(g.startswith("one-dword") for g in gens) == nd and ("ab-split" in gens) == (size == 2) and any(g.startswith("borrow") for g in gens)
    for g in gens:
        vals = plantbins.lows_values(g, rbits, np.random.default_rng(len(g)))
        assert len(set(vals)) == len(vals) >= 2 and all(0 <= v < (1 << rbits) for v in vals)
        rows = plantbins.lows_named(g, 64, rbits, size, np.random.default_rng(len(g)))
        assert set(plantbins.to_ints(rows)) == set(vals)
        if g.startswith("one-dword-differs"):
            i = int(g.split("[")[1][:-1])
            assert all([d for d in range(nd) if dw(a)[d] != dw(vals[0])[d]] == [i] for a in vals[1:])
        elif g.startswith("borrow-through"):
            i, j = (int(x) for x in g.split("[")[1][:-1].split(".."))
            A, C, E = vals[0], vals[-1], vals[-2]
            assert all(dw(A)[d] == 0xFFFFFFFF for d in range(i, j + 1))
            assert [d for d in range(nd + 1) if dw(A)[d] != dw(E)[d]] == [j + 1]
            assert C == A + (1 << (32 * i)) and all(dw(C)[d] == 0 for d in range(i, j + 1)) and dw(C)[j + 1] == dw(A)[j + 1] + 1 and dw(C)[:i] == dw(A)[:i]
            assert (len(vals) == 4) == (i > 0) and (i == 0 or [d for d in range(nd + 1) if dw(A)[d] != dw(vals[1])[d]] == [0])
        elif g == "extremes":
            assert vals == [0, (1 << rbits) - 1, 1, 1 << (rbits - 1)]
        elif g == "ab-split":
            assert sorted((v ^ vals[0]).bit_length() - 1 for v in vals[1:]) == sorted({b for b in (0, 15, 16, 17, 47, 48, 63, 64, rbits - 1) if b < rbits})
            assert all(bin(v ^ vals[0]).count("1") == 1 for v in vals[1:])
        else:
            assert g == "ties" and 3 <= len(vals) <= 7


@pytest.mark.parametrize("case", [c for c in plantbins.WIDE_CASES if c != "w2-k55-indirect-off"])
def test_every_wide_case_is_what_it_says_in_the_small_geometry(case):
    c = plantbins.make_wide_case(_small(), case, env={})
    op = O.make_params(c.k, c.kw["both_strands"])
    for (img, n, packs, _), o in zip(c.bins, c.ordered):
        exp = O.expand(op, img)
        assert np.array_equal(exp[plantbins.order_of(exp)], o)
    g_n, g_rec, back = plantbins.n_giant_wide(c.wg, c.planted)
    assert g_n >= 2 and back == ([1] if case.startswith("gt-max") else [])


def test_the_product_geometry_admits_every_named_wide_placement():
    for case in ("w2-k55", "w4-k127"):
        c = plantbins.make_wide_case(plantbins.geometry_of(0), case, env={})
        assert set(plantbins.full_names(c.wg)) <= c.names and not any(n.endswith("@is-chunk1") for n in c.names)  # CAP - S + 1 >= BR_BIG + 1 there (see plantbins)
    assert any(n.endswith("@is-chunk1") for n in plantbins.make_wide_case(_small(), "w3-k70", env={}).names)


# clause of check_named_wide (the placement's name up to its parameters) -> the move of its own bucket that the clause must reject: (first, length) -> (first, length)
_WIDE_MOVES = {
    "bin-start": lambda f, L, wg: (7, L),
    "bin-end-middle-bin": lambda f, L, wg: (f - 3, L),
    "bin-end-last-bin": lambda f, L, wg: (f - 3, L),
    "tile-exactly-cap": lambda f, L, wg: (f + 7, L),
    "tile-cap-plus-1": lambda f, L, wg: (f + 7, L),
    "bucket-cap@window-first": lambda f, L, wg: (f + 7, L),
    "bucket-cap@window-last": lambda f, L, wg: (f + 7, L),
    "bucket-cap-plus-1@window-first": lambda f, L, wg: (f + 7, L),
    "bucket-cap-plus-1@window-last": lambda f, L, wg: (f + 7, L),
    "big@row": lambda f, L, wg: (f + 7, L),
    "big@wave": lambda f, L, wg: (f + wg.WAVE, L),          # the clause takes any bucket that lies over the first wave seam: moved behind the seam
    "big@ends-chunk0": lambda f, L, wg: (f + 7, L),
    "big@is-chunk1": lambda f, L, wg: (f - 3, L),
    "bounds-distance": lambda f, L, wg: (f + 7, L),
    "windows-without-a-start": lambda f, L, wg: (f, L - 2 * wg.S),
    "giant-chunk": lambda f, L, wg: (f, L + 2),
    "giant-run": lambda f, L, wg: (f + 3, L),
    "gt-max": lambda f, L, wg: (f, L - 1),
    "gt-max-plus-1": lambda f, L, wg: (f, L + 1),
}
_NO_CLAIM = {"lows", "second-chunk", "inner-big"}  # planted for their low bits or as the rest of another placement: no place of their own is claimed


def _clause_of(place):
    if place.startswith("big-"):
        return "big@" + place.split("@")[1]
    return "bounds-distance" if place.startswith("bounds-distance-") else place


@pytest.mark.parametrize("case", ["w2-k55-4bins", "w3-k70", "giant-run-k55", "gt-max-k127"])
def test_every_wide_check_rejects_a_misplaced_bucket(case):
    """check_named_wide with ONE planted bucket moved as _WIDE_MOVES says, everything else as built: every clause must fail on every bucket it speaks of. The four cases
    together hold every clause (asserted by test_the_moves_cover_every_clause)."""
    c = plantbins.make_wide_case(_small(), case, env={})
    plantbins.check_named_wide(c.wg, c.planted, c.ordered, c.rbits)
    n = 0
    for bi, pl in enumerate(c.planted):
        for j, (f, L, name) in enumerate(pl):
            clause = _clause_of(name.split("|")[0])
            if clause in _NO_CLAIM:
                continue
            f2, L2 = _WIDE_MOVES[clause](f, L, c.wg)
            moved = [list(x) for x in c.planted]
            moved[bi][j] = (f2, L2, name)
            with pytest.raises(AssertionError):
                plantbins.check_named_wide(c.wg, moved, c.ordered, c.rbits)
            n += 1
    assert n >= 3
    if len(c.planted) >= 3:  # a bucket named for the last bin in a middle bin, and the other way round; the bin that comes back anywhere but in the middle
        for bi, pl in enumerate(c.planted):
            for j, (f, L, name) in enumerate(pl):
                swap = {"bin-end-last-bin": "bin-end-middle-bin", "bin-end-middle-bin": "bin-end-last-bin"}.get(name.split("|")[0])
                if swap:
                    moved = [list(x) for x in c.planted]
                    moved[bi][j] = (f, L, swap)
                    with pytest.raises(AssertionError):
                        plantbins.check_named_wide(c.wg, moved, c.ordered, c.rbits)
    if case.startswith("gt-max"):
        with pytest.raises(AssertionError):
            plantbins.check_named_wide(c.wg, [c.planted[1], c.planted[0], c.planted[2]], [c.ordered[1], c.ordered[0], c.ordered[2]], c.rbits)
        with pytest.raises(AssertionError):  # a name that is wanted and absent
            plantbins.check_named_wide(c.wg, c.planted, c.ordered, c.rbits, ["giant-run"])
        with pytest.raises(AssertionError):  # verify_wide: a planted bucket that is not a whole bucket
            plantbins.verify_wide(c.wg, c.ordered[0], c.k, c.rbits[0], 0, [(c.planted[0][0][0] + 1, c.planted[0][0][1], "x")])


def test_the_moves_cover_every_clause():
    seen = set()
    for case in ("w2-k55-4bins", "w3-k70", "giant-run-k55", "gt-max-k127"):
        seen |= {_clause_of(n) for n in plantbins.make_wide_case(_small(), case, env={}).names if ":" not in n}
    assert seen - _NO_CLAIM == set(_WIDE_MOVES), (sorted(seen - _NO_CLAIM - set(_WIDE_MOVES)), sorted(set(_WIDE_MOVES) - seen))
    every = set()
    for case in plantbins.WIDE_CASES:
        if case != "w2-k55-indirect-off":
            every |= {_clause_of(n) for n in plantbins.make_wide_case(_small(), case, env={}).names if ":" not in n}
    assert every == seen, sorted(every - seen)


def test_plan_for_agrees_with_the_emulated_library_on_one_bin_per_width():
    """the `indirect` counter, the other path counters and the giant counts of one small case per record width (2, 3, 4, 7, 8 words), in a child over the emulated host library"""
    code = ("import sys, numpy as np; sys.path.insert(0, 'tests'); from kmc_amd import capi; import test_gpu_parity as T; ctx = capi.Context((0,));"
            "[T._run_wide_case(ctx, c) for c in ('kff-k55', 'giant-odd-k74', 'kff-k124', 'w7-k200', 'w8-k256')]; print('PLAN-OK')")
    env = dict({k: v for k, v in os.environ.items() if k != "KMC_HIP_INDIRECT"}, KMC_HIP_LIB=emu.build_hostlib("small"), KMC_PLANT_GEOMETRY="small")
    r = subprocess.run([sys.executable, "-c", code], cwd=plantbins.ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "PLAN-OK" in r.stdout, (r.stdout + r.stderr)[-2000:]
