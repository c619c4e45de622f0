"""Bins with buckets of a CHOSEN length at a CHOSEN place — TEST INFRASTRUCTURE for the trust boundary between k_bucket_detect (arena_sort.hip.h) and
k_bucket_rank (bucket_sort.hip.h br_tile: a bucket beyond BR_MID records keeps the places it has and is never compared again, which is right only if the detector's
samples — one record per BD_STRIDE — found it and the arena put it in order first).

A bin image here holds one-word k-mers as super-k-mers of their own (e = 0: `[0][ceil(k/4) packed bytes]`, 4096 of them per pack), shuffled, so the record array after
the stable HBM passes holds every bucket in arrival order, never in key order. A "bucket" is the set of records that share the key bits above `rbits` (rbits_for: the
plan the host library makes). A PLANTED bucket has L records whose low bits come from a pool of 5 to 10 values; FILLER is runs of 1 to 5 copies of one k-mer, a bucket
each, counted out so that the next planted bucket starts where it is wanted. Everything the helper claims about where a bucket lies it checks on np.sort of what it built
(verify), never on anything the library reports."""
from __future__ import annotations

import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACK_SUPERKMERS = 4096


# ------------------------------------------------------------------------------------------------ geometry
class Geometry:
    def __init__(self, MID, DS, THREADS, SLACK_DIV, name):
        self.MID, self.DS, self.THREADS, self.name = MID, DS, THREADS, name
        self.CAP = THREADS * 8                      # BrCfg<1>::CAP
        self.S = self.CAP - self.CAP // SLACK_DIV   # BrCfg<1>::STRIDE: the window
        self.BLOCK = 64 * DS                        # records one wave of k_bucket_detect samples
        assert self.MID + 1 >= 2 * self.DS, "the library's own static_assert"

    def __repr__(self):
        return f"Geometry({self.name}: MID={self.MID} DS={self.DS} CAP={self.CAP} S={self.S})"


def _header_defaults():
    with open(os.path.join(ROOT, "kmc_amd", "csrc", "bucket_sort.hip.h")) as f:
        text = f.read()
    out = {}
    for name in ("BR_MID", "BD_STRIDE_N", "BR_THREADS", "BR_SLACK_DIV"):
        m = re.findall(r"^#define\s+%s\s+(\d+)" % name, text, flags=re.M)
        assert len(m) == 1, f"{name}: expected one #define default in bucket_sort.hip.h, found {len(m)}"
        out[name] = int(m[0])
    return out


def geometry_of(backend_kind: int, lib_path: str = "", env=os.environ) -> Geometry:
    """backend 0 (the GPU library): the #define defaults of bucket_sort.hip.h. Backend 1 (the emulated host library): emu.GEOMETRY_FLAGS[name] over those defaults, the
    name from KMC_PLANT_GEOMETRY or from the library's file name (libkmc_hip_emu_<name>.so). Anything else is an error: a sweep that does not know the grid proves nothing."""
    d = _header_defaults()
    name = "device"
    if backend_kind == 1:
        import emu

        name = env.get("KMC_PLANT_GEOMETRY") or ""
        if not name:
            m = re.fullmatch(r"libkmc_hip_emu_(\w+)\.so", os.path.basename(lib_path or ""))
            assert m, f"cannot tell the geometry of the emulated library {lib_path!r}: set KMC_PLANT_GEOMETRY"
            name = m.group(1)
        assert name in emu.GEOMETRY_FLAGS, name
        for flag in emu.GEOMETRY_FLAGS[name]:
            m = re.fullmatch(r"-D(\w+)=(\d+)", flag)
            if m and m.group(1) in d:
                d[m.group(1)] = int(m.group(2))
    else:
        assert backend_kind == 0, f"backend kind {backend_kind}: neither the GPU library nor the emulated host library"
    return Geometry(d["BR_MID"], d["BD_STRIDE_N"], d["BR_THREADS"], d["BR_SLACK_DIV"], name)


def rbits_for(k: int, n_bins: int, n_records: int, geo: Geometry) -> int:
    """Key bits below the bucket bits for a group of `n_bins` non-empty bins of one-word k-mers: plan_sort of host_plan_and_groups.hip.h restated (default mode). Raises
    where the group would take LSD passes over every byte. The sweep's counter assertions (rank_count rises, lsd does not; the giant counts are exact, and a planted bucket
    of CAP + 1 records is a giant one only if the bucket bits are what this says) check the restatement."""
    tag_bits = 0
    while (1 << tag_bits) < n_bins:
        tag_bits += 1
    key_bits = 2 * k + tag_bits
    assert k <= 32 and key_bits <= 64, "one-word records only"
    key_bytes = (key_bits + 7) // 8
    spare = 8 * key_bytes - key_bits
    assert n_records > geo.THREADS * 8, "a tiny group takes plain LSD passes"
    h = 1
    while h + 2 <= key_bytes and h <= 6:
        eff = 8 * h - spare if 8 * h > spare else 0
        if eff >= 28 and (eff >= 63 or (n_records >> eff) <= 2) and key_bits - eff <= 48:
            return key_bits - eff
        h += 1
    raise AssertionError(f"k={k}, {n_bins} bins: no rank plan")


# ------------------------------------------------------------------------------------------------ k-mers
def revcomp(v: np.ndarray, k: int) -> np.ndarray:
    v = v.astype(np.uint64)
    x = ~v
    for sh, m in ((2, 0x3333333333333333), (4, 0x0F0F0F0F0F0F0F0F), (8, 0x00FF00FF00FF00FF), (16, 0x0000FFFF0000FFFF)):
        m = np.uint64(m)
        x = ((x >> np.uint64(sh)) & m) | ((x & m) << np.uint64(sh))
    x = (x >> np.uint64(32)) | (x << np.uint64(32))
    return x >> np.uint64(64 - 2 * k)


def canonical(v: np.ndarray, k: int) -> np.ndarray:
    return np.minimum(v, revcomp(v, k))


def image_of(kmers: np.ndarray, k: int):
    """(image, n_rec, pack_bytes, None): every k-mer a super-k-mer with e = 0, in the order given"""
    n = kmers.size
    nb = (k + 3) // 4
    be = (kmers.astype(np.uint64) << np.uint64(8 * nb - 2 * k)).astype(">u8").view(np.uint8).reshape(n, 8)
    img = np.zeros((n, 1 + nb), dtype=np.uint8)
    img[:, 1:] = be[:, 8 - nb:]
    n_packs = (n + PACK_SUPERKMERS - 1) // PACK_SUPERKMERS
    packs = np.full(n_packs, PACK_SUPERKMERS * (1 + nb), dtype=np.uint64)
    if n_packs:
        packs[-1] = (n - (n_packs - 1) * PACK_SUPERKMERS) * (1 + nb)
    return img.reshape(-1), n, packs, None


# ------------------------------------------------------------------------------------------------ one bin
class Bin:
    """records are added in KEY order (bucket after bucket); build() gives the shuffled image"""

    def __init__(self, geo: Geometry, k: int, rbits: int, rng, both_strands: int = 0):
        self.geo, self.k, self.rbits, self.rng, self.both = geo, k, rbits, rng, both_strands
        self.pos = 0
        self.lens, self.lows = [], []  # per bucket: its length; per record: its low bits
        self.planted = []              # (first, L, name)

    def _low(self, n):
        v = self.rng.integers(0, 1 << self.rbits, size=n, dtype=np.uint64)
        if self.both:  # the k-mer is its own canonical form: first symbol A (bucket numbers, build), last symbol not T
            v = (v & ~np.uint64(3)) | self.rng.integers(0, 3, size=n, dtype=np.uint64)
        return v

    def fill(self, count: int):
        """`count` records of filler: runs of 1 to 5 copies of one k-mer, every run a bucket of its own"""
        assert count >= 0
        if count == 0:
            return
        runs = self.rng.integers(1, 6, size=count)
        cs = np.cumsum(runs)
        m = int(np.searchsorted(cs, count)) + 1
        runs = runs[:m].copy()
        runs[-1] -= int(cs[m - 1]) - count
        self.lens.append(runs.astype(np.int64))
        self.lows.append(np.repeat(self._low(m), runs))
        self.pos += count

    def fill_to(self, position: int):
        assert position >= self.pos, (position, self.pos)
        self.fill(position - self.pos)

    def plant(self, L: int, name: str = "", lows: np.ndarray | None = None):
        """a bucket of L records at the bin's current end; returns its first record"""
        if lows is None:
            pool = self._low(int(self.rng.integers(5, 11)))
            lows = pool[self.rng.integers(0, pool.size, size=L)]
        assert lows.size == L
        first = self.pos
        self.lens.append(np.array([L], dtype=np.int64))
        self.lows.append(lows.astype(np.uint64))
        self.planted.append((first, L, name))
        self.pos += L
        return first

    def plant_at(self, first: int, L: int, name: str = "", lows=None):
        self.fill_to(first)
        return self.plant(L, name, lows)

    def plant_at_residue(self, s: int, L: int, name: str = ""):
        self.fill((s - self.pos) % self.geo.DS)
        return self.plant(L, name)

    def next_window(self, margin: int = 0) -> int:
        """the first window that starts at or behind the bin's end + margin"""
        return -(-(self.pos + margin) // self.geo.S)

    def next_block(self, margin: int = 0) -> int:
        """the first detect block m >= 1 whose seam placements (from m BLOCK - 2 DS on) lie at or behind the bin's end + margin"""
        return max(1, -(-(self.pos + margin + 2 * self.geo.DS) // self.geo.BLOCK))

    def build(self):
        """-> (bin tuple for _run_batch / O.process_bin, planted [(first, L, name)], ordered records): shuffled image; geometry verified on np.sort"""
        lens = np.concatenate(self.lens)
        lows = np.concatenate(self.lows)
        nb = lens.size
        bits = 2 * self.k - self.rbits - (2 if self.both else 0)
        gmax = max(1, min(1 << 20, ((1 << bits) - 1) // (nb + 1)))
        ids = np.cumsum(self.rng.integers(1, gmax + 1, size=nb, dtype=np.int64)).astype(np.uint64)
        assert int(ids[-1]) < (1 << bits)
        kmers = (np.repeat(ids, lens) << np.uint64(self.rbits)) | lows
        assert kmers.size == self.pos
        if self.both:
            assert np.array_equal(canonical(kmers, self.k), kmers)
            flip = self.rng.random(kmers.size) < 0.5
            kmers = np.where(flip, revcomp(kmers, self.k), kmers)
        kmers = kmers[self.rng.permutation(kmers.size)]
        ordered = verify(self.geo, kmers, self.k, self.rbits, self.both, self.planted)
        return image_of(kmers, self.k), list(self.planted), ordered


def verify(geo, kmers, k, rbits, both, planted):
    """On np.sort of the records (canonicalised first for both strands): every planted (first, L) is a whole bucket, no other bucket is longer than BR_MID, and no planted
    bucket arrives in key order. Returns the ordered records."""
    recs = canonical(kmers, k) if both else kmers
    ordered = np.sort(recs)
    bucket = ordered >> np.uint64(rbits)
    n = ordered.size
    starts = np.flatnonzero(np.concatenate([[True], bucket[1:] != bucket[:-1]]))
    blen = np.diff(np.concatenate([starts, [n]]))
    want = {f: L for f, L, _ in planted}
    assert len(want) == len(planted)
    idx = np.searchsorted(starts, np.array(sorted(want), dtype=np.int64))
    assert np.array_equal(starts[idx], np.array(sorted(want))), "a planted bucket does not start where it was planted"
    assert np.array_equal(blen[idx], np.array([want[f] for f in sorted(want)])), "a planted bucket is not a whole bucket of its length"
    big = np.flatnonzero(blen > geo.MID)
    assert set(starts[big].tolist()) <= set(want), "filler made a bucket beyond BR_MID"
    assert blen[np.setdiff1d(np.arange(starts.size), idx)].max(initial=0) <= 5
    # arrival order (the HBM passes are stable): the records of a bucket in image order
    arrival = recs[np.argsort(recs >> np.uint64(rbits), kind="stable")]
    for f, L, _ in planted:
        a = arrival[f:f + L]
        assert np.any(a[1:] < a[:-1]), ("a planted bucket arrives in order", f, L)
    return ordered


def bucket_starts(ordered, rbits):
    b = ordered >> np.uint64(rbits)
    return np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))


def tile_of(geo, starts, n, w):
    """[b0, b1) of window w as k_bucket_bounds cuts it: from the first bucket start in the window to the first one behind it"""
    i0, i1 = np.searchsorted(starts, w * geo.S), np.searchsorted(starts, (w + 1) * geo.S)
    return (int(starts[i0]) if i0 < starts.size else n), (int(starts[i1]) if i1 < starts.size else n)


def chunk_cut(geo, starts, b0, b1):
    """where br_tile cuts a tile that outgrows the capacity: the last bucket start in (b0, b0 + CAP]; None if the tile fits"""
    if b1 - b0 <= geo.CAP:
        return None
    i = np.searchsorted(starts, b0 + geo.CAP, side="right") - 1
    return int(starts[i])


def n_samples(geo, first, L):
    return (first + L - 1) // geo.DS - (first + geo.DS - 1) // geo.DS + 1


# ------------------------------------------------------------------------------------------------ plans
def finish_group(bins):
    """[Bin] -> (bins for _run_batch, [[(first, L, name)] per bin], [ordered records per bin])"""
    built = [b.build() for b in bins]
    return [x[0] for x in built], [x[1] for x in built], [x[2] for x in built]


def sweep(geo, k, n_bins, lengths, seed, both_strands=0, split_residues=False):
    """every length of `lengths` at every start residue 0 .. DS-1 of the sample grid, dealt out over `n_bins` bins (whole lengths, or — split_residues — the residues of
    every length); two planted buckets back to back at the end of bin 0 (and wherever L = 1 mod DS). Asserts the cover on the verified geometry."""
    rng = np.random.default_rng(seed)
    est = sum(geo.DS * (L + geo.DS // 2) for L in lengths) + n_bins * geo.CAP
    rb = rbits_for(k, n_bins, est, geo)
    bins = [Bin(geo, k, rb, rng, both_strands) for _ in range(n_bins)]
    for i, b in enumerate(bins):
        b.fill(int(rng.integers(1, 2 * geo.DS)))
        for j, L in enumerate(lengths):
            order = rng.permutation(geo.DS) if j % 2 else np.arange(geo.DS)
            for s in order:
                if (int(s) % n_bins == i) if split_residues else (j % n_bins == i):
                    b.plant_at_residue(int(s), L, "sweep")
        b.fill(int(rng.integers(geo.DS, 3 * geo.DS)))
    bins[0].plant(geo.MID + 1, "back-to-back")
    bins[0].plant(geo.MID + 2, "back-to-back")
    bins[0].fill(int(rng.integers(geo.DS, 3 * geo.DS)))
    for b in bins:
        if b.pos <= geo.CAP:
            b.fill(geo.CAP + 1 + int(rng.integers(0, geo.DS)) - b.pos)
    out, planted, ordered = finish_group(bins)
    for L in lengths:
        seen = {f % geo.DS for pl in planted for f, l, name in pl if l == L and name == "sweep"}
        assert seen == set(range(geo.DS)), (L, sorted(set(range(geo.DS)) - seen))
    assert any(a[0] + a[1] == b[0] for pl in planted for a, b in zip(pl, pl[1:])), "no two planted buckets back to back"
    return out, planted, ordered, rb


def _seams_and_windows(geo, b, L1, L2):
    """the named placements that need no particular bin: detect-block seams, window seams, chunked tiles, the giant boundary"""
    DS, S, CAP, MID, BLOCK = geo.DS, geo.S, geo.CAP, geo.MID, geo.BLOCK
    for L in (L1, L2):
        m = b.next_block(5)
        b.plant_at(m * BLOCK - 2 * DS + 1, L, "seam-low")   # samples: lane 63 of block m - 1, lane 0 of block m (edge_n finds the pair)
        m = b.next_block(5)
        b.plant_at(m * BLOCK - DS, L, "seam-high")
        m = b.next_block(5)
        b.plant_at(m * BLOCK - DS + 1, L, "first-sample-lane0-low")  # first sample: lane 0 of block m (edge_p says that nothing of it lies in front)
        m = b.next_block(5 + DS)
        b.plant_at(m * BLOCK, L, "first-sample-lane0-high")
        w = b.next_window(5)
        b.plant_at((w + 1) * S - L // 2, L, "window-seam")
    # chunked tiles: a bucket start on the window's first record, a trusted bucket so late in the window that the tile outgrows the capacity
    for L in sorted({max(MID + 1, CAP - S + 20), CAP // 2}):
        w = b.next_window(5)
        b.fill_to(w * S)
        b.plant_at((w + 1) * S - 5, L, "chunk1-is-the-trusted-bucket")
    w = b.next_window(5)
    b.plant_at(w * S, L1, "trusted-bucket-on-the-windows-first-record")
    b.plant_at((w + 1) * S - 5, CAP // 2, "chunk1-is-the-trusted-bucket")
    if CAP - S + 10 <= MID:  # a second chunk is ONE bucket of more than CAP - S records: an untrusted one exists only where CAP - S < BR_MID (not in the product's geometry)
        w = b.next_window(5 + L1)
        b.fill_to(w * S)
        b.plant_at((w + 1) * S - 5 - L2, L2, "trusted-bucket-ends-chunk0")
        b.plant(CAP - S + 10, "untrusted-chunk1")
    # the giant boundary: CAP (the longest bucket that goes back into its tile) and CAP + 1 (the shortest that is counted from the arena), on a window's first and last record
    for L in (CAP, CAP + 1):
        w = b.next_window(5)
        b.plant_at(w * S, L, "giant-boundary-window-first")
        w = b.next_window(5)
        b.plant_at(w * S + S - 1, L, "giant-boundary-window-last")


def edges(geo, k, seed):
    """Three bins in one group. Bin 0: a bucket on the bin's first record, then every seam placement at L = MID+1 / MID+2. Bin 1 (a middle bin): the same with the two
    lengths swapped, and a bucket that ends the bin. Bin 2 (the last bin): a bucket that ends the bin (and the group)."""
    rng = np.random.default_rng(seed)
    L1, L2 = geo.MID + 1, geo.MID + 2
    rb = rbits_for(k, 3, 8 * geo.BLOCK, geo)
    bins = [Bin(geo, k, rb, rng) for _ in range(3)]
    bins[0].plant_at(0, L1, "bin-start")
    _seams_and_windows(geo, bins[0], L1, L2)
    bins[0].fill(int(rng.integers(geo.DS, 3 * geo.DS)))
    bins[1].plant_at(0, L2, "bin-start")
    _seams_and_windows(geo, bins[1], L2, L1)
    bins[1].fill(int(rng.integers(1, geo.DS)))
    bins[1].plant(L1, "bin-end-middle-bin")
    bins[2].fill(geo.CAP + int(rng.integers(1, geo.DS)))
    for L in (L1, L2):
        m = bins[2].next_block(5)
        bins[2].plant_at(m * geo.BLOCK - 2 * geo.DS + 1, L, "seam-low")
    bins[2].fill(int(rng.integers(1, geo.DS)))
    bins[2].plant(L2, "bin-end-last-bin")
    out, planted, ordered = finish_group(bins)
    check_named(geo, planted, ordered, rb)
    return out, planted, ordered, rb


def short_last_bin(geo, k, seed):
    """two full-size bins and a last bin shorter than BD_STRIDE records (its only sample is record 0; it has no block of its own beyond the first)"""
    rng = np.random.default_rng(seed)
    L1, L2 = geo.MID + 1, geo.MID + 2
    rb = rbits_for(k, 3, 4 * geo.CAP, geo)
    bins = [Bin(geo, k, rb, rng) for _ in range(3)]
    for b, (La, Lb) in zip(bins[:2], ((L1, L2), (L2, L1))):
        b.plant_at(0, La, "bin-start")
        b.fill(geo.CAP + int(rng.integers(1, geo.DS)))
        for s in (0, 1, geo.DS - 1):
            b.plant_at_residue(s, Lb, "sweep")
        b.fill(int(rng.integers(1, geo.DS)))
        b.plant(La, "bin-end-middle-bin")
    bins[2].fill(geo.DS - 1 - int(rng.integers(0, geo.DS // 2)))
    out, planted, ordered = finish_group(bins)
    assert 0 < out[2][1] < geo.DS and all(o[1] > geo.CAP for o in out[:2])
    check_named(geo, planted, ordered, rb, want=("bin-start", "bin-end-middle-bin"))
    return out, planted, ordered, rb


def giant_run(geo, k, seed):
    """One giant bucket over several windows (five segments in k_arena_finish) in which ONE k-mer is repeated from in front of the second segment to behind the third: its
    count reaches back over two segment boundaries. The caller sets cutoff_max below that count (the run is dropped, a tally) and counter_max = 255 below the count of a
    second k-mer (clamped). Returns also (length of the long run, length of the second)."""
    rng = np.random.default_rng(seed)
    S, CAP = geo.S, geo.CAP
    rb = rbits_for(k, 2, 8 * S, geo)
    bins = [Bin(geo, k, rb, rng) for _ in range(2)]
    b = bins[0]
    b.fill(CAP + int(rng.integers(1, geo.DS)))
    w = b.next_window(5)
    first, L = w * S + 50, 3 * S + 100
    n_seg = 2 * (((first + L - 1) // S) - w) - 1
    assert n_seg == 5
    lo_n, run = L // n_seg - 30, (2 * L) // n_seg + 30 - (L // n_seg - 30)
    second = 300
    X, Y = np.uint64(1 << (rb - 1)), np.uint64((1 << (rb - 1)) + 12345)
    below = rng.integers(0, int(X), size=lo_n, dtype=np.uint64)
    above = rng.integers(int(Y) + 1, 1 << rb, size=L - lo_n - run - second, dtype=np.uint64)
    lows = np.concatenate([below, np.full(run, X), np.full(second, Y), above])
    b.plant_at(first, L, "giant-run", lows=lows)
    b.fill(CAP)
    bins[1].fill(CAP + 77)
    bins[1].plant(geo.MID + 1, "sweep")
    bins[1].fill(geo.DS)
    out, planted, ordered = finish_group(bins)
    o = ordered[0][first:first + L]
    for s in (1, 2):  # the run covers the records on both sides of two segment boundaries (segment s starts at L s / n_seg: k_arena_finish)
        cut = L * s // n_seg
        assert o[cut - 1] == o[cut] == o[lo_n] and lo_n < cut < lo_n + run
    assert o[lo_n - 1] != o[lo_n] and o[lo_n + run] != o[lo_n] and run > 2 * second > 2 * 255
    return out, planted, ordered, rb, run, second


def check_named(geo, planted, ordered, rbits, want=None):
    """every named placement is present and IS what its name says — decided on the ordered records"""
    DS, S, CAP, MID, BLOCK = geo.DS, geo.S, geo.CAP, geo.MID, geo.BLOCK
    names = set()
    for pl, o in zip(planted, ordered):
        n = o.size
        starts = bucket_starts(o, rbits)
        for f, L, name in pl:
            names.add((name, L))
            m = -(-f // BLOCK)  # the first block seam at or behind the bucket's first record
            w = f // S
            b0, b1 = tile_of(geo, starts, n, w)
            cut = chunk_cut(geo, starts, b0, b1)
            if name == "bin-start":
                assert f == 0
            elif name.startswith("bin-end"):
                assert f + L == n and ((n - 1) // DS) * DS >= f, "the bin's last sample lies inside the bucket"
            elif name == "seam-low":
                assert m >= 1 and f == m * BLOCK - 2 * DS + 1 and f + L > m * BLOCK
            elif name == "seam-high":
                assert m >= 1 and f == m * BLOCK - DS and f + L > m * BLOCK
                assert L != 2 * DS or n_samples(geo, f, L) == 2
            elif name == "first-sample-lane0-low":
                assert m >= 1 and f == m * BLOCK - DS + 1 and f + L > m * BLOCK + DS
            elif name == "first-sample-lane0-high":
                assert f >= BLOCK and f % BLOCK == 0
            elif name == "window-seam":
                assert f // S + 1 == (f + L - 1) // S
            elif name == "chunk1-is-the-trusted-bucket":
                assert MID < L <= CAP and cut == f and b1 == f + L and cut > b0, (f, L, b0, b1, cut)
            elif name == "trusted-bucket-on-the-windows-first-record":
                assert f == w * S == b0 and cut is not None and cut > f + L
            elif name == "trusted-bucket-ends-chunk0":
                assert cut == f + L and b1 - cut <= MID and b1 - b0 > CAP
            elif name == "untrusted-chunk1":
                assert cut == f and L <= MID and b1 == f + L
            elif name == "giant-boundary-window-first":
                assert f % S == 0 and (L <= CAP or (f + L - 1) // S == w + 1)  # CAP + 1: one segment
            elif name == "giant-boundary-window-last":
                assert f % S == S - 1 and (f + L - 1) // S == w + 2            # CAP + 1: three segments; CAP: the whole second chunk of its tile
                assert L > CAP or (cut == f and b1 == f + L)
    L1, L2 = MID + 1, MID + 2
    if want is None:
        want = ["bin-start", "bin-end-middle-bin", "bin-end-last-bin", "seam-low", "seam-high", "first-sample-lane0-low", "first-sample-lane0-high", "window-seam",
                "trusted-bucket-on-the-windows-first-record"]
        for nm in ("giant-boundary-window-first", "giant-boundary-window-last"):
            assert (nm, CAP) in names and (nm, CAP + 1) in names, nm
        assert any(nm == "chunk1-is-the-trusted-bucket" for nm, _ in names)
        if CAP - S + 10 <= MID:
            assert ("trusted-bucket-ends-chunk0", L1) in names or ("trusted-bucket-ends-chunk0", L2) in names
            assert any(nm == "untrusted-chunk1" for nm, _ in names)
        for nm in want:
            if nm.startswith("bin-end") or nm == "trusted-bucket-on-the-windows-first-record":
                assert (nm, L1) in names or (nm, L2) in names, nm
            else:
                assert (nm, L1) in names and (nm, L2) in names, nm
    else:
        for nm in want:
            assert (nm, L1) in names and (nm, L2) in names, nm


def n_giant(geo, planted):
    g = [L for pl in planted for _, L, _ in pl if L > geo.CAP]
    return len(g), sum(g)


# ------------------------------------------------------------------------------------------------ the cases of the sweep
CASES = ("sweep-k27", "edges-k27", "short-last-bin-k27", "giant-run-k27", "k32", "k25-many-bins", "k21", "both-strands", "kff", "without-output")


def sweep_lengths(geo, device: bool):
    MID, DS, CAP = geo.MID, geo.DS, geo.CAP
    ls = (list(range(MID - 11, MID + 15)) if device else [MID, MID + 1, MID + 2]) + [DS, DS + 1, 2 * DS - 1, 2 * DS, CAP, CAP + 1]
    if not device:
        ls.remove(DS + 1)
    return list(dict.fromkeys(ls))


def make_case(geo, case: str, device: bool):
    """-> (k, parameters of capi.make_params, bins, planted, ordered records per bin, rbits)"""
    seed = 1000 + CASES.index(case)
    one = [geo.MID + 1]
    if case == "sweep-k27":
        return (27, dict(lut_prefix_len=3, both_strands=0)) + sweep(geo, 27, 4 if device else 3, sweep_lengths(geo, device), seed)
    if case == "edges-k27":
        return (27, dict(lut_prefix_len=3, both_strands=0)) + edges(geo, 27, seed)
    if case == "short-last-bin-k27":
        return (27, dict(lut_prefix_len=3, both_strands=0)) + short_last_bin(geo, 27, seed)
    if case == "giant-run-k27":
        out, planted, ordered, rb, run, second = giant_run(geo, 27, seed)
        assert second > 255
        return 27, dict(lut_prefix_len=3, both_strands=0, cutoff_max=(run + second) // 2, counter_max=255), out, planted, ordered, rb
    if case == "k32":  # 32 key bits below the passes, 64-bit pairs in the tiles, a group of one bin
        return (32, dict(lut_prefix_len=4, both_strands=0)) + sweep(geo, 32, 1, one, seed)
    if case == "k25-many-bins":  # 9 to 16 bins in one group: the bin's tag rides above the bucket bits
        return (25, dict(lut_prefix_len=1, both_strands=0)) + sweep(geo, 25, 16 if device else 9, one, seed, split_residues=True)
    if case == "k21":
        return (21, dict(lut_prefix_len=1, both_strands=0)) + sweep(geo, 21, 3, one, seed, split_residues=True)
    if case == "both-strands":
        return (27, dict(lut_prefix_len=3, both_strands=1)) + sweep(geo, 27, 2, one, seed, both_strands=1, split_residues=True)
    if case == "kff":
        return (27, dict(lut_prefix_len=0, output_type=1, both_strands=0)) + sweep(geo, 27, 2, one, seed, split_residues=True)
    if case == "without-output":
        return (27, dict(lut_prefix_len=3, without_output=1, both_strands=0)) + sweep(geo, 27, 2, one, seed, split_residues=True)
    raise KeyError(case)


def locate(geo, planted_of_bin, ordered, kmer_index, cutoff_min, cutoff_max):
    """the planted bucket (first, L, name, residue) that holds — or, failing that, lies nearest in front of — the `kmer_index`-th COUNTED k-mer of a bin: where a difference
    in the output records points to"""
    uniq, first_at, counts = np.unique(ordered, return_index=True, return_counts=True)
    kept = first_at[(counts >= cutoff_min) & (counts <= cutoff_max)]
    if kmer_index >= kept.size:
        return ("behind the last counted k-mer", kmer_index, int(kept.size))
    pos = int(kept[kmer_index])
    best = None
    for f, L, name in planted_of_bin:
        if f <= pos:
            best = dict(first=f, len=L, name=name, residue=f % geo.DS, holds_it=pos < f + L, record=pos)
    return best
