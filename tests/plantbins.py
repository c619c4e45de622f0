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
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACK_SUPERKMERS = 4096


# ------------------------------------------------------------------------------------------------ geometry
class Geometry:
    def __init__(self, MID, DS, THREADS, SLACK_DIV, name, GT_THREADS=1024, GT_MAX_LOG2=20, BIG=128):
        self.MID, self.DS, self.THREADS, self.name = MID, DS, THREADS, name
        self.SLACK_DIV, self.GT_THREADS, self.GT_MAX, self.BIG = SLACK_DIV, GT_THREADS, 1 << GT_MAX_LOG2, BIG
        self.CAP = THREADS * 8                      # BrCfg<1>::CAP
        self.S = self.CAP - self.CAP // SLACK_DIV   # BrCfg<1>::STRIDE: the window
        self.BLOCK = 64 * DS                        # records one wave of k_bucket_detect samples
        assert self.MID + 1 >= 2 * self.DS, "the library's own static_assert"

    def wide(self, size):
        """the geometry records of `size` words (two and more) see: BrCfg<SIZE> and k_giant_tiles<SIZE> of bucket_sort.hip.h"""
        return WideGeometry(self, size)

    def __repr__(self):
        return f"Geometry({self.name}: MID={self.MID} DS={self.DS} CAP={self.CAP} S={self.S})"


def _header_defaults():
    with open(os.path.join(ROOT, "kmc_amd", "csrc", "bucket_sort.hip.h")) as f:
        text = f.read()
    out = {}
    for name in ("BR_MID", "BD_STRIDE_N", "BR_THREADS", "BR_SLACK_DIV", "GT_THREADS", "GT_MAX_RECORDS_LOG2", "BR_BIG"):
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
    return Geometry(d["BR_MID"], d["BD_STRIDE_N"], d["BR_THREADS"], d["BR_SLACK_DIV"], name, d["GT_THREADS"], d["GT_MAX_RECORDS_LOG2"], d["BR_BIG"])


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


# ================================================================================================ records of two words and more (k >= 33)
# No arena: k_bucket_rank<2> ranks split (A, B) pairs, k_bucket_rank<3..> whole records through br_rank_add_less; a bucket beyond the capacity goes to k_giant_tiles, one
# beyond GT_MAX_RECORDS sends its bin back. Records are (n, SIZE) uint64 arrays, word 0 the least significant, as the library's records are. Everything below follows the
# rule of the one-word half: where a bucket lies is decided on a sort of what was built (np.lexsort over the words), never on anything the library reports.
M64 = (1 << 64) - 1
GRP_MAX = 16


class WideGeometry:
    """BrCfg<SIZE> and k_giant_tiles<SIZE> for SIZE >= 2, from the same #defines as Geometry"""

    def __init__(self, geo: Geometry, size: int):
        assert size >= 2
        self.base, self.size, self.name = geo, size, geo.name
        self.ITEMS = 4 if size == 2 else 2           # rows of 64 records per wave
        self.WAVE = 64 * self.ITEMS                  # records a wave owns
        self.CAP = geo.THREADS * self.ITEMS          # BrCfg<SIZE>::CAP
        self.S = self.CAP - self.CAP // geo.SLACK_DIV
        self.GT_CHUNK = geo.GT_THREADS * self.ITEMS  # records k_giant_tiles takes per round
        self.GT_MAX, self.BIG = geo.GT_MAX, geo.BIG
        assert self.BIG + 1 < self.S - 8 and self.CAP < self.GT_CHUNK <= self.GT_MAX // 2

    def __repr__(self):
        return f"Geometry({self.name}: SIZE={self.size} CAP={self.CAP} S={self.S} BIG={self.BIG} GT_CHUNK={self.GT_CHUNK} GT_MAX={self.GT_MAX})"


def words_of(k: int) -> int:
    return (k + 31) // 32


def group_sizes(k: int, n_bins: int):
    """how kmc_hip_process_bins_device (one stream, small bins) deals `n_bins` bins out over sort groups: group_capacity of host_plan_and_groups.hip.h restated"""
    room = 64 * words_of(k) - 2 * k
    G = min(1 << min(room, 4), GRP_MAX)
    return [min(G, n_bins - i) for i in range(0, n_bins, G)]


def plan_for(k: int, n_bins: int, n_records: int, geo: Geometry, out_rec_bytes: int = 0, env=os.environ):
    """(rbits, n_pass, indirect) of a group of `n_bins` non-empty bins of records of two words and more: plan_sort<SIZE> and the `indirect` condition of run_group_device_t
    (host_plan_and_groups.hip.h) restated — br_rem_limit, the `eff >= 28` rule, INDIRECT_MIN_WORDS = 2, four passes, KMC_HIP_INDIRECT. Raises where the group would take LSD
    passes over every byte. rbits is a multiple of 8 (the passes are whole bytes from the key's top down to byte `key_bytes - n_pass`): 56, 64, 72, 80 for two words, never 65
    or 79. (Two mutants of the issue are equivalent BECAUSE of that — see tests/README.md: `passes = nbits / 8` in k_giant_tiles, for one; the equivalence ends the day plan_sort
    leaves a partial byte below the passes, and this function's `assert rbits == 8 * (key_bytes - top)` then fails first.) The sweep's exact counters (rank_count, indirect, lsd, the giant counts — a bucket of CAP + 1 is a giant one only if the bucket bits are these) check this."""
    size = words_of(k)
    assert size >= 2, "one-word records: rbits_for"
    wg = geo.wide(size)
    tag_bits = 0
    while (1 << tag_bits) < n_bins:
        tag_bits += 1
    key_bits = 2 * k + tag_bits
    assert key_bits <= 64 * size, "group too large for the record width"
    key_bytes = (key_bits + 7) // 8
    spare = 8 * key_bytes - key_bits
    rem_limit = 80 if size == 2 else 64 * size
    assert out_rec_bytes <= 8 * size, "a counted record longer than the record it was counted from: not counted in place (count_applicable), LSD passes"
    assert n_records > geo.THREADS * max(8 // size, 2), "a tiny group takes plain LSD passes"
    top = None
    h = 1
    while h + 2 <= key_bytes and h <= 6:
        eff = 8 * h - spare if 8 * h > spare else 0
        if eff >= 28 and (eff >= 63 or (n_records >> eff) <= 2) and key_bits - eff <= rem_limit:
            top = h
            break
        h += 1
    assert top is not None and 8 * top - spare <= 48, f"k={k}, {n_bins} bins: no rank plan"
    rbits = key_bits - (8 * top - spare)
    assert rbits == 8 * (key_bytes - top)
    e = env.get("KMC_HIP_INDIRECT")
    enabled = e is None or (re.match(r"\s*[+-]?\d+", e) is not None and int(re.match(r"\s*[+-]?\d+", e).group(0)) != 0)
    return rbits, top, bool(enabled and top == 4 and 2 <= n_records < (1 << 32))


def giant_passes(rbits: int) -> int:
    """LSD passes k_giant_tiles takes over ONE bucket (first and last record share the bucket bits): odd = the ordered records end in U, even = in T"""
    return (rbits + 7) // 8


# ------------------------------------------------------------------------------------------------ multi-word k-mers
def to_words(values, size: int) -> np.ndarray:
    return np.array([[(int(v) >> (64 * w)) & M64 for w in range(size)] for v in values], dtype=np.uint64).reshape(len(values), size)


def to_ints(recs: np.ndarray):
    return [sum(int(x) << (64 * w) for w, x in enumerate(row)) for row in recs]


def symbols_of(recs: np.ndarray, k: int) -> np.ndarray:
    """(n, k) uint8, column j = symbol j counted from the k-mer's LAST symbol (bits 2j, 2j + 1)"""
    out = np.empty((recs.shape[0], k), dtype=np.uint8)
    for j in range(k):
        out[:, j] = (recs[:, (2 * j) // 64] >> np.uint64((2 * j) % 64)) & np.uint64(3)
    return out


def from_symbols(sym: np.ndarray, size: int) -> np.ndarray:
    out = np.zeros((sym.shape[0], size), dtype=np.uint64)
    for j in range(sym.shape[1]):
        out[:, (2 * j) // 64] |= sym[:, j].astype(np.uint64) << np.uint64((2 * j) % 64)
    return out


def revcomp_wide(recs: np.ndarray, k: int) -> np.ndarray:
    return from_symbols(3 - symbols_of(recs, k)[:, ::-1], recs.shape[1])


def order_of(recs: np.ndarray) -> np.ndarray:
    """stable ascending order of multi-word records"""
    return np.lexsort(tuple(recs[:, w] for w in range(recs.shape[1])))


def less_wide(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """row-wise a < b"""
    lt = np.zeros(a.shape[0], dtype=bool)
    for w in range(a.shape[1]):
        lt = (a[:, w] < b[:, w]) | ((a[:, w] == b[:, w]) & lt)
    return lt


def canonical_wide(recs: np.ndarray, k: int) -> np.ndarray:
    rc = revcomp_wide(recs, k)
    return np.where(less_wide(rc, recs)[:, None], rc, recs)


def bucket_words(recs: np.ndarray, rbits: int) -> np.ndarray:
    """the records with the `rbits` low bits cleared: equal rows = one bucket"""
    out = recs.copy()
    w, r = rbits // 64, rbits % 64
    out[:, :w] = 0
    if w < out.shape[1] and r:
        out[:, w] &= np.uint64(M64 ^ ((1 << r) - 1))
    return out


def bucket_starts_wide(ordered: np.ndarray, rbits: int) -> np.ndarray:
    b = bucket_words(ordered, rbits)
    return np.flatnonzero(np.concatenate([[True], np.any(b[1:] != b[:-1], axis=1)]))


def image_of_wide(recs: np.ndarray, k: int):
    """(image, n_rec, pack_bytes, None): every k-mer a super-k-mer of its own (e = 0, ceil(k/4) packed bytes, 4096 per pack), in the order given"""
    n, size = recs.shape
    nb = (k + 3) // 4
    pad = 8 * nb - 2 * k  # 0, 2, 4, 6: the packed bytes are the k-mer left-aligned; 8 nb <= 64 SIZE
    sh = recs.copy()
    if pad:
        sh = recs << np.uint64(pad)
        sh[:, 1:] |= recs[:, :-1] >> np.uint64(64 - pad)
    be = np.ascontiguousarray(sh[:, ::-1]).astype(">u8").view(np.uint8).reshape(n, 8 * size)
    img = np.zeros((n, 1 + nb), dtype=np.uint8)
    img[:, 1:] = be[:, 8 * size - nb:]
    n_packs = (n + PACK_SUPERKMERS - 1) // PACK_SUPERKMERS
    packs = np.full(n_packs, PACK_SUPERKMERS * (1 + nb), dtype=np.uint64)
    if n_packs:
        packs[-1] = (n - (n_packs - 1) * PACK_SUPERKMERS) * (1 + nb)
    return img.reshape(-1), n, packs, None


# ------------------------------------------------------------------------------------------------ planted low bits
def lows_generators(rbits: int, size: int):
    """the named generators a remainder of `rbits` bits admits"""
    nd = (rbits + 31) // 32  # dwords with bits below rbits
    gens = [f"one-dword-differs[{i}]" for i in range(nd)]
    spans = {(0, 0), (0, nd - 2), (1, 1), (1, nd - 2), (nd - 2, nd - 2), (0, nd // 2)}
    gens += [f"borrow-through[{i}..{j}]" for i, j in sorted(spans) if 0 <= i <= j <= nd - 2]
    gens += ["ties", "extremes"]
    if size == 2:
        gens.append("ab-split")
    return gens


def lows_values(gen: str, rbits: int, rng):
    """the distinct remainders (python integers below 2^rbits) of a generator:
    one-dword-differs[i]   one value and copies of it that differ in dword i alone
    borrow-through[i..j]   A: dwords i..j all ones; B = A with another dword 0 (i > 0: the compare's borrow travels through equal all-ones dwords); E = A with another dword
                           j + 1 (the mirror image: decided at the top, everything below equal); C = A + 2^(32 i): dwords i..j all zero against all ones, dword j + 1 one more
                           (x and x + 1 in units of dword i)
    ties                   3 to 7 unrelated values
    extremes               0, all ones, only bit 0, only bit rbits - 1
    ab-split               one value and copies that differ in bit 0 / 15 / 16 / 17 / 47 / 48 / 63 / 64 / rbits - 1 alone"""
    mask = (1 << rbits) - 1
    rnd = lambda bits: int.from_bytes(rng.bytes((bits + 7) // 8), "little") & ((1 << bits) - 1)
    width = lambda d: min(32, rbits - 32 * d)
    field = lambda v, d, x: (v & ~(((1 << width(d)) - 1) << (32 * d))) | (x << (32 * d))
    m = re.fullmatch(r"one-dword-differs\[(\d+)\]", gen)
    if m:
        i = int(m.group(1))
        assert 32 * i < rbits
        base, n = rnd(rbits), min(4, 1 << width(i))
        xs = set()
        while len(xs) < n:
            xs.add(rnd(width(i)))
        return [field(base, i, x) for x in sorted(xs)]
    m = re.fullmatch(r"borrow-through\[(\d+)\.\.(\d+)\]", gen)
    if m:
        i, j = int(m.group(1)), int(m.group(2))
        assert i <= j and 32 * (j + 1) < rbits
        t = rnd(width(j + 1)) % ((1 << width(j + 1)) - 1)  # not the field's maximum: t + 1 stays inside it
        A = field(rnd(rbits), j + 1, t)
        for d in range(i, j + 1):
            A = field(A, d, 0xFFFFFFFF)
        vals = [A]
        if i > 0:
            vals.append(field(A, 0, (A & 0xFFFFFFFF) ^ (1 + rnd(31))))
        vals.append(field(A, j + 1, t + 1 if t == 0 else t - 1))
        vals.append(A + (1 << (32 * i)))
        assert len(set(vals)) == len(vals) and max(vals) <= mask
        return vals
    if gen == "ties":
        return list({rnd(rbits) for _ in range(int(rng.integers(3, 8)))})
    if gen == "extremes":
        return [0, mask, 1, 1 << (rbits - 1)]
    if gen == "ab-split":
        base = rnd(rbits)
        return [base] + [base ^ (1 << b) for b in sorted({0, 15, 16, 17, 47, 48, 63, 64, rbits - 1}) if b < rbits]
    raise KeyError(gen)


def lows_named(gen: str, L: int, rbits: int, size: int, rng) -> np.ndarray:
    """(L, size) words: every value of the generator at least once, the rest drawn from them"""
    vals = lows_values(gen, rbits, rng)
    assert L >= 2 * len(vals), (gen, L)
    idx = rng.integers(0, len(vals), size=L)
    idx[:len(vals)] = np.arange(len(vals))
    return to_words(vals, size)[idx]


# ------------------------------------------------------------------------------------------------ one bin of wide records
class WideBin:
    """records are added in KEY order (bucket after bucket); build() gives the shuffled image. `gens`: names of lows generators dealt out in turn to the buckets planted
    through plant_named (forward strand only: a generator's values end in any symbol)."""

    def __init__(self, wg: WideGeometry, k: int, rbits: int, rng, both_strands: int = 0, gens=()):
        assert words_of(k) == wg.size and rbits < 2 * k
        self.geo, self.k, self.rbits, self.rng, self.both, self.size = wg, k, rbits, rng, both_strands, wg.size
        self.pos = 0
        self.lens, self.lows, self.planted = [], [], []
        self.gens, self.gen_at, self.used = ([] if both_strands else list(gens)), int(rng.integers(0, 1000)), set()

    def _low(self, n):
        v = self.rng.integers(0, 1 << 63, size=(n, self.size), dtype=np.uint64) * np.uint64(2) + self.rng.integers(0, 2, size=(n, self.size), dtype=np.uint64)
        v ^= bucket_words(v, self.rbits)
        if self.both:  # the k-mer is its own canonical form: first symbol A (bucket numbers, build), last symbol not T — its reverse complement then BEGINS with a symbol above A
            v[:, 0] = (v[:, 0] & np.uint64(M64 ^ 3)) | self.rng.integers(0, 3, size=n, dtype=np.uint64)
        return v

    def fill(self, count: int):
        assert count >= 0
        if count == 0:
            return
        runs = self.rng.integers(1, 6, size=count)
        cs = np.cumsum(runs)
        m = int(np.searchsorted(cs, count)) + 1
        runs = runs[:m].copy()
        runs[-1] -= int(cs[m - 1]) - count
        self.lens.append(runs.astype(np.int64))
        self.lows.append(np.repeat(self._low(m), runs, axis=0))
        self.pos += count

    def fill_to(self, position: int):
        assert position >= self.pos, (position, self.pos)
        self.fill(position - self.pos)

    def plant(self, L: int, name: str = "", lows=None):
        if lows is None:
            pool = self._low(int(self.rng.integers(5, 11)))
            lows = pool[self.rng.integers(0, pool.shape[0], size=L)]
        assert lows.shape == (L, self.size)
        first = self.pos
        self.lens.append(np.array([L], dtype=np.int64))
        self.lows.append(lows.astype(np.uint64))
        self.planted.append((first, L, name))
        self.pos += L
        return first

    def plant_at(self, first: int, L: int, name: str = "", lows=None):
        self.fill_to(first)
        return self.plant(L, name, lows)

    def plant_named(self, first, L: int, place: str, gen=None):
        """a bucket at `first` (None: the bin's end) whose low bits come from the next lows generator in turn (or `gen`); the name is `place|generator`"""
        if first is not None:
            self.fill_to(first)
        if gen is None and self.gens and L >= 24:
            gen = self.gens[self.gen_at % len(self.gens)]
            self.gen_at += 1
        if gen is None:
            return self.plant(L, place)
        self.used.add(gen)
        return self.plant(L, f"{place}|{gen}", lows_named(gen, L, self.rbits, self.size, self.rng))

    def next_window(self, margin: int = 0) -> int:
        return -(-(self.pos + margin) // self.geo.S)

    def build(self):
        lens = np.concatenate(self.lens)
        lows = np.concatenate(self.lows)
        nb = lens.size
        bits = 2 * self.k - self.rbits - (2 if self.both else 0)
        gmax = max(1, min(1 << 20, ((1 << min(bits, 62)) - 1) // (nb + 1)))
        ids = np.cumsum(self.rng.integers(1, gmax + 1, size=nb, dtype=np.int64)).astype(np.uint64)
        assert int(ids[-1]) < (1 << min(bits, 63))
        recs = lows.copy()
        idr = np.repeat(ids, lens)
        w, r = self.rbits // 64, self.rbits % 64
        recs[:, w] |= idr << np.uint64(r)
        if r and w + 1 < self.size:
            recs[:, w + 1] |= idr >> np.uint64(64 - r)
        assert recs.shape[0] == self.pos and np.array_equal(bucket_words(recs, 2 * self.k) if 2 * self.k < 64 * self.size else np.zeros_like(recs), np.zeros_like(recs))
        if self.both:
            assert np.array_equal(canonical_wide(recs, self.k), recs), "first symbol A, last symbol not T: the k-mer is its own canonical form"
            flip = self.rng.random(recs.shape[0]) < 0.5
            recs = np.where(flip[:, None], revcomp_wide(recs, self.k), recs)
        recs = recs[self.rng.permutation(recs.shape[0])]
        ordered = verify_wide(self.geo, recs, self.k, self.rbits, self.both, self.planted)
        return image_of_wide(recs, self.k), list(self.planted), ordered


def verify_wide(wg, recs, k, rbits, both, planted):
    """On the lexicographic sort of the records (canonicalised first for both strands): every planted (first, L) is a whole bucket, every other bucket has at most 5 records,
    and no planted bucket arrives in key order. Returns the ordered records."""
    if both:
        recs = canonical_wide(recs, k)
    order = order_of(recs)
    ordered = recs[order]
    n = ordered.shape[0]
    starts = bucket_starts_wide(ordered, rbits)
    blen = np.diff(np.concatenate([starts, [n]]))
    want = {f: L for f, L, _ in planted}
    assert len(want) == len(planted)
    firsts = np.array(sorted(want), dtype=np.int64)
    idx = np.searchsorted(starts, firsts)
    assert np.array_equal(starts[idx], firsts), "a planted bucket does not start where it was planted"
    assert np.array_equal(blen[idx], np.array([want[f] for f in sorted(want)])), "a planted bucket is not a whole bucket of its length"
    assert blen[np.setdiff1d(np.arange(starts.size), idx)].max(initial=0) <= 5, "filler made a long bucket"
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)  # equal records: in arrival order (the sort is stable)
    arrival = rank[order_of(bucket_words(recs, rbits))]  # the HBM passes are stable: the records of a bucket in image order
    for f, L, _ in planted:
        a = arrival[f:f + L]
        assert a.min() == f and a.max() == f + L - 1 and np.any(a[1:] < a[:-1]), ("a planted bucket arrives in order", f, L)
    return ordered


def finish_wide(bins):
    built = [b.build() for b in bins]
    return [x[0] for x in built], [x[1] for x in built], [x[2] for x in built]


# ------------------------------------------------------------------------------------------------ named placements of wide records
# A tile of wide records is the buckets that START in its window; S < CAP, so the last bucket start inside (b0, b0 + CAP] is the window's last one: a tile that outgrows the
# capacity is cut in front of its LAST bucket, whatever lies before. That bucket is the second chunk (up to CAP records) or a giant one (beyond).
#   - a tile that starts on its window's first record and holds exactly CAP (CAP + 1) records therefore ENDS in a bucket of more than CAP - S records: "small buckets summing
#     to CAP" is small buckets and one of CAP - S + 3 (+ 4) records, a big one (beyond BR_BIG) in the product's geometry.
#   - a bucket of BR_BIG - 1 .. BR_BIG + 1 records can BE the second chunk only where CAP - S + 1 < its length: not in the product's geometry for three words and more
#     (CAP - S = 128) nor for two (256); there such a bucket is planted as the END of the first chunk instead (`@ends-chunk0`), and `@is-chunk1` where the geometry admits it
#     (the emulated ones). check_named_wide asserts `@is-chunk1` present exactly where it can exist.
FAR = 4097


def far_distance(wg):
    """bounds-distance-far: 4097 (the tail of a giant bucket) where a bucket that long is still k_giant_tiles' to take, else what the emulated GT_MAX admits"""
    return FAR if wg.GT_MAX >= 2 * FAR else wg.GT_MAX - wg.GT_MAX // 4


def bounds_distances(wg):
    return [0, 1, 63, 64, 65, 127, 128, far_distance(wg)]


def place_lows(b: WideBin):
    """every generator on a bucket its owners walk (40 records) and on one dealt out over the workgroup (BR_BIG + 40)"""
    for gen in b.gens:
        for L in (40, b.geo.BIG + 40):
            b.fill(int(b.rng.integers(3, 20)))
            b.plant_named(None, L, "lows", gen)


def place_big(b: WideBin):
    S, CAP, BIG, WAVE = b.geo.S, b.geo.CAP, b.geo.BIG, b.geo.WAVE
    for L in (BIG - 1, BIG, BIG + 1):
        nm = f"big-{L}"
        w = b.next_window(3)
        b.plant_named(w * S, L, nm + "@row")  # from the tile's first record: over a row seam (64), inside one wave's rows where the width admits
        w = b.next_window(3)
        b.fill_to(w * S)
        b.plant_named(w * S + WAVE - 60, L, nm + "@wave")
        w = b.next_window(3)
        b.fill_to(w * S)
        p = (w + 1) * S - 3
        b.plant_named(p - L, L, nm + "@ends-chunk0")
        b.plant(w * S + CAP + 5 - p, "second-chunk")
        if L > CAP - S + 1:
            w = b.next_window(3)
            b.fill_to(w * S)
            b.plant_named(w * S + S - 1, L, nm + "@is-chunk1")


def place_tiles(b: WideBin):
    S, CAP = b.geo.S, b.geo.CAP
    for extra, nm in ((0, "tile-exactly-cap"), (1, "tile-cap-plus-1")):
        w = b.next_window(3)
        b.fill_to(w * S)
        p = (w + 1) * S - 3
        b.plant_named(p, w * S + CAP + extra - p, nm)


def place_bucket_cap(b: WideBin, lengths=None):
    S, CAP = b.geo.S, b.geo.CAP
    for L in lengths or (CAP, CAP + 1):
        nm = "bucket-cap" if L == CAP else "bucket-cap-plus-1"
        w = b.next_window(3)
        b.plant_named(w * S, L, nm + "@window-first")
        w = b.next_window(3)
        b.fill_to(w * S)
        b.plant_named(w * S + S - 1, L, nm + "@window-last")


def place_bounds(b: WideBin):
    S = b.geo.S
    for d in bounds_distances(b.geo):
        w = b.next_window(3)
        nm = "bounds-distance-far" if d == far_distance(b.geo) else f"bounds-distance-{d}"
        if d == 0:
            b.plant_named((w + 1) * S, 30, nm)
        else:
            b.plant_named((w + 1) * S - 20, d + 20, nm)
    w = b.next_window(3)
    b.plant_named(w * S + 5, 3 * S, "windows-without-a-start")


def place_giant_chunks(b: WideBin, lengths=None):
    GC = b.geo.GT_CHUNK
    for L in lengths or (GC, GC + 1, 2 * GC - 1, 2 * GC):
        w = b.next_window(3)
        b.plant_named(w * b.geo.S + 7, L, "giant-chunk")


def place_giant_run(b: WideBin):
    """one k-mer repeated from 30 records in front of k_giant_tiles' first chunk seam to 30 behind its second (where GT_MAX admits three chunks; else over the first seam
    alone), a second k-mer 300 times behind it. -> (run, second)"""
    wg, rb, size, rng = b.geo, b.rbits, b.size, b.rng
    GC, second = wg.GT_CHUNK, 300
    L = min(3 * GC + 100, wg.GT_MAX)
    lo_n = GC - 30
    run = min(2 * GC + 30, L - second - 10) - lo_n
    X, Y = 1 << (rb - 1), (1 << (rb - 1)) + 12345
    below = b._low(lo_n)
    below ^= bucket_words(below, rb - 1)                  # bit rbits - 1 clear: below X
    above = b._low(L - lo_n - run - second)
    above |= to_words([3 << (rb - 2)], size)              # bits rbits - 1 and rbits - 2 set: above Y
    lows = np.concatenate([below, np.repeat(to_words([X], size), run, axis=0), np.repeat(to_words([Y], size), second, axis=0), above])
    w = b.next_window(3)
    b.plant_at(w * wg.S + 50, L, "giant-run", lows=lows)
    assert run > second + 100 > 355
    return run, second


LAYOUTS = {
    "full": (place_lows, place_big, place_tiles, place_bucket_cap, place_bounds, place_giant_chunks),
    "thin": (place_tiles, lambda b: place_bucket_cap(b, (b.geo.CAP + 1,)), lambda b: place_giant_chunks(b, (b.geo.GT_CHUNK + 1,))),
}


def check_named_wide(wg, planted, ordered, rbits, want=()):
    """every named placement IS what its name says — decided on the ordered records — and every name of `want` is present"""
    S, CAP, BIG, WAVE, GC = wg.S, wg.CAP, wg.BIG, wg.WAVE, wg.GT_CHUNK
    seen = set()
    for bi, (pl, o, rb) in enumerate(zip(planted, ordered, rbits)):
        n = o.shape[0]
        starts = bucket_starts_wide(o, rb)
        for f, L, name in pl:
            place = name.split("|")[0]
            seen.add(place)
            if place.startswith("bin-"):
                assert L == BIG + 1 or L > CAP, where
                seen.add(place + (":giant" if L > CAP else ":big"))
            w = f // S
            b0, b1 = tile_of(wg, starts, n, w)
            cut = chunk_cut(wg, starts, b0, b1)
            where = (bi, f, L, name, b0, b1, cut)
            if place == "bin-start":
                assert f == 0, where
            elif place.startswith("bin-end"):
                last = bi == len(planted) - 1
                assert f + L == n and len(planted) >= 2 and (last if place == "bin-end-last-bin" else (place == "bin-end-middle-bin" and not last)), where
            elif place == "tile-exactly-cap":
                assert b0 == w * S and b1 == f + L and b1 - b0 == CAP and cut is None and f > b0, where
            elif place == "tile-cap-plus-1":
                assert b0 == w * S and b1 == f + L and b1 - b0 == CAP + 1 and cut == f and L <= CAP, where
            elif place.startswith("bucket-cap"):
                assert L == (CAP + 1 if "plus-1" in place else CAP), where
                if place.endswith("@window-first"):
                    assert f == w * S == b0 and b1 == f + L and (cut is None if L == CAP else cut == b0), where  # CAP + 1: a giant tile with nothing in front, cut 0
                else:
                    assert f == w * S + S - 1 and b0 == w * S and b1 == f + L and cut == f, where          # CAP: the tile's second chunk; CAP + 1: giant behind S - 1 records
            elif place.startswith("big-"):
                assert L == int(place[4:].split("@")[0]) and BIG - 1 <= L <= BIG + 1, where
                rel = f - b0
                if place.endswith("@row"):
                    assert rel == 0 and f == w * S and b1 - b0 <= CAP, where
                elif place.endswith("@wave"):
                    assert b0 == w * S and rel < WAVE < rel + L and b1 - b0 <= CAP, where
                elif place.endswith("@ends-chunk0"):
                    assert cut == f + L and b1 - b0 > CAP and b1 - cut <= CAP, where
                else:
                    assert place.endswith("@is-chunk1") and cut == f and b1 == f + L and b1 - b0 > CAP, where
            elif place.startswith("bounds-distance-"):
                d = far_distance(wg) if place.endswith("far") else int(place.rsplit("-", 1)[1])
                seam = (f // S + 1) * S if d else f
                assert seam % S == 0 and seam > 0 and f + L - seam == (d if d else L) and (d == 0 or f < seam), where
                i = np.searchsorted(starts, seam)
                assert (int(starts[i]) if i < starts.size else n) == seam + d, where  # what k_bucket_bounds must answer for that seam
            elif place == "windows-without-a-start":
                assert (f + L) // S - (f // S + 1) >= 2 and CAP < L <= wg.GT_MAX, where
            elif place == "giant-chunk":
                assert L in (GC, GC + 1, 2 * GC - 1, 2 * GC) and L <= wg.GT_MAX, where
            elif place == "giant-run":
                g = o[f:f + L]
                seams = [s for s in (GC, 2 * GC) if s + 30 < L - 310]
                assert seams and (len(seams) == 2 or wg.GT_MAX < 3 * GC), where
                r0, r1 = GC - 30, min(2 * GC + 30, L - 310)  # the run is exactly [r0, r1) of the bucket: the records are ordered, so equal ends mean one k-mer throughout
                assert np.array_equal(g[r0], g[r1 - 1]) and not np.array_equal(g[r0 - 1], g[r0]) and not np.array_equal(g[r1 - 1], g[r1]), where
                assert all(r0 < s < r1 - 1 for s in seams), where
            elif place == "gt-max":
                assert L == wg.GT_MAX, where
            elif place == "gt-max-plus-1":
                assert L == wg.GT_MAX + 1 and len(planted) == 3 and bi == 1, where
    for L in (BIG - 1, BIG, BIG + 1):
        assert (f"big-{L}@is-chunk1" in seen) == (L > CAP - S + 1 and f"big-{L}@row" in seen), ("a big bucket as the second chunk exists exactly where CAP - S + 1 < L", L)
    missing = [nm for nm in want if nm not in seen]
    assert not missing, missing
    return seen


FULL_NAMES = (["lows", "tile-exactly-cap", "tile-cap-plus-1", "windows-without-a-start", "giant-chunk", "bounds-distance-far"] +
              [f"bounds-distance-{d}" for d in (0, 1, 63, 64, 65, 127, 128)] +
              [f"bucket-cap{p}@window-{x}" for p in ("", "-plus-1") for x in ("first", "last")])


def full_names(wg):
    return FULL_NAMES + [f"big-{L}@{x}" for L in (wg.BIG - 1, wg.BIG, wg.BIG + 1) for x in ("row", "wave", "ends-chunk0")]


def n_giant_wide(wg, planted):
    """(tiles, records) k_giant_tiles must report — every planted bucket beyond CAP and up to GT_MAX records is one tile of its own length — and the bins that must come back
    (a bucket beyond GT_MAX records)"""
    g = [L for pl in planted for _, L, _ in pl if wg.CAP < L <= wg.GT_MAX]
    back = [i for i, pl in enumerate(planted) if any(L > wg.GT_MAX for _, L, _ in pl)]
    return len(g), sum(g), back


def locate_wide(wg, planted_of_bin, ordered, kmer_index, cutoff_min, cutoff_max):
    """the planted bucket (place|generator) that holds — or lies nearest in front of — the `kmer_index`-th COUNTED k-mer of a bin"""
    n = ordered.shape[0]
    first_at = np.flatnonzero(np.concatenate([[True], np.any(ordered[1:] != ordered[:-1], axis=1)]))
    counts = np.diff(np.concatenate([first_at, [n]]))
    kept = first_at[(counts >= cutoff_min) & (counts <= cutoff_max)]
    if kmer_index >= kept.size:
        return ("behind the last counted k-mer", kmer_index, int(kept.size))
    pos = int(kept[kmer_index])
    best = None
    for f, L, name in planted_of_bin:
        if f <= pos:
            best = dict(first=f, len=L, name=name, holds_it=pos < f + L, record=pos)
    return best


def independent_counts(ordered, cutoff_min, cutoff_max):
    """(distinct, below cutoff_min, above cutoff_max, records, counted k-mers) of a bin from its ordered records: np.unique over byte rows, the cutoffs applied here"""
    rows = np.ascontiguousarray(ordered[:, ::-1]).astype(">u8").view(np.uint8).reshape(ordered.shape[0], -1)
    _, counts = np.unique(rows, axis=0, return_counts=True)
    below, above = int((counts < cutoff_min).sum()), int(((counts >= cutoff_min) & (counts > cutoff_max)).sum())
    return counts.size, below, above, ordered.shape[0], counts.size - below - above


# ------------------------------------------------------------------------------------------------ the cases of the wide sweep
# name -> (k, bins per layout, parameters). Forward strand only unless the name says otherwise (`forward-only` of the issue is every case but `both-strands-*`): a lows
# generator's values end in any symbol. KFF at k = 127 is not a rank case — a KFF record of 32 + 1 bytes outgrows the 32-byte record it is counted from (count_applicable) —
# so the KFF legs are k = 55 and k = 124 (31 + 1 bytes).
WIDE_SPECS = {
    "w2-k55": (55, ["full"], dict(lut_prefix_len=3)),                                # two words, indirect, rbits 80; k_giant_tiles: 10 passes (even: the result in T)
    "w2-k55-4bins": (55, ["full", "start-giant", "end-big", "end-giant"], dict(lut_prefix_len=3)),
    "w2-rbits-56": (44, ["full"], dict(lut_prefix_len=4)),                           # m0 = 2^56 - 1, m1 = 0
    "w2-rbits-64": (48, ["full"], dict(lut_prefix_len=4)),                           # m0 = all ones, m1 = 0: word 1 is bucket bits alone
    "w2-rbits-72": (51, ["full"], dict(lut_prefix_len=3)),                           # m1 = 0xFF; k_giant_tiles: 9 passes (odd: the result in U, counted in place)
    "w2-k64-direct": (64, ["full", "thin"], dict(lut_prefix_len=4)),                 # six direct passes; no room for a tag: every bin a group of its own
    "w2-k40-direct": (40, ["full", "thin", "end-big"], dict(lut_prefix_len=4)),      # five passes: 6 spare bits above the key in the top byte; BR_BIG + 1 ends the LAST bin
    "w2-k55-indirect-off": (55, ["full"], dict(lut_prefix_len=3)),                   # the bins of w2-k55 under KMC_HIP_INDIRECT=0 (the caller sets it, in a child process)
    "w3-k70": (70, ["full", "thin", "end-big"], dict(lut_prefix_len=2)),                 # BR_BIG + 1 ends the last bin of the group
    "w3-k96": (96, ["full"], dict(lut_prefix_len=4)),                                # a k-mer that fills word 2
    "w4-k127": (127, ["full", "start-giant", "end-big", "end-giant"], dict(lut_prefix_len=3)),
    "w7-k200": (200, ["full", "end-giant"], dict(lut_prefix_len=4)),                 # two bins: five passes
    "w8-k256": (256, ["full"], dict(lut_prefix_len=4)),
    "giant-odd-k74": (74, ["thin", "end-giant"], dict(lut_prefix_len=2)),           # three words, rbits 120; k_giant_tiles: 15 passes (odd)
    "giant-run-k55": (55, ["giant-run", "thin"], dict(lut_prefix_len=3)),
    "giant-run-k127": (127, ["giant-run", "thin"], dict(lut_prefix_len=3)),
    "gt-max-k55": (55, ["gt-max", "gt-max-plus-1", "end-giant"], dict(lut_prefix_len=3)),
    "gt-max-k127": (127, ["gt-max", "gt-max-plus-1", "end-giant"], dict(lut_prefix_len=3)),
    "kff-k55": (55, ["thin", "end-giant"], dict(lut_prefix_len=0, output_type=1)),
    "kff-k124": (124, ["thin", "end-giant"], dict(lut_prefix_len=0, output_type=1)),
    "without-output-k55": (55, ["thin", "end-giant"], dict(lut_prefix_len=3, without_output=1)),
    "without-output-k127": (127, ["thin", "end-giant"], dict(lut_prefix_len=3, without_output=1)),
    "both-strands-k55": (55, ["thin", "end-giant"], dict(lut_prefix_len=3, both_strands=1)),
    "both-strands-k127": (127, ["thin", "end-giant"], dict(lut_prefix_len=3, both_strands=1)),
}
WIDE_CASES = tuple(WIDE_SPECS)
WIDE_PLANS = {  # case -> (rbits, passes, indirect) per group, as the issue's table wants them: plan_for must agree (make_wide_case asserts it)
    "w2-k55": [(80, 4, True)], "w2-k55-4bins": [(80, 4, True)], "w2-rbits-56": [(56, 4, True)], "w2-rbits-64": [(64, 4, True)], "w2-rbits-72": [(72, 4, True)],
    "w2-k64-direct": [(80, 6, False)] * 2, "w2-k40-direct": [(48, 5, False)], "w2-k55-indirect-off": [(80, 4, False)], "w3-k70": [(112, 4, True)], "w3-k96": [(160, 4, True)],
    "w4-k127": [(224, 4, True)], "w7-k200": [(368, 5, False)], "w8-k256": [(480, 4, True)],
}


GIANT_PASSES_ODD = {"w2-rbits-72": True, "giant-odd-k74": True, "w2-k55": False, "w4-k127": False}  # the issue's giant-odd / giant-even: make_wide_case asserts the parity


class WideCase:
    pass


def make_wide_case(geo: Geometry, case: str, env=os.environ):
    """-> WideCase: k, kw (parameters of capi.make_params), bins, planted, ordered (per bin), rbits (per bin), groups [(bins, rbits, passes, indirect)], wg, names present"""
    k, layout, kw = WIDE_SPECS[case]
    kw = dict(dict(both_strands=0), **kw)
    size = words_of(k)
    wg = geo.wide(size)
    seed = 2000 + zlib.crc32(("w2-k55" if case == "w2-k55-indirect-off" else case).encode()) % 1000
    rng = np.random.default_rng(seed)
    if case == "w2-k55-indirect-off":
        assert env.get("KMC_HIP_INDIRECT") == "0", "this case is for a process of its own with KMC_HIP_INDIRECT=0 (the switch is read once per process)"
    c = WideCase()
    c.case, c.k, c.kw, c.wg, c.size = case, k, kw, wg, size
    rec_bytes = 0 if kw.get("without_output") else -(-(k - kw["lut_prefix_len"]) // 4) + 1
    sizes = group_sizes(k, len(layout))
    c.groups = [(g,) + plan_for(k, g, 2 * wg.CAP, geo, rec_bytes, env) for g in sizes]
    if case in WIDE_PLANS:
        assert [g[1:] for g in c.groups] == WIDE_PLANS[case], (case, c.groups)
    rbits = [g[1] for g in c.groups for _ in range(g[0])]
    if case in GIANT_PASSES_ODD:
        assert all((giant_passes(rb) % 2 == 1) == GIANT_PASSES_ODD[case] for rb in rbits), (case, rbits)
    bins = []
    c.kw_extra = {}
    for i, (lay, rb) in enumerate(zip(layout, rbits)):
        b = WideBin(wg, k, rb, rng, kw["both_strands"], lows_generators(rb, size) if lay in ("full", "thin") else ())
        if lay == "full":
            b.plant_named(0, wg.BIG + 1, "bin-start")
            for f in LAYOUTS["full"]:
                f(b)
            b.fill(int(rng.integers(20, 60)))
            assert b.used == set(b.gens), sorted(set(b.gens) - b.used)
        elif lay == "thin":
            b.fill(wg.CAP + int(rng.integers(1, 50)))
            for f in LAYOUTS["thin"]:
                f(b)
            w = b.next_window(3)
            b.fill_to(w * wg.S)
            b.plant_named(w * wg.S + wg.WAVE - 60, wg.BIG + 1, f"big-{wg.BIG + 1}@wave")
            b.fill(int(rng.integers(20, 60)))
        elif lay == "start-giant":
            b.plant_named(0, wg.CAP + 40, "bin-start")
            b.fill(wg.CAP)
            b.plant_named(None, wg.CAP + 7, "bin-end-middle-bin")
        elif lay == "end-big":
            b.fill(wg.CAP + int(rng.integers(1, 50)))
            b.plant_named(None, wg.BIG + 1, "bin-end-last-bin" if i == len(layout) - 1 else "bin-end-middle-bin")
        elif lay == "end-giant":
            b.fill(wg.CAP + int(rng.integers(1, 50)))
            b.plant_named(None, wg.BIG + 1, "inner-big")
            b.fill(wg.S)
            b.plant_named(None, wg.CAP + 1 + int(rng.integers(0, 50)), "bin-end-last-bin")
        elif lay == "giant-run":
            b.fill(wg.CAP + int(rng.integers(1, 50)))
            run, second = place_giant_run(b)
            b.fill(wg.CAP)
            c.kw = dict(kw, cutoff_max=(run + second) // 2, counter_max=255)
            c.run, c.second = run, second
        elif lay == "gt-max":
            b.fill(wg.CAP + int(rng.integers(1, 50)))
            b.plant(wg.GT_MAX, "gt-max")
            b.fill(int(rng.integers(20, 60)))
        elif lay == "gt-max-plus-1":
            b.fill(wg.CAP + int(rng.integers(1, 50)))
            b.plant(wg.GT_MAX + 1, "gt-max-plus-1")
            b.fill(int(rng.integers(20, 60)))
        else:
            raise KeyError(lay)
        assert b.pos > wg.CAP
        bins.append(b)
    assert all(sum(b.pos for b in bins[i:i + g]) > wg.CAP for i, g in zip(np.cumsum([0] + sizes[:-1]), sizes))
    c.bins, c.planted, c.ordered = finish_wide(bins)
    c.rbits = rbits
    want = []
    if "full" in layout:
        want += full_names(wg) + ["bin-start"]
    if "thin" in layout:
        want += ["tile-cap-plus-1", "bucket-cap-plus-1@window-first", "bucket-cap-plus-1@window-last", "giant-chunk", f"big-{wg.BIG + 1}@wave"]
    if "full" in layout:
        want.append("bin-start:big")
    for i, x in enumerate(layout):
        if x == "start-giant":
            want += ["bin-start:giant", "bin-end-middle-bin:giant"]
        elif x == "end-big":
            want.append("bin-end-last-bin:big" if i == len(layout) - 1 else "bin-end-middle-bin:big")
        elif x == "end-giant":
            want.append("bin-end-last-bin:giant")
        elif x not in ("full", "thin"):
            want.append(x)
    c.names = check_named_wide(wg, c.planted, c.ordered, rbits, want)
    assert all(x not in ("end-giant",) or i == len(layout) - 1 for i, x in enumerate(layout))
    return c
