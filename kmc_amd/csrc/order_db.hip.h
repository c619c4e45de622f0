/*
 * kmc_amd/csrc/order_db.hip.h — a GLOBALLY ordered database on the device (what `kmc_tools transform <db> sort <out>` does
 * with KMC's database on the CPU, kmc_tools/kmc1_db_writer.h:368-395).
 *
 * Stage 2 leaves the counted k-mers ordered INSIDE every signature bin: per bin a run of (suffix, count) records and a LUT of how many records
 * each lut_prefix_len-symbol prefix has (kb_sorter.h:1196-1203). Bins partition the k-mers by signature, so every counted k-mer is in exactly
 * one bin: the globally ordered database is a sort of the union, no counts to merge.
 *   k_db_cumsum   one workgroup: a bin's LUT counts -> exclusive prefix sums (record index of the first record of every prefix)
 *   k_db_unpack   one thread per record of a bin: prefix by binary search in those sums, k-mer = prefix . suffix, record = (k-mer words, count)
 *   (sort)        the library's own 8-bit LSD passes over the k-mer bytes of those records (stable: the count rides along above the key)
 *   k_db_pack     one thread per record: (suffix, count) bytes for the NEW lut_prefix_len (kmc1_db_writer.h:388-391: kmer.store big-endian, counter
 *                 little-endian), and the KMC1 LUT (entry i = records with a prefix below i, :376-383) from the prefix boundaries — no atomics
 * HBM-bound byte shuffling; a utility next to the hot path, not part of it (bench.py does not time it).
 *
 * Set operations between TWO such databases (`kmc_tools simple`, kmc_tools/operations.h:298-491 feeding kmc1_db_writer.h:375-404): both bodies unpacked by
 * k_db_unpack (a KMC1 LUT already holds the exclusive sums; a record outside its input's cutoffs gets the count SO_ABSENT and stays where it is), then
 *   k_so_partition  one thread per tile boundary of the merged sequence: the merge-path split (i, j) by bisection on the diagonal, A before B on equal keys
 *   k_so_tile       one workgroup per tile: its slices of A and B staged in LDS with one record of halo (A[i0 - 1], B[j1]), merged there, every element
 *                   classified only-in-A / only-in-B / pair, operation + counter mode + the writer's cutoffs and clamp applied; run twice — <false> counts the
 *                   kept records of the tile and the six tallies, k_db_cumsum scans the counts, <true> writes the kept records at their offsets
 * and k_db_pack packs the result for the output's lut_prefix_len and counter size.
 */
#ifndef KMC_AMD_ORDER_DB_HIP_H
#define KMC_AMD_ORDER_DB_HIP_H

#include "kernels.hip.h"

__global__ void __launch_bounds__(256) k_db_cumsum(const u64 *__restrict__ counts, u64 n_entries, u64 *__restrict__ sums /* [n_entries + 1] */)
{
	__shared__ u64 s_scan[5];
	u64 carry = 0;
	for (u64 c0 = 0; c0 < n_entries; c0 += 256) {
		const u64 i = c0 + threadIdx.x;
		const u64 v = i < n_entries ? counts[i] : 0;
		u64 total;
		const u64 ex = block_excl_sum<4, u64>(v, s_scan, total);
		if (i < n_entries)
			sums[i] = carry + ex;
		carry += total;
	}
	if (threadIdx.x == 0)
		sums[n_entries] = carry;
}

constexpr u64 SO_ABSENT = ~0ull; /* count word of a record its input's cutoffs removed (a count has 32 bits) */

/* records of one bin: [sbytes suffix bytes, most significant first][cbytes count bytes, least significant first] -> (SIZE k-mer words, 1 count word) */
template <int SIZE>
__global__ void __launch_bounds__(256) k_db_unpack(const uint8_t *__restrict__ recs, u64 n, const u64 *__restrict__ sums, u32 n_entries, u32 k, u32 p, u32 sbytes,
                                                  u32 cbytes, u64 *__restrict__ out /* [n][SIZE + 1] */, u32 cut_min, u64 cut_range /* a count c with
                                                  (u32)(c - cut_min) > cut_range (kmc_tools/kmc1_db_reader.h:574-576,618) is stored as SO_ABSENT */)
{
	const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
	if (j >= n)
		return;
	u32 lo = 0, hi = n_entries; /* largest i with sums[i] <= j */
	while (hi - lo > 1) {
		const u32 mid = (lo + hi) >> 1;
		if (sums[mid] <= j)
			lo = mid;
		else
			hi = mid;
	}
	const uint8_t *r = recs + j * (u64)(sbytes + cbytes);
	u64 x[SIZE];
#pragma unroll
	for (int w = 0; w < SIZE; ++w)
		x[w] = 0;
	for (u32 q = 0; q < sbytes; ++q) { /* byte sbytes-1-q of the k-mer */
		const u32 pb = sbytes - 1 - q;
#pragma unroll
		for (int w = 0; w < SIZE; ++w)
			if ((pb >> 3) == (u32)w)
				x[w] |= (u64)r[q] << ((pb & 7) * 8);
	}
	const u32 pbit = 2 * (k - p); /* the prefix sits above the suffix symbols */
#pragma unroll
	for (int w = 0; w < SIZE; ++w) {
		if ((pbit >> 6) == (u32)w)
			x[w] |= (u64)lo << (pbit & 63);
		if ((pbit & 63) && (pbit >> 6) + 1 == (u32)w)
			x[w] |= (u64)lo >> (64 - (pbit & 63));
	}
	u64 c = 0;
	for (u32 q = 0; q < cbytes; ++q)
		c |= (u64)r[sbytes + q] << (8 * q);
	if ((u64)(u32)((u32)c - cut_min) > cut_range)
		c = SO_ABSENT;
	u64 *o = out + j * (u64)(SIZE + 1);
#pragma unroll
	for (int w = 0; w < SIZE; ++w)
		o[w] = x[w];
	o[SIZE] = c;
}

template <int SIZE>
__global__ void __launch_bounds__(256) k_db_pack(const u64 *__restrict__ recs /* [n][SIZE + 1] ascending */, u64 n, u32 k, u32 p_out, u32 cbytes, uint8_t *__restrict__ out,
                                                u64 *__restrict__ lut /* [4^p_out], zeroed */, const u64 *__restrict__ n_dev /* nullptr, or n as an earlier kernel left it (then `n` is the launch's upper bound) */)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (n_dev)
		n = *n_dev;
	if (i >= n)
		return;
	const u32 sbytes = (k - p_out) / 4, rb = sbytes + cbytes;
	u64 x[SIZE], nx[SIZE];
	const u64 *r = recs + i * (u64)(SIZE + 1);
#pragma unroll
	for (int w = 0; w < SIZE; ++w) {
		x[w] = r[w];
		nx[w] = i + 1 < n ? r[SIZE + 1 + w] : 0;
	}
	const u64 cnt = r[SIZE];
	uint8_t *o = out + i * (u64)rb;
	for (u32 q = 0; q < sbytes; ++q)
		o[q] = (uint8_t)kmc_get_byte<SIZE>(x, sbytes - 1 - q);
	for (u32 q = 0; q < cbytes; ++q)
		o[sbytes + q] = (uint8_t)(cnt >> (8 * q));
	const u32 pshift = 2 * (k - p_out);
	const u64 n_pref = 1ull << (2 * p_out);
	const u64 pa = kmc_remove_suffix<SIZE>(x, pshift) & (n_pref - 1);
	const u64 pb = i + 1 < n ? (kmc_remove_suffix<SIZE>(nx, pshift) & (n_pref - 1)) : n_pref - 1 + 1;
	for (u64 q = pa + 1; q <= pb && q < n_pref; ++q)
		lut[q] = i + 1; /* records with a prefix below q */
}

/* ---- set operations between two ordered databases (`kmc_tools simple`) ---- */

#ifndef SO_THREADS
#define SO_THREADS 256 /* threads of a k_so_tile workgroup */
#endif
/* merged records per thread of k_so_tile: the tile is SO_THREADS x this many. The default keeps a tile's two LDS areas (its slices of A and B, the kept records
 * on their way out) at 2 x 16 KB for every record width — five workgroups of 4 waves on a CU's 160 KB, enough to hide the serial LDS walk of a thread's share —
 * $KMC_HIP_SETOP_IPT overrides (tests: 1, a tile of 256 records, so that a database of a thousand records crosses tile boundaries). */
#ifndef SO_IPT_WORDS
#define SO_IPT_WORDS 8 /* 64-bit words of record per thread: records per thread = max(1, SO_IPT_WORDS / (SIZE + 1)) */
#endif
constexpr u32 SO_IPT_MAX = 16;
template <int SIZE> constexpr u32 so_default_ipt() { return SO_IPT_WORDS / (SIZE + 1) ? SO_IPT_WORDS / (SIZE + 1) : 1u; }
/* dynamic LDS of k_so_tile: the slices with one record of halo each, and (WRITE) the kept records */
template <int SIZE> constexpr size_t so_lds_bytes(u32 ipt, bool write) { return ((size_t)SO_THREADS * ipt + 2) * (SIZE + 1) * 8 + (write ? (size_t)SO_THREADS * ipt * (SIZE + 1) * 8 : 0); }

enum : u32 { SO_INTERSECT = 0, SO_UNION = 1, SO_KMERS_SUBTRACT = 2, SO_COUNTERS_SUBTRACT = 3, SO_REVERSE_KMERS_SUBTRACT = 4, SO_REVERSE_COUNTERS_SUBTRACT = 5, SO_N_OPS = 6 };
enum : u32 { SO_CNT_MIN = 0, SO_CNT_MAX = 1, SO_CNT_SUM = 2, SO_CNT_DIFF = 3, SO_CNT_LEFT = 4, SO_CNT_RIGHT = 5, SO_N_CNT = 6 };
enum : u32 { SO_ST_PAIRS = 0, SO_ST_ONLY_A = 1, SO_ST_ONLY_B = 2, SO_ST_BELOW_MIN = 3, SO_ST_ABOVE_MAX = 4, SO_ST_WRITTEN = 5 };
struct SoStep {
	const u64 *rec; /* the record to keep, nullptr: none */
	u32 c, kind /* 0 none, 1 only in A, 2 only in B, 3 pair */, cut;
	bool took_a;
};
struct SoTally { /* a thread's share of stats[0..4] */
	u32 pairs = 0, only_a = 0, only_b = 0, below_min = 0, above_max = 0;
};
struct SoOp {
	u32 op, counter_op, cutoff_min, counter_max;
	u64 cutoff_max;
};

/* keys of unpacked records (SIZE words, word 0 least significant) */
template <int SIZE> __device__ __forceinline__ bool so_less(const u64 *a, const u64 *b)
{
#pragma unroll
	for (int w = SIZE - 1; w >= 0; --w) {
		if (a[w] != b[w])
			return a[w] < b[w];
	}
	return false;
}
template <int SIZE> __device__ __forceinline__ bool so_equal(const u64 *a, const u64 *b)
{
	bool eq = true;
#pragma unroll
	for (int w = 0; w < SIZE; ++w)
		eq = eq && a[w] == b[w];
	return eq;
}

/* COutputBundle::GetCounter (kmc_tools/bundle.h:257-278) on 32-bit unsigned counts: sum wraps, diff stops at 0 */
__device__ __forceinline__ u32 so_counter(u32 mode, u32 c1, u32 c2)
{
	switch (mode) {
	case SO_CNT_MIN: return c1 < c2 ? c1 : c2;
	case SO_CNT_MAX: return c1 > c2 ? c1 : c2;
	case SO_CNT_SUM: return c1 + c2;
	case SO_CNT_DIFF: return c1 > c2 ? c1 - c2 : 0u;
	case SO_CNT_LEFT: return c1;
	default: return c2;
	}
}

/* merge-path split of diagonal `diag` (records of the merged sequence in front of it): how many of them are A's, A before B on equal keys.
 * a / b: records of W = SIZE + 1 words; na / nb: the records the diagonal may take from each */
template <int SIZE> __device__ __forceinline__ u64 so_split(const u64 *a, u64 na, const u64 *b, u64 nb, u64 diag)
{
	constexpr int W = SIZE + 1;
	u64 lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
	while (lo < hi) {
		const u64 mid = (lo + hi) >> 1;
		if (!so_less<SIZE>(b + (diag - 1 - mid) * W, a + mid * W)) /* A[mid] <= B[diag - 1 - mid]: A[mid] lies in front of the diagonal */
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

template <int SIZE>
__global__ void __launch_bounds__(256) k_so_partition(const u64 *__restrict__ a, u64 na, const u64 *__restrict__ b, u64 nb, u32 tile, u64 n_tiles, u64 *__restrict__ split /* [n_tiles + 1] */)
{
	const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
	if (t > n_tiles)
		return;
	const u64 n = na + nb, diag = t * tile < n ? t * tile : n;
	split[t] = so_split<SIZE>(a, na, b, nb, diag);
}

/* One element of a thread's walk over the merged tile: takes the smaller head (A on equal keys), classifies it and applies operation, counter mode and the writer's
 * rule (kmc1_db_writer.h:382-385). sa: A[i0 - ha ..], sb: B[j0 ..] with B[j1] behind the slice when hb — keys are distinct inside an input, so the partner of A[i] can
 * only be the B head, and the partner of B[j] the A record taken last, whichever tile they lie in. A record with the count SO_ABSENT (cut by its input's cutoffs)
 * takes its place in the walk and counts as missing. i, j: the heads; the caller advances the one that was taken. */
template <int SIZE>
__device__ __forceinline__ SoStep so_step(const u64 *sa, const u64 *sb, u32 ha, u32 na, u32 nb, u32 hb, u32 i, u32 j, const SoOp op)
{
	constexpr int W = SIZE + 1;
	const u64 *ra = sa + (size_t)(ha + i) * W, *rb = sb + (size_t)j * W;
	const bool take_a = j >= nb || (i < na && !so_less<SIZE>(rb, ra));
	const u64 *rec;
	u32 c = 0;
	u32 kind; /* 0 none, 1 only in A, 2 only in B, 3 pair */
	u32 c1 = 0, c2 = 0;
	if (take_a) {
		rec = ra;
		const bool have_b = j < nb + hb && so_equal<SIZE>(ra, rb) && rb[SIZE] != SO_ABSENT;
		kind = ra[SIZE] == SO_ABSENT ? 0u : have_b ? 3u : 1u;
		c1 = (u32)ra[SIZE];
		c2 = have_b ? (u32)rb[SIZE] : 0u;
	} else {
		rec = rb;
		const u64 *pa = ra - W; /* the A record in front of the head */
		const bool have_a = ha + i > 0 && so_equal<SIZE>(pa, rb) && pa[SIZE] != SO_ABSENT;
		kind = rb[SIZE] == SO_ABSENT || have_a ? 0u : 2u;
		c2 = (u32)rb[SIZE];
	}
	bool keep = false;
	u32 cut = 0; /* 1 below the output's cutoff_min, 2 above its cutoff_max */
	if (kind == 3) {
		keep = op.op == SO_INTERSECT || op.op == SO_UNION || op.op == SO_COUNTERS_SUBTRACT || op.op == SO_REVERSE_COUNTERS_SUBTRACT; /* operations.h:317 */
		c = op.op == SO_REVERSE_COUNTERS_SUBTRACT ? so_counter(op.counter_op, c2, c1) : so_counter(op.counter_op, c1, c2); /* :337-340 */
	} else if (kind == 1) {
		keep = op.op == SO_UNION || op.op == SO_KMERS_SUBTRACT || op.op == SO_COUNTERS_SUBTRACT; /* :319 */
		c = c1;
	} else if (kind == 2) {
		keep = op.op == SO_UNION || op.op == SO_REVERSE_KMERS_SUBTRACT || op.op == SO_REVERSE_COUNTERS_SUBTRACT; /* :321 */
		c = c2;
	}
	if (keep && c < op.cutoff_min) {
		cut = 1;
		keep = false;
	} else if (keep && (u64)c > op.cutoff_max) {
		cut = 2;
		keep = false;
	}
	if (c > op.counter_max)
		c = op.counter_max;
	return SoStep{keep ? rec : nullptr, c, kind, cut, take_a};
}

/* WRITE = false: tile_count[tile] = kept records of the tile, stats[0..4] += the tile's tallies. WRITE = true: the kept records to out[tile_base[tile] ..]. */
template <int SIZE, bool WRITE>
__global__ void __launch_bounds__(SO_THREADS) k_so_tile(const u64 *__restrict__ a, u64 n_a, const u64 *__restrict__ b, u64 n_b, const u64 *__restrict__ split, u32 ipt, SoOp op,
                                                       const u64 *__restrict__ tile_base, u64 *__restrict__ tile_count, u64 *__restrict__ out, u64 *__restrict__ stats)
{
	constexpr int W = SIZE + 1;
	KMC_DYN_LDS(u64, so_lds);
	__shared__ u32 s_scan[SO_THREADS / 64 + 1];
	const u32 tid = threadIdx.x, tile = SO_THREADS * ipt;
	const u64 t = blockIdx.x, n = n_a + n_b;
	const u64 d0 = t * tile, d1 = d0 + tile < n ? d0 + tile : n;
	const u64 i0 = split[t], i1 = split[t + 1], j0 = d0 - i0, j1 = d1 - i1;
	const u32 na = (u32)(i1 - i0), nb = (u32)(j1 - j0), ha = i0 > 0 ? 1u : 0u, hb = j1 < n_b ? 1u : 0u;
	u64 *sa = so_lds, *sb = so_lds + (size_t)(na + ha) * W, *s_out = so_lds + (size_t)(tile + 2) * W;
	{ /* both slices are runs of whole records: flat, coalesced copies */
		const u64 *ga = a + (i0 - ha) * W, *gb = b + j0 * W;
		for (u32 g = tid; g < (na + ha) * W; g += SO_THREADS)
			sa[g] = ga[g];
		for (u32 g = tid; g < (nb + hb) * W; g += SO_THREADS)
			sb[g] = gb[g];
	}
	__syncthreads();
	const u32 len = na + nb;
	const u32 m0 = tid * ipt < len ? tid * ipt : len, m1 = m0 + ipt < len ? m0 + ipt : len;
	const u32 is = (u32)so_split<SIZE>(sa + (size_t)ha * W, na, sb, nb, m0), js = m0 - is;
	SoTally tally;
	u32 kept = 0;
	{
		u32 i = is, j = js;
		for (u32 m = m0; m < m1; ++m) {
			const SoStep r = so_step<SIZE>(sa, sb, ha, na, nb, hb, i, j, op);
			i += r.took_a ? 1u : 0u;
			j += r.took_a ? 0u : 1u;
			kept += r.rec ? 1u : 0u;
			tally.pairs += r.kind == 3 ? 1u : 0u;
			tally.only_a += r.kind == 1 ? 1u : 0u;
			tally.only_b += r.kind == 2 ? 1u : 0u;
			tally.below_min += r.cut == 1 ? 1u : 0u;
			tally.above_max += r.cut == 2 ? 1u : 0u;
		}
	}
	u32 total;
	const u32 first = block_excl_sum<SO_THREADS / 64, u32>(kept, s_scan, total);
	if (!WRITE) {
		const u32 mine[5] = {tally.pairs, tally.only_a, tally.only_b, tally.below_min, tally.above_max};
#pragma unroll
		for (int q = 0; q < 5; ++q) {
			const u32 v = wave_sum<u32>(mine[q]);
			if ((tid & 63) == 0 && v)
				atomicAdd(stats + q, (u64)v);
		}
		if (tid == 0)
			tile_count[t] = total;
		return;
	}
	{
		u32 i = is, j = js;
		u64 *o = s_out + (size_t)first * W;
		for (u32 m = m0; m < m1; ++m) {
			const SoStep r = so_step<SIZE>(sa, sb, ha, na, nb, hb, i, j, op);
			i += r.took_a ? 1u : 0u;
			j += r.took_a ? 0u : 1u;
			if (r.rec) {
#pragma unroll
				for (int w = 0; w < SIZE; ++w)
					o[w] = r.rec[w];
				o[SIZE] = r.c;
				o += W;
			}
		}
	}
	__syncthreads();
	u64 *go = out + tile_base[t] * W;
	for (u32 g = tid; g < total * W; g += SO_THREADS)
		go[g] = s_out[g];
}

#endif
