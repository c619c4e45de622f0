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
 *
 * A set expression over SEVERAL such databases (`kmc_tools complex`): every named input through k_db_unpack once, then
 *   k_cx_partition  one thread per sample (every S-th record of every leaf): its rank among all samples; every M-th sample by rank is a tile's splitter
 *   k_cx_tile       one workgroup per tile of the key space: every leaf's slice in LDS, the postfix program walked once per record — <false> counts, <true> writes
 * and k_db_pack as above (the comment in front of the kernels has the partition's bound and its proof).
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

/* ---- reads against an ordered database (`kmc_tools filter`) ---- */

#ifndef DQ_THREADS
#define DQ_THREADS 256 /* threads of a k_dbq_lookup workgroup */
#endif
/* window starts per thread of k_dbq_lookup: the tile is DQ_THREADS x this many positions and stages tile + k - 1 symbols, so the halo is read (k - 1) / tile times
 * too often — 11 % at k = 224 with 2048 positions. LDS is 3 bits per staged symbol: no limit in practice. $KMC_HIP_QUERY_IPT overrides (tests: 1). */
constexpr u32 DQ_IPT_MAX = 64;
template <int SIZE> constexpr u32 dq_default_ipt() { return SIZE <= 2 ? 4u : 8u; }
constexpr u32 dq_staged_symbols(u32 ipt, u32 k) { return (DQ_THREADS * ipt + k - 1 + DQ_THREADS - 1) / DQ_THREADS * DQ_THREADS; } /* whole rows of DQ_THREADS symbols */
constexpr u32 DQ_CODE_PAD = 2; /* zero words in front of the codes: dq_bits64 reads up to two words before the first symbol */
constexpr u32 dq_code_words(u32 ipt, u32 k) { return DQ_CODE_PAD + dq_staged_symbols(ipt, k) / 16 + 1; }
constexpr size_t dq_lds_bytes(u32 ipt, u32 k) { return ((size_t)dq_code_words(ipt, k) + dq_staged_symbols(ipt, k) / 32) * 4; }
enum : u32 { DQ_ST_VALID = 0, DQ_ST_FOUND = 1, DQ_ST_CUT = 2, DQ_ST_INVALID = 3 };

/* CKmerAPI::num_codes (kmc_api/kmer_api.h:268-275): ACGTacgt -> 0..3, every other byte 4 */
__device__ __forceinline__ u32 dq_code(u32 c)
{
	const u32 u = c & 0xDFu;
	return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

/* the 64 bits in front of bit `e` of the staged code stream (symbol s: bits 2s, 2s + 1, the first symbol in the most significant bits of word DQ_CODE_PAD) */
__device__ __forceinline__ u64 dq_bits64(const u32 *code, u32 e)
{
	const u32 g = DQ_CODE_PAD + (e >> 5), r = e & 31;
	const u64 ab = ((u64)code[g - 2] << 32) | code[g - 1];
	return r ? (ab << r) | (code[g] >> (32 - r)) : ab;
}

/* flat over the window starts i of d_seq: the k-mer at i (the smaller of it and its reverse complement with both_strands, kmc_file.cpp:998-1001) looked up as
 * CKMCFile::BinarySearch does under the bounds of its LUT prefix (kmc_file.cpp:905-925,1321-1399) */
template <int SIZE>
__global__ void __launch_bounds__(DQ_THREADS) k_dbq_lookup(const uint8_t *__restrict__ seq, u64 n_bytes, u32 k, u32 both_strands, const uint8_t *__restrict__ recs, u64 n_recs,
                                                          const u64 *__restrict__ lut, u32 p, u32 cbytes, u32 cut_min, u64 cut_max, u32 ipt, u32 *__restrict__ counters /* [n_bytes] */,
                                                          u64 *__restrict__ stats /* [4] */)
{
	KMC_DYN_LDS(u32, dq_lds);
	__shared__ u32 s_tally[DQ_THREADS / 64][4];
	const u32 tid = threadIdx.x, lane = tid & 63, tile = DQ_THREADS * ipt, n_sym = dq_staged_symbols(ipt, k);
	u32 *s_code = dq_lds, *s_inv = dq_lds + dq_code_words(ipt, k);
	const u64 base = (u64)blockIdx.x * tile;
	if (tid < DQ_CODE_PAD)
		s_code[tid] = 0;
	if (tid == DQ_CODE_PAD)
		s_code[DQ_CODE_PAD + n_sym / 16] = 0; /* the word dq_bits64 names, and does not use, for a window that ends with the staged symbols */
	for (u32 row = 0; row < n_sym; row += DQ_THREADS) { /* one coalesced byte per lane; a wave packs its 64 symbols into 4 code words and 2 mask words */
		const u64 pos = base + row + tid;
		const u32 c = pos < n_bytes ? dq_code(seq[pos]) : 4u;
		const u64 inv = __ballot(c > 3);
		u32 w = (c & 3u) << (30 - 2 * (lane & 15));
#pragma unroll
		for (int o = 1; o < 16; o <<= 1)
			w |= __shfl_down(w, o); /* lanes 0, 16, 32, 48: the OR over their 16 */
		if ((lane & 15) == 0)
			s_code[DQ_CODE_PAD + (row + tid) / 16] = w;
		if (lane == 0) {
			s_inv[(row + tid) / 32] = (u32)inv;
			s_inv[(row + tid) / 32 + 1] = (u32)(inv >> 32);
		}
	}
	__syncthreads();
	const u32 sbytes = (k - p) / 4, rb = sbytes + cbytes, hb = sbytes < 8 ? sbytes : 8;
	const u64 n_pref = 1ull << (2 * p);
	u32 tally[4] = {0, 0, 0, 0};
	for (u32 it = 0; it < ipt; ++it) {
		const u32 o = it * DQ_THREADS + tid;
		const u64 i = base + o;
		if (i >= n_bytes)
			continue;
		u32 cnt = 0;
		if (i + k <= n_bytes) {
			u32 bad = 0;
			const u32 g0 = o >> 5, g1 = (o + k - 1) >> 5;
			for (u32 g = g0; g <= g1; ++g) {
				u32 m = s_inv[g];
				if (g == g0)
					m &= ~0u << (o & 31);
				if (g == g1)
					m &= (2u << ((o + k - 1) & 31)) - 1u;
				bad |= m;
			}
			if (bad)
				++tally[DQ_ST_INVALID];
			else {
				++tally[DQ_ST_VALID];
				u64 x[SIZE];
#pragma unroll
				for (int w = 0; w < SIZE; ++w)
					x[w] = 64u * w < 2 * k ? dq_bits64(s_code, 2 * (o + k) - 64u * w) : 0; /* 2 (o + k) - 64 w > 2 o >= 0 */
				kmc_mask_low<SIZE>(x, 2 * k);
				if (both_strands) {
					u64 rc[SIZE];
					kmc_revcomp<SIZE>(x, k, rc);
					if (!kmc_less<SIZE>(x, rc)) { /* kmer < kmer_rev ? kmer : kmer_rev */
#pragma unroll
						for (int w = 0; w < SIZE; ++w)
							x[w] = rc[w];
					}
				}
				const u64 pref = kmc_remove_suffix<SIZE>(x, 2 * (k - p)) & (n_pref - 1);
				u64 hi = pref + 1 < n_pref ? lut[pref + 1] : n_recs, lo = lut[pref];
				hi = hi < n_recs ? hi : n_recs; /* a LUT that does not ascend finds nothing; it cannot lead outside the records */
				lo = lo < hi ? lo : hi;
				/* the first hb suffix bytes as one number, then byte by byte */
				u64 head = kmc_remove_suffix<SIZE>(x, 8 * (sbytes - hb));
				if (hb < 8)
					head &= (1ull << (8 * hb)) - 1;
				while (lo < hi) {
					const u64 mid = (lo + hi) >> 1;
					const uint8_t *r = recs + mid * rb;
					u64 rh = 0;
					for (u32 q = 0; q < hb; ++q)
						rh = (rh << 8) | r[q];
					int cmp = rh < head ? -1 : rh > head ? 1 : 0;
					for (u32 q = hb; cmp == 0 && q < sbytes; ++q) {
						const u32 pb = sbytes - 1 - q;
						u32 kb = 0;
#pragma unroll
						for (int w = 0; w < SIZE; ++w)
							if ((pb >> 3) == (u32)w)
								kb = (u32)(x[w] >> ((pb & 7) * 8)) & 0xFFu;
						cmp = r[q] < kb ? -1 : r[q] > kb ? 1 : 0;
					}
					if (cmp == 0) {
						u32 c = 0;
						for (u32 q = 0; q < cbytes; ++q)
							c |= (u32)r[sbytes + q] << (8 * q);
						if (c >= cut_min && (u64)c <= cut_max) {
							cnt = c;
							++tally[DQ_ST_FOUND];
						} else
							++tally[DQ_ST_CUT];
						break;
					}
					if (cmp < 0)
						lo = mid + 1;
					else
						hi = mid;
				}
			}
		}
		counters[i] = cnt;
	}
#pragma unroll
	for (int q = 0; q < 4; ++q) {
		const u32 v = wave_sum<u32>(tally[q]);
		if (lane == 0)
			s_tally[tid >> 6][q] = v;
	}
	__syncthreads();
	if (tid < 4) {
		u32 v = 0;
		for (u32 w = 0; w < DQ_THREADS / 64; ++w)
			v += s_tally[w][tid];
		if (v)
			atomicAdd(stats + tid, (u64)v);
	}
}

/* The per-read results, from the counters and the read offsets alone. Reads may be empty or megabases long, so nothing here walks a read: the counters become two bit
 * arrays with a count per 64 positions (PHASE 0), k_db_cumsum turns the counts into prefix sums, and with those a read's non-zero counters are a difference of two sums and
 * its first low window a bisection (PHASE 1: one thread per read, which also checks the read's offsets and terminator), and a base is masked when one of the at most k
 * windows over it — a few words of the bit array — is low (PHASE 2: one thread per byte, its read found by bisection in the offsets).
 *   0: nz_bits / low_bits[c] bit b = counters[64 c + b] != 0 / < threshold, nz_cnt / low_cnt[c] their population
 *   1: n_valid[r], trim_len[r] (either may be nullptr); KERR_CORRUPT for offsets that do not ascend, end behind n_bytes, or a terminator that is a valid symbol
 *   2: masked[i] */
__device__ __forceinline__ u64 dq_rank(const u64 *__restrict__ sums, const u64 *__restrict__ bits, u64 pos) /* set bits in front of position pos, pos <= n_bytes */
{
	const u64 c = pos >> 6;
	return (pos & 63) ? sums[c] + (u64)__popcll(bits[c] & ((1ull << (pos & 63)) - 1)) : sums[c];
}
template <int PHASE>
__global__ void __launch_bounds__(256) k_dbq_reads(const uint8_t *__restrict__ seq, u64 n_bytes, u32 k, const u64 *__restrict__ read_off, u64 n_reads, u32 threshold,
                                                  const u32 *__restrict__ counters, u64 *__restrict__ nz_bits, u64 *__restrict__ low_bits, u64 *__restrict__ nz_cnt,
                                                  u64 *__restrict__ low_cnt /* PHASE 1, 2: the prefix sums of the counts, [chunks + 1] */, u32 *__restrict__ n_valid,
                                                  u32 *__restrict__ trim_len, uint8_t *__restrict__ masked, u32 *__restrict__ err)
{
	const u64 t = (u64)blockIdx.x * 256 + threadIdx.x, n_chunks = (n_bytes + 63) >> 6;
	if (PHASE == 0) {
		if ((t >> 6) >= n_chunks) /* the whole wave */
			return;
		const u32 c = t < n_bytes ? counters[t] : 0u;
		const u64 nz = __ballot(t < n_bytes && c != 0), low = __ballot(t < n_bytes && c < threshold);
		if ((threadIdx.x & 63) == 0) {
			nz_bits[t >> 6] = nz;
			low_bits[t >> 6] = low;
			nz_cnt[t >> 6] = (u64)__popcll(nz);
			low_cnt[t >> 6] = (u64)__popcll(low);
		}
	} else if (PHASE == 1) {
		if (t >= n_reads)
			return;
		const u64 a = read_off[t], b = read_off[t + 1];
		u32 nv = 0, tl = 0;
		if (!(a < b) || b > n_bytes || dq_code(seq[b - 1]) < 4)
			atomicOr(err, KERR_CORRUPT);
		else if (b - 1 - a >= k) {
			const u64 n_win = b - a - k; /* len - k + 1 */
			nv = (u32)(dq_rank(nz_cnt, nz_bits, a + n_win) - dq_rank(nz_cnt, nz_bits, a));
			if (!((low_bits[a >> 6] >> (a & 63)) & 1)) {
				/* the first low window behind the read's first: the first set bit at or behind a + 1 — the chunk where the prefix sums pass the rank of a + 1 */
				const u64 from = a + 1, rank = dq_rank(low_cnt, low_bits, from);
				u64 j = n_win;
				if (low_cnt[n_chunks] > rank) {
					u64 lo = from >> 6, hi = n_chunks - 1; /* smallest chunk c with sums[c + 1] > rank */
					while (lo < hi) {
						const u64 mid = (lo + hi) >> 1;
						if (low_cnt[mid + 1] > rank)
							hi = mid;
						else
							lo = mid + 1;
					}
					u64 w = low_bits[lo];
					if (lo == from >> 6)
						w &= ~0ull << (from & 63);
					const u64 at = (lo << 6) + (u64)(__ffsll(w) - 1);
					j = at - a < n_win ? at - a : n_win;
				}
				tl = k - 1 + (u32)j;
			}
		}
		if (n_valid)
			n_valid[t] = nv;
		if (trim_len)
			trim_len[t] = tl;
	} else {
		if (t >= n_bytes)
			return;
		uint8_t c = seq[t];
		u64 lo = 0, hi = n_reads + 1; /* offsets <= t */
		while (lo < hi) {
			const u64 mid = (lo + hi) >> 1;
			if (read_off[mid] <= t)
				lo = mid + 1;
			else
				hi = mid;
		}
		if (lo >= 1 && lo <= n_reads) {
			const u64 a = read_off[lo - 1], b = read_off[lo];
			if (a <= t && t + 1 < b && b <= n_bytes && b - 1 - a >= k) { /* a base of a read of at least k symbols: the windows a + max(j - k + 1, 0) .. a + min(j, n_win - 1) */
				const u64 j = t - a, n_win = b - a - k;
				const u64 w0 = a + (j + 1 > k ? j + 1 - k : 0), w1 = a + (j < n_win - 1 ? j : n_win - 1);
				u64 any = 0;
				for (u64 g = w0 >> 6; g <= (w1 >> 6); ++g) {
					u64 m = low_bits[g];
					if (g == (w0 >> 6))
						m &= ~0ull << (w0 & 63);
					if (g == (w1 >> 6))
						m &= (2ull << (w1 & 63)) - 1;
					any |= m;
				}
				if (any)
					c = 'N';
			}
		}
		masked[t] = c;
	}
}

/* ---- one database transformed (`kmc_tools transform`: reduce / compact / set_counts / sort, histogram, dump) ----
 * reduce     k_db_unpack (every record present), k_tr_compact<false> counts the records of every tile the cutoffs keep and the tallies, k_db_cumsum scans the counts,
 *            k_tr_compact<true> writes the kept records — clamped, or with the count of set_counts — at their offsets (a stable compaction: the order stays), k_db_pack
 * histogram  k_tr_hist: the counters read straight from the packed records; the bins of a workgroup in LDS while the range fits (equal counters of a wave combined
 *            before the LDS atomic, one flush per workgroup), 64-bit atomics on the bins in HBM otherwise
 * dump       k_tr_dump<false> counts the text bytes of every tile, k_db_cumsum scans them, k_tr_dump<true> formats the tile's text into LDS and copies it out */
#ifndef TR_THREADS
#define TR_THREADS 256 /* threads of a k_tr_* workgroup */
#endif
constexpr u32 TR_REDUCE_IPT = 1;        /* consecutive records per thread of k_tr_compact: a tile is TR_THREADS x this many (1: neighbouring lanes read neighbouring records) */
/* bins k_tr_hist keeps in LDS: 40 KiB of 32-bit bins, four workgroups (16 waves) on a CU's 160 KiB, and the whole default range of `kmc_tools transform histogram`
 * (-cx 10000, parameters_parser.cpp:884) */
constexpr u32 TR_HIST_LDS_BINS = 10240;
constexpr u32 TR_HIST_PEEL = 2;         /* rounds in which a wave combines the lanes that hold its first active lane's counter; what is left adds lane by lane */
constexpr u32 TR_HIST_MAX_GROUPS = 1024; /* workgroups of k_tr_hist: each flushes its bins once */
constexpr u32 TR_IMAGE_BYTES = 32 * 1024; /* a dump tile's text by default: four workgroups on a CU */
constexpr u32 TR_IMAGE_MAX = 64 * 1024 - 64; /* the most an override may ask for (with the 16 bytes of alignment slack in front) */
constexpr u32 TR_REC_EXTRA = 12;        /* '\t', ten digits, '\n': a record of the dump is at most kmer_len + 12 bytes */
enum : u32 { TR_ST_CUT_IN = 0, TR_ST_BELOW_MIN = 1, TR_ST_ABOVE_MAX = 2, TR_ST_WRITTEN = 3 };
constexpr u32 tr_default_tile(u32 k) { return TR_IMAGE_BYTES / (k + TR_REC_EXTRA) ? TR_IMAGE_BYTES / (k + TR_REC_EXTRA) : 1u; }
constexpr size_t tr_dump_lds_bytes(u32 tile, u32 k) { return (size_t)tile * (k + TR_REC_EXTRA) + 16; }

struct TrCut {
	u32 in_min;
	u64 in_max; /* the input's cutoffs: a record outside them is absent (kmc1_db_reader.h:574-576, kmc2_db_reader.h:1812) */
	u32 out_min;
	u64 out_max;
	u32 counter_max, counter_value; /* of the output; counter_value != 0: set_counts */
};

/* the readers' and the writers' rule for one counter: 0 kept (c: what is written), TR_ST_CUT_IN + 1, TR_ST_BELOW_MIN + 1, TR_ST_ABOVE_MAX + 1 otherwise
 * (kmc1_db_writer.h:378-385, dump_writer.h:145-148) */
__device__ __forceinline__ u32 tr_classify(u32 &c, const TrCut &cut)
{
	if (c < cut.in_min || (u64)c > cut.in_max)
		return TR_ST_CUT_IN + 1;
	if (cut.counter_value) {
		c = cut.counter_value;
		return 0;
	}
	if (c < cut.out_min)
		return TR_ST_BELOW_MIN + 1;
	if ((u64)c > cut.out_max)
		return TR_ST_ABOVE_MAX + 1;
	if (c > cut.counter_max)
		c = cut.counter_max;
	return 0;
}

__device__ __forceinline__ u32 tr_counter(const uint8_t *__restrict__ r, u32 cbytes) /* counter bytes, least significant first */
{
	u32 c = 0;
	for (u32 q = 0; q < cbytes; ++q)
		c |= (u32)r[q] << (8 * q);
	return c;
}

__device__ __forceinline__ void tr_add_tallies(const u32 mine[3], u64 *__restrict__ stats)
{
#pragma unroll
	for (int q = 0; q < 3; ++q) {
		const u32 v = wave_sum<u32>(mine[q]);
		if ((threadIdx.x & 63) == 0 && v)
			atomicAdd(stats + q, (u64)v);
	}
}

/* WRITE = false: tile_count[tile] = records of the tile that are kept, stats[0..2] += the tile's tallies. WRITE = true: the kept records, in their order, to
 * out[tile_base[tile] ..] with the count that is written. */
template <int SIZE, bool WRITE>
__global__ void __launch_bounds__(TR_THREADS) k_tr_compact(const u64 *__restrict__ recs /* [n][SIZE + 1] */, u64 n, TrCut cut, const u64 *__restrict__ tile_base, u64 *__restrict__ tile_count,
                                                          u64 *__restrict__ out, u64 *__restrict__ stats)
{
	constexpr int W = SIZE + 1;
	__shared__ u32 s_scan[TR_THREADS / 64 + 1];
	const u64 j0 = ((u64)blockIdx.x * TR_THREADS + threadIdx.x) * TR_REDUCE_IPT;
	u32 kept = 0, keep_bits = 0, cnt[TR_REDUCE_IPT], mine[3] = {0, 0, 0};
#pragma unroll
	for (u32 q = 0; q < TR_REDUCE_IPT; ++q) {
		cnt[q] = 0;
		if (j0 + q < n) {
			cnt[q] = (u32)recs[(j0 + q) * W + SIZE];
			const u32 cls = tr_classify(cnt[q], cut);
			if (cls)
				mine[cls - 1] += 1;
			else {
				keep_bits |= 1u << q;
				++kept;
			}
		}
	}
	u32 total;
	const u32 first = block_excl_sum<TR_THREADS / 64, u32>(kept, s_scan, total);
	if (!WRITE) {
		tr_add_tallies(mine, stats);
		if (threadIdx.x == 0)
			tile_count[blockIdx.x] = total;
		return;
	}
	u64 *o = out + (tile_base[blockIdx.x] + first) * W;
#pragma unroll
	for (u32 q = 0; q < TR_REDUCE_IPT; ++q)
		if (keep_bits & (1u << q)) {
			const u64 *r = recs + (j0 + q) * W;
#pragma unroll
			for (int w = 0; w < SIZE; ++w)
				o[w] = r[w];
			o[SIZE] = cnt[q];
			o += W;
		}
}

/* hist[c - lo] += 1 for every record whose counter c lies inside the input's cutoffs and in [lo, hi]; stats[0] += cut by the input, [1] += outside [lo, hi], [2] += counted.
 * LDS_BINS: n_bins <= TR_HIST_LDS_BINS 32-bit bins in dynamic LDS (a workgroup sees fewer than 2^32 records). */
template <bool LDS_BINS>
__global__ void __launch_bounds__(TR_THREADS) k_tr_hist(const uint8_t *__restrict__ recs, u64 n, u32 sbytes, u32 cbytes, u32 in_min, u64 in_max, u32 lo, u64 hi, u32 n_bins,
                                                       u64 *__restrict__ hist, u64 *__restrict__ stats)
{
	KMC_DYN_LDS(u32, s_bins);
	const u32 tid = threadIdx.x, lane = tid & 63;
	if (LDS_BINS) {
		for (u32 i = tid; i < n_bins; i += TR_THREADS)
			s_bins[i] = 0;
		__syncthreads();
	}
	const u64 stride = (u64)gridDim.x * TR_THREADS, rounds = (n + stride - 1) / stride; /* every lane makes every round: the wave votes together */
	const u32 rb = sbytes + cbytes;
	u32 mine[3] = {0, 0, 0};
	for (u64 r = 0; r < rounds; ++r) {
		const u64 j = r * stride + (u64)blockIdx.x * TR_THREADS + tid;
		u32 c = 0;
		bool active = false;
		if (j < n) {
			c = tr_counter(recs + j * rb + sbytes, cbytes);
			if (c < in_min || (u64)c > in_max)
				mine[0] += 1;
			else if (c < lo || (u64)c > hi)
				mine[1] += 1;
			else {
				mine[2] += 1;
				active = true;
			}
		}
		const u32 bin = c - lo;
		for (u32 peel = 0; peel < TR_HIST_PEEL; ++peel) {
			const u64 todo = __ballot(active);
			if (!todo)
				break;
			const int leader = __ffsll(todo) - 1;
			const u32 lbin = __shfl(bin, leader);
			const u64 same = __ballot(active && bin == lbin);
			if ((int)lane == leader) {
				if (LDS_BINS)
					atomicAdd(s_bins + lbin, (u32)__popcll(same));
				else
					atomicAdd(hist + lbin, (u64)__popcll(same));
			}
			if (bin == lbin)
				active = false;
		}
		if (active) {
			if (LDS_BINS)
				atomicAdd(s_bins + bin, 1u);
			else
				atomicAdd(hist + bin, (u64)1);
		}
	}
	tr_add_tallies(mine, stats);
	if (LDS_BINS) {
		__syncthreads();
		for (u32 i = tid; i < n_bins; i += TR_THREADS) {
			const u32 v = s_bins[i];
			if (v)
				atomicAdd(hist + i, (u64)v);
		}
	}
}

struct TrDump {
	u32 k, p, sbytes, cbytes;
	u32 n_entries; /* of the LUT: segments x 4^p (a KMC1 body: one segment; a KMC2 body: one per bin, the entries global record offsets) */
	u32 tile;      /* records of a tile */
};
struct __attribute__((aligned(16))) TrVec16 {
	u64 a, b;
};

__device__ __forceinline__ u32 tr_digits(u32 v)
{
	return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
__device__ __forceinline__ uint8_t tr_symbol(u32 x) { return (uint8_t)(0x54474341u >> (8 * (x & 3))); } /* "ACGT" */

/* Records [first, first + count) of the body as text, `<k symbols>\t<decimal counter>\n` per record the cutoffs keep (dump_writer.h:111-160), in record order.
 * WRITE = false: tile_bytes[tile] = text bytes of the tile, stats[0..2] += its tallies. WRITE = true: the tile's text to text[tile_base[tile] ..). A thread takes
 * ceil(tile / TR_THREADS) consecutive records; the prefix of its first one is found by bisection of the LUT (the last entry <= the record's number; in a segmented
 * LUT the prefix is that entry's index modulo 4^p, kmc2_db_reader.h:1776-1791), the following ones by walking on. The text is built in LDS at the byte offset the
 * tile's first byte has inside its 16 bytes of HBM, so that whole aligned 16-byte pieces go out; the bytes in front of the first piece and behind the last one are
 * written one by one. Nothing outside text[tile_base[tile] .. tile_base[tile + 1]) is written. */
template <bool WRITE>
__global__ void __launch_bounds__(TR_THREADS) k_tr_dump(const uint8_t *__restrict__ recs, const u64 *__restrict__ lut, u64 first, u64 count, TrDump d, TrCut cut, const u64 *__restrict__ tile_base,
                                                       u64 *__restrict__ tile_bytes, uint8_t *__restrict__ text, u64 *__restrict__ stats)
{
	KMC_DYN_LDS(uint8_t, s_img);
	__shared__ u32 s_scan[TR_THREADS / 64 + 1];
	const u32 tid = threadIdx.x, ipt = (d.tile + TR_THREADS - 1) / TR_THREADS, rb = d.sbytes + d.cbytes;
	const u64 l0 = (u64)blockIdx.x * d.tile;
	const u32 len = (u32)(count - l0 < (u64)d.tile ? count - l0 : (u64)d.tile);
	const u32 m0 = tid * ipt < len ? tid * ipt : len, m1 = m0 + ipt < len ? m0 + ipt : len;
	u32 bytes = 0, mine[3] = {0, 0, 0};
	for (u32 m = m0; m < m1; ++m) {
		u32 c = tr_counter(recs + (first + l0 + m) * rb + d.sbytes, d.cbytes);
		const u32 cls = tr_classify(c, cut);
		if (cls)
			mine[cls - 1] += 1;
		else
			bytes += d.k + 2 + tr_digits(c);
	}
	u32 total;
	u32 off = block_excl_sum<TR_THREADS / 64, u32>(bytes, s_scan, total);
	if (!WRITE) {
		tr_add_tallies(mine, stats);
		if (tid == 0)
			tile_bytes[blockIdx.x] = total;
		return;
	}
	uint8_t *dst = text + tile_base[blockIdx.x];
	const u32 mis = (u32)((size_t)dst & 15);
	uint8_t *img = s_img + mis;
	if (m0 < m1) {
		const u64 ja = first + l0 + m0;
		u32 lo = 0, hi = d.n_entries; /* the last entry <= ja (entry 0 is 0) */
		while (hi - lo > 1) {
			const u32 mid = (lo + hi) >> 1;
			if (lut[mid] <= ja)
				lo = mid;
			else
				hi = mid;
		}
		const u32 pmask = (1u << (2 * d.p)) - 1;
		for (u32 m = m0; m < m1; ++m) {
			const u64 j = ja + (m - m0);
#pragma unroll 1
			while (lo + 1 < d.n_entries && lut[lo + 1] <= j)
				++lo;
			const uint8_t *r = recs + j * rb;
			u32 c = tr_counter(r + d.sbytes, d.cbytes);
			if (tr_classify(c, cut))
				continue;
			uint8_t *o = img + off;
			const u32 prefix = lo & pmask;
#pragma unroll 1
			for (u32 q = 0; q < d.p; ++q)
				*o++ = tr_symbol(prefix >> (2 * (d.p - 1 - q)));
#pragma unroll 1
			for (u32 q = 0; q < d.sbytes; ++q) {
				const u32 b = r[q];
				o[0] = tr_symbol(b >> 6);
				o[1] = tr_symbol(b >> 4);
				o[2] = tr_symbol(b >> 2);
				o[3] = tr_symbol(b);
				o += 4;
			}
			*o++ = '\t';
			const u32 nd = tr_digits(c);
#pragma unroll 1
			for (u32 q = nd; q > 0; --q) { /* c / 10 as a multiplication: 0xCCCCCCCD = ceil(2^35 / 10) */
				const u32 tenth = (u32)(((u64)c * 0xCCCCCCCDull) >> 35);
				o[q - 1] = (uint8_t)('0' + (c - tenth * 10u));
				c = tenth;
			}
			o[nd] = '\n';
			off += d.k + 2 + nd;
		}
	}
	__syncthreads();
	const u32 head = total < ((16u - mis) & 15u) ? total : ((16u - mis) & 15u), n_vec = (total - head) / 16, tail0 = head + n_vec * 16;
	for (u32 i = tid; i < head; i += TR_THREADS)
		dst[i] = img[i];
	const TrVec16 *src16 = reinterpret_cast<const TrVec16 *>(img + head);
	TrVec16 *dst16 = reinterpret_cast<TrVec16 *>(dst + head);
	for (u32 i = tid; i < n_vec; i += TR_THREADS)
		dst16[i] = src16[i];
	for (u32 i = tail0 + tid; i < total; i += TR_THREADS)
		dst[i] = img[i];
}

/* ---- a set expression over several ordered databases (`kmc_tools complex`) ----
 * kmc_tools/operations.h:40-256 (the nodes), expression_node.h (the tree), kmc1_db_writer.h:382-385 (the root). Every operation is pointwise per k-mer: whether a
 * k-mer is in a node's result, and with which counter, depends only on whether it is in the node's two children and with which counters. So the key space is cut into
 * tiles, every LEAF's (occurrence of an input in the expression) slice of a tile is brought into LDS, and the postfix program is walked once per record.
 *
 * k_cx_partition. Every S-th record of every leaf (indices 0, S, 2S, ...) is a sample. Samples are ordered by (key, leaf); a sample's rank is the number of samples in
 * front of it, found by one binary search per leaf. Every M-th sample by rank is a splitter and writes, per leaf, the lower bound of its key. Tile t holds the keys in
 * [splitter t, splitter t + 1) (the last tile: everything from its splitter on), so (i) equal keys lie in one tile and every slice is a lower-bound range.
 * (ii), (iii): a tile's slices hold at most S (M + 2L - 1) - L records, L the number of leaves. Proof. Let the tile be the keys in [x_a, x_b), its splitters' ranks r_a and
 * r_b = r_a + M. A sample with a key in that range sorts before (x_b, leaf of b), so its rank is below r_b; if its rank is below r_a its key is x_a and its leaf lies in
 * front of a's leaf — keys are distinct inside a leaf, so there are at most L - 1 of those. The range holds at most M + L - 1 samples. Leaf l's slice is a run of
 * record indices that holds m_l multiples of S, hence at most (m_l + 1) S - 1 records (it starts behind the multiple in front and ends before the next one).
 * Summed: S (sum of m_l + L) - L <= S (M + 2L - 1) - L. The host takes M = 2L and S = (T + L) / (4L - 1): never more than T records (half of T on average).
 * The rank-0 sample is the smallest record of all, so tile 0 starts at record 0 of every leaf.
 *
 * k_cx_tile. LDS: the slices, T records of SIZE + 1 words, and (WRITE) one 64-bit word per merged rank. The default T keeps both at 32 KiB together for every record
 * width (cx_default_tile: 1365 records of one key word ... 455 of seven) — five workgroups on a CU's 160 KiB; $KMC_HIP_EXPR_TILE overrides downwards (not below
 * CX_MIN_TILE). A tile whose slices hold more than T records writes nothing and raises stats[CX_ST_FLAG]: LDS is never overrun.
 * The value stack is a presence bit mask and a register array that is SHIFTED on every push and pop, so every index is static: no scratch. */
#ifndef CX_THREADS
#define CX_THREADS 256 /* threads of a k_cx_tile workgroup */
#endif
/* leaf occurrences of an expression (KMC_HIP_DB_EXPR_MAX_LEAVES). 16: the stack of a right-deep tree is then 16 registers, the leaves' pointers and lengths 256 bytes of
 * kernel arguments, and at the narrowest default tile (455 records) S is still 7 */
constexpr u32 CX_MAX_LEAVES = 16;
constexpr u32 CX_MAX_STEPS = 2 * CX_MAX_LEAVES - 1;
constexpr u32 CX_MIN_TILE = 64; /* >= 3 L - 1 for L = 16: S >= 1 */
constexpr u32 CX_INPUT = 16;    /* KMC_HIP_DB_EXPR_INPUT */
enum : u32 { CX_ST_KEYS = 0, CX_ST_RESULT = 1, CX_ST_BELOW_MIN = 2, CX_ST_ABOVE_MAX = 3, CX_ST_FLAG = 5 };
template <int SIZE> constexpr u32 cx_default_tile() { return 32 * 1024 / ((SIZE + 2) * 8); }
template <int SIZE> constexpr size_t cx_lds_bytes(u32 tile, bool write) { return (size_t)tile * (SIZE + 1) * 8 + (write ? (size_t)tile * 8 : 0); }

struct CxLeaves {
	const u64 *rec[CX_MAX_LEAVES]; /* the leaf's input, unpacked */
	u64 n[CX_MAX_LEAVES];
	u64 first_sample[CX_MAX_LEAVES + 1]; /* samples of the leaves in front */
	u32 n_leaves;
};
struct CxProg {
	u32 n_steps;
	u32 step[CX_MAX_STEPS]; /* CX_INPUT, or SO_INTERSECT | SO_UNION | SO_KMERS_SUBTRACT | SO_COUNTERS_SUBTRACT, the counter mode << 8 */
};
struct CxOut {
	u32 cutoff_min, counter_max;
	u64 cutoff_max;
};

/* records of s[0 .. n) with a key below x */
template <int SIZE> __device__ __forceinline__ u64 cx_lower_bound(const u64 *s, u64 n, const u64 *x)
{
	u64 lo = 0, hi = n;
	while (lo < hi) {
		const u64 mid = (lo + hi) >> 1;
		if (so_less<SIZE>(s + mid * (SIZE + 1), x))
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

template <int SIZE>
__global__ void __launch_bounds__(256) k_cx_partition(CxLeaves lv, u32 S, u32 M, u64 n_samples, u64 n_tiles, u64 *__restrict__ bounds /* [n_tiles + 1][n_leaves] */)
{
	constexpr int W = SIZE + 1;
	const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
	const u32 L = lv.n_leaves;
	if (g < L)
		bounds[n_tiles * L + g] = lv.n[g]; /* the end of the last tile */
	if (g >= n_samples)
		return;
	u32 mine = 0;
	while (mine + 1 < L && g >= lv.first_sample[mine + 1])
		++mine;
	const u64 j = g - lv.first_sample[mine];
	u64 x[SIZE];
	{
		const u64 *r = lv.rec[mine] + j * S * W;
#pragma unroll
		for (int w = 0; w < SIZE; ++w)
			x[w] = r[w];
	}
	u64 rank = j;
	for (u32 l = 0; l < L; ++l) {
		if (l == mine)
			continue;
		u64 lb = cx_lower_bound<SIZE>(lv.rec[l], lv.n[l], x);
		if (l < mine && lb < lv.n[l] && so_equal<SIZE>(lv.rec[l] + lb * W, x))
			++lb; /* a leaf in front: its sample of the same key sorts before this one */
		rank += (lb + S - 1) / S; /* samples at the indices 0, S, .. below lb */
	}
	if (rank % M)
		return;
	u64 *o = bounds + rank / M * L;
	for (u32 l = 0; l < L; ++l)
		o[l] = l == mine ? j * S : cx_lower_bound<SIZE>(lv.rec[l], lv.n[l], x);
}

/* one operation node on (present, counter) of its children: C2ArgOper::EqualsToOuputBundle for a pair (DIFF with c1 <= c2 inserts nothing), the loops of
 * CUnion / CIntersection / CKmersSubtract / CCountersSubtract for what is in one child only */
__device__ __forceinline__ bool cx_node(u32 kind, u32 mode, bool p1, u32 c1, bool p2, u32 c2, u32 &c)
{
	if (p1 && p2) {
		c = so_counter(mode, c1, c2);
		return kind != SO_KMERS_SUBTRACT && !(mode == SO_CNT_DIFF && c1 <= c2);
	}
	c = p1 ? c1 : c2;
	return p1 ? kind != SO_INTERSECT : (p2 && kind == SO_UNION);
}

/* WRITE = false: tile_count[tile] = records the tile keeps, stats[0..3] += its tallies. WRITE = true: the kept records, in key order, to out[tile_base[tile] ..]. */
template <int SIZE, bool WRITE>
__global__ void __launch_bounds__(CX_THREADS) k_cx_tile(CxLeaves lv, CxProg pg, const u64 *__restrict__ bounds, u32 T, CxOut wr, const u64 *__restrict__ tile_base,
                                                       u64 *__restrict__ tile_count, u64 *__restrict__ out, u64 out_cap /* records */, u64 *__restrict__ stats)
{
	constexpr int W = SIZE + 1;
	KMC_DYN_LDS(u64, cx_lds);
	__shared__ u32 s_off[CX_MAX_LEAVES + 1];
	__shared__ u32 s_scan[CX_THREADS / 64 + 1];
	__shared__ u32 s_bad;
	const u32 tid = threadIdx.x, L = lv.n_leaves;
	const u64 t = blockIdx.x;
	const u64 *b0 = bounds + t * L, *b1 = b0 + L;
	u64 *s_rec = cx_lds, *s_slot = cx_lds + (size_t)T * W;
	if (tid == 0) {
		u32 off = 0, bad = 0;
		for (u32 l = 0; l < L; ++l) {
			const u64 lo = b0[l], hi = b1[l];
			s_off[l] = off;
			if (hi < lo || hi > lv.n[l] || hi - lo > (u64)(T - off))
				bad = 1;
			else
				off += (u32)(hi - lo);
		}
		s_off[L] = off;
		s_bad = bad;
	}
	__syncthreads();
	if (s_bad) { /* more than the LDS was sized for: nothing is read or written, the entry reports it */
		if (tid == 0) {
			atomicOr((unsigned long long *)(stats + CX_ST_FLAG), 1ull);
			if (!WRITE)
				tile_count[t] = 0;
		}
		return;
	}
	const u32 total = s_off[L];
	for (u32 l = 0; l < L; ++l) { /* runs of whole records: flat, coalesced copies */
		const u64 *src = lv.rec[l] + b0[l] * W;
		u64 *dst = s_rec + (size_t)s_off[l] * W;
		const u32 words = (s_off[l + 1] - s_off[l]) * W;
		for (u32 g = tid; g < words; g += CX_THREADS)
			dst[g] = src[g];
	}
	if (WRITE)
		for (u32 g = tid; g < total; g += CX_THREADS)
			s_slot[g] = 0;
	__syncthreads();
	u32 n_keys = 0, n_result = 0, n_below = 0, n_above = 0, kept = 0;
	for (u32 r = tid; r < total; r += CX_THREADS) {
		u32 mine = 0;
		while (r >= s_off[mine + 1])
			++mine;
		u64 x[SIZE];
#pragma unroll
		for (int w = 0; w < SIZE; ++w)
			x[w] = s_rec[(size_t)r * W + w];
		u32 cnt[CX_MAX_LEAVES]; /* the value stack, top at [0]; bit d of pmask: the value at depth d is present */
#pragma unroll
		for (u32 d = 0; d < CX_MAX_LEAVES; ++d)
			cnt[d] = 0;
		u32 pmask = 0, rank = 0, leaf = 0;
		bool earlier = false, any = false;
		for (u32 i = 0; i < pg.n_steps; ++i) {
			const u32 kind = pg.step[i] & 0xFFu, mode = pg.step[i] >> 8;
			if (kind == CX_INPUT) {
				const u32 l = leaf++, base = s_off[l], n = s_off[l + 1] - base;
				const u64 *sl = s_rec + (size_t)base * W;
				u32 lb = (u32)cx_lower_bound<SIZE>(sl, n, x);
				bool hit = lb < n && so_equal<SIZE>(sl + (size_t)lb * W, x);
				if (l == mine) {
					lb = r - base;
					hit = true;
				}
				const u64 c = hit ? sl[(size_t)lb * W + SIZE] : SO_ABSENT;
				const bool present = c != SO_ABSENT;
				rank += lb + (l < mine && hit ? 1u : 0u); /* equal keys order by leaf */
				earlier = earlier || (l < mine && hit);
				any = any || present;
#pragma unroll
				for (u32 d = CX_MAX_LEAVES - 1; d > 0; --d)
					cnt[d] = cnt[d - 1];
				cnt[0] = present ? (u32)c : 0u;
				pmask = (pmask << 1) | (present ? 1u : 0u);
			} else {
				u32 c;
				const bool p = cx_node(kind, mode, (pmask & 2u) != 0, cnt[1], (pmask & 1u) != 0, cnt[0], c);
#pragma unroll
				for (u32 d = 1; d + 1 < CX_MAX_LEAVES; ++d)
					cnt[d] = cnt[d + 1];
				cnt[0] = c;
				pmask = ((pmask >> 2) << 1) | (p ? 1u : 0u);
			}
		}
		if (earlier) /* not the head of its key's run */
			continue;
		n_keys += any ? 1u : 0u;
		if (!(pmask & 1u))
			continue;
		++n_result;
		u32 c = cnt[0];
		if (c < wr.cutoff_min) /* kmc1_db_writer.h:382-385 */
			++n_below;
		else if ((u64)c > wr.cutoff_max)
			++n_above;
		else {
			++kept;
			if (c > wr.counter_max)
				c = wr.counter_max;
			if (WRITE)
				s_slot[rank] = (u64)c << 32 | (r + 1);
		}
	}
	if (!WRITE) {
		const u32 mine4[5] = {n_keys, n_result, n_below, n_above, kept};
		u32 sums[5];
#pragma unroll
		for (int q = 0; q < 5; ++q)
			sums[q] = wave_sum<u32>(mine4[q]);
		if ((tid & 63) == 0) {
#pragma unroll
			for (int q = 0; q < 4; ++q)
				if (sums[q])
					atomicAdd((unsigned long long *)(stats + q), (unsigned long long)sums[q]);
			s_scan[tid >> 6] = sums[4];
		}
		__syncthreads();
		if (tid == 0) {
			u32 all = 0;
			for (u32 q = 0; q < CX_THREADS / 64; ++q)
				all += s_scan[q];
			tile_count[t] = all;
		}
		return;
	}
	__syncthreads();
	/* compaction in key order: a thread owns a run of merged ranks */
	const u32 chunk = (total + CX_THREADS - 1) / CX_THREADS;
	const u32 p0 = tid * chunk < total ? tid * chunk : total, p1 = p0 + chunk < total ? p0 + chunk : total;
	u32 have = 0;
	for (u32 p = p0; p < p1; ++p)
		have += s_slot[p] ? 1u : 0u;
	u32 all;
	const u32 first = block_excl_sum<CX_THREADS / 64, u32>(have, s_scan, all);
	const u64 base = tile_base[t];
	if (base + all > out_cap) { /* inputs that are not ordered sets: more than the tree's bound */
		if (tid == 0)
			atomicOr((unsigned long long *)(stats + CX_ST_FLAG), 2ull);
		return;
	}
	u64 *o = out + (base + first) * W;
	for (u32 p = p0; p < p1; ++p) {
		const u64 v = s_slot[p];
		if (!v)
			continue;
		const u64 *src = s_rec + (size_t)((u32)v - 1) * W;
#pragma unroll
		for (int w = 0; w < SIZE; ++w)
			o[w] = src[w];
		o[SIZE] = v >> 32;
		o += W;
	}
}

/* ---- two ordered databases compared (`kmc_tools compare`) ----
 * Both bodies through k_db_unpack (every record present), k_tr_compact<false> counts what each input's cutoffs remove; an input that lost records is made dense by
 * k_db_cumsum and k_tr_compact<true>, an input that lost nothing is dense already. Then
 *   k_db_compare         flat over the min(na, nb) x (SIZE + 1) words of the two dense arrays: the smallest record that holds a differing word, by one atomicMin per
 *                        wave that saw one
 *   k_db_compare_finish  one workgroup: the kind of the difference from the two records at the minimum (the counter first, CComparer::Equals), the counters, and the
 *                        records' numbers in the bodies (the compaction's tile sums, then one scan over the tile's 256 records) */
#ifndef DC_THREADS
#define DC_THREADS 256 /* threads of a k_db_compare workgroup */
#endif
constexpr u32 DC_STEPS_LOG2 = 3;     /* words per thread of a tile, log2: 2048 words = 16 KiB of either input per workgroup */
constexpr u32 DC_STEPS_LOG2_MAX = 8;
constexpr u64 DC_NONE = ~0ull;       /* no difference seen */
enum : u32 { DC_EQUAL = 0, DC_COUNTER = 1, DC_KMER = 2, DC_A_ENDED = 3, DC_B_ENDED = 4 };

/* first: DC_NONE before the launch, the smallest record index with a differing word after it. A tile is 2^tile_shift words. A wave whose tile starts behind the
 * tile in which the published minimum's record starts leaves at once (the value lane 0 read, for the whole wave): every record with a word in it is larger (a record that straddles into the minimum's own tile
 * from the one before starts there, and may be smaller: that tile is walked). Wave-level operations stand outside the loop: its trip count differs between lanes. */
template <int SIZE>
__global__ void __launch_bounds__(DC_THREADS) k_db_compare(const u64 *__restrict__ a, const u64 *__restrict__ b, u64 n_words, u32 tile_shift, u32 reversed, u64 *__restrict__ first)
{
	constexpr u64 W = SIZE + 1;
	const u64 tile = reversed ? (u64)(gridDim.x - 1 - blockIdx.x) : (u64)blockIdx.x;
	const u64 seen = __shfl(ld_agent(first), 0); /* one value per wave: its lanes leave together or stay together for the ballot and the shuffles below */
	if (seen != DC_NONE && ((seen * W) >> tile_shift) < tile)
		return;
	const u64 w0 = tile << tile_shift, w1 = w0 + (1ull << tile_shift) < n_words ? w0 + (1ull << tile_shift) : n_words;
	u64 mine = DC_NONE;
#pragma unroll 4
	for (u64 w = w0 + threadIdx.x; w < w1; w += DC_THREADS) {
		const u64 x = a[w], y = b[w];
		if (x != y && mine == DC_NONE)
			mine = w; /* ascending: a thread's first is its smallest */
	}
	if (__ballot(mine != DC_NONE) == 0)
		return;
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const u64 t = __shfl_down(mine, o);
		mine = t < mine ? t : mine;
	}
	if ((threadIdx.x & 63) == 0)
		atomicMin((unsigned long long *)first, (unsigned long long)(mine / W));
}

struct DcInput {
	const u64 *dense;     /* [n][SIZE + 1]: the present records */
	u64 n;
	const u64 *body;      /* [n_body][SIZE + 1]: every record of the body, as k_db_unpack left it */
	u64 n_body;
	const u64 *tile_base; /* nullptr: nothing was cut, dense is body; otherwise the present records in front of every tile of TR_THREADS x TR_REDUCE_IPT records [n_tiles + 1] */
	u64 n_tiles;
	u32 cut_min;
	u64 cut_max;
};

/* the number in the body of the present record `i` (all threads of the workgroup call; the answer lands in *s_rec) */
template <int SIZE> __device__ __forceinline__ void dc_locate(const DcInput &in, u64 i, bool any, u32 *s_scan, u64 *s_rec)
{
	constexpr u64 W = SIZE + 1;
	if (!any || i >= in.n || !in.tile_base) {
		if (threadIdx.x == 0)
			*s_rec = !any ? 0 : i >= in.n ? in.n_body : i;
		return;
	}
	u64 lo = 0, hi = in.n_tiles; /* the last tile with tile_base[t] <= i holds record i (tiles in front of it with the same sum keep nothing; tile_base[n_tiles] = n > i) */
	while (hi - lo > 1) {
		const u64 mid = (lo + hi) >> 1;
		if (in.tile_base[mid] <= i)
			lo = mid;
		else
			hi = mid;
	}
	const u64 r = lo * (TR_THREADS * TR_REDUCE_IPT) + threadIdx.x;
	u32 present = 0;
	if (threadIdx.x < TR_THREADS * TR_REDUCE_IPT && r < in.n_body) {
		const u32 c = (u32)in.body[r * W + SIZE];
		present = c >= in.cut_min && (u64)c <= in.cut_max;
	}
	u32 total;
	const u32 before = block_excl_sum<TR_THREADS / 64, u32>(present, s_scan, total);
	if (present && in.tile_base[lo] + before == i)
		*s_rec = r;
}

template <int SIZE> __global__ void __launch_bounds__(TR_THREADS) k_db_compare_finish(DcInput A, DcInput B, const u64 *__restrict__ first, u64 *__restrict__ result /* [8] */)
{
	static_assert(TR_REDUCE_IPT == 1, "dc_locate scans one record per thread");
	constexpr u64 W = SIZE + 1;
	__shared__ u32 s_scan[TR_THREADS / 64 + 1];
	__shared__ u64 s_rec[2];
	const u64 f = *first, n = A.n < B.n ? A.n : B.n;
	u32 kind;
	u64 i;
	if (f != DC_NONE) {
		i = f;
		kind = A.dense[i * W + SIZE] != B.dense[i * W + SIZE] ? DC_COUNTER : DC_KMER;
	} else if (A.n == B.n) {
		i = 0;
		kind = DC_EQUAL;
	} else {
		i = n;
		kind = A.n < B.n ? DC_A_ENDED : DC_B_ENDED;
	}
	dc_locate<SIZE>(A, i, kind != DC_EQUAL, s_scan, s_rec);
	__syncthreads();
	dc_locate<SIZE>(B, i, kind != DC_EQUAL, s_scan, s_rec + 1);
	__syncthreads();
	if (threadIdx.x == 0) {
		result[0] = kind;
		result[1] = i;
		result[2] = A.n;
		result[3] = B.n;
		result[4] = kind != DC_EQUAL && i < A.n ? A.dense[i * W + SIZE] : 0;
		result[5] = kind != DC_EQUAL && i < B.n ? B.dense[i * W + SIZE] : 0;
		result[6] = s_rec[0];
		result[7] = s_rec[1];
	}
}

#endif
