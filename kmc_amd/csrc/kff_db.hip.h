/*
 * kmc_amd/csrc/kff_db.hip.h — a KFF file's records as a database body on the device (gfx950, wave64): what kmc_tools' KFF readers do on the CPU
 * (kmc_tools/kff_db_reader.h:929-1112 the priority-queue merge over the sections, :1320-1492 the sequential reader; the container: kmc_core/kff_writer.cpp,
 * kmc_tools/kff_info_reader.cpp).
 *
 * A KFF record of the files read here (`max` = 1: no per-block count) is ceil(k/4) bytes of k-mer, most significant first and right-aligned (k % 4 != 0: the top bits
 * of the first byte are padding), then data_size counter bytes, MOST significant first (kff_db_reader.h:374-401). A database record for lut_prefix_len p with
 * (k - p) % 4 == 0 is the last (k - p) / 4 of those k-mer bytes verbatim and the counter bytes reversed; the leading ceil(k/4) - (k - p)/4 = ceil(p/4) bytes hold the
 * prefix and nothing else. A file of ordered sections is therefore a KMC2 database of ordered bins:
 *   k_kff_repack  all sections in one launch: the tile's records staged in LDS (whole aligned 16-byte pieces on both sides, as k_tr_dump and k_cnt_gather move theirs),
 *                 per record the prefix bytes dropped, the suffix bytes copied, the counter reversed, and — from the prefix of the record and of its predecessor in the
 *                 same section — the entries of the segmented LUT that lie between them: n_sections x 4^p global record offsets (+ one closing entry = n), the shape
 *                 kmc_hip_db_dump_device and kmc_hip_db_histogram_device take through n_lut_segments (kmc2_db_reader.h:1776-1791). One section: the KMC1 LUT.
 *                 Workgroups behind the tiles write the entries of the empty sections. No 64-bit words, no width template.
 *   k_kff_unpack  one thread per record: (SIZE k-mer words, count word), the layout k_db_unpack leaves, for the sort of several sections into one body
 *   k_kff_verify  over the sorted records: neighbours strictly ascending (a k-mer present in two sections is corrupt: the reference would emit it twice)
 *   k_kff_frame   the inverse of k_kff_repack, for KFF output (kmc_tools/kff_db_writer.h:98-118): the prefix bytes back from the LUT, the suffix bytes copied, the counter
 *                 reversed and widened to the file's data_size; the same two images in LDS
 * k_kff_repack and k_kff_unpack verify what they read: the padding bits are zero and the prefix is below 4^p (with (k - p) % 4 == 0 the padding bits are the top bits of
 * the prefix bytes: one comparison), and every record is strictly greater than its predecessor in its section, compared on the big-endian bytes. A violation lowers
 * *bad to the smallest offending record number; nothing outside the outputs is written (a prefix out of range writes no LUT entry).
 */
#ifndef KMC_AMD_KFF_DB_HIP_H
#define KMC_AMD_KFF_DB_HIP_H

#include "order_db.hip.h"

#ifndef KFF_THREADS
#define KFF_THREADS 256 /* threads of a k_kff_repack workgroup */
#endif
constexpr u32 KFF_TILE_BYTES = 32 * 1024; /* both images of a tile (records in, records out) by default: four workgroups on a CU's 160 KiB */
constexpr u32 KFF_IPT_MAX = 8;            /* consecutive records per thread: a tile is KFF_THREADS x ipt records */
constexpr u32 KFF_LDS_MAX = 60 * 1024;    /* the most an override may ask for */
constexpr u32 KFF_GAP = 64;               /* LUT entries in a run beyond which the wave writes the run together */
constexpr u32 KFF_FILL_GROUPS = 64;       /* workgroups that write the LUT entries of empty sections */
constexpr u64 KFF_NONE = ~0ull;           /* *bad while nothing is wrong */

struct KffGeo {
	u32 k, p, kbytes /* ceil(k / 4) */, sbytes /* (k - p) / 4 */, cbytes;
	u32 n_sections, ipt;
	u32 closing; /* 1: the LUT has the closing entry behind its n_sections x 4^p entries */
};
constexpr u32 kff_default_ipt(u32 rb_in, u32 rb_out)
{
	const u32 v = KFF_TILE_BYTES / (KFF_THREADS * (rb_in + rb_out));
	return v < 1 ? 1u : v > KFF_IPT_MAX ? KFF_IPT_MAX : v;
}
/* the image of the records read: one record of halo in front, up to 15 bytes of alignment slack; a multiple of 16, so that the image behind it is aligned */
constexpr size_t kff_in_lds_bytes(u32 tile, u32 rb_in) { return (((size_t)(tile + 1) * rb_in + 16) + 15) & ~(size_t)15; }
constexpr size_t kff_lds_bytes(u32 tile, u32 rb_in, u32 rb_out) { return kff_in_lds_bytes(tile, rb_in) + (size_t)tile * rb_out + 16; }

/* the section of record j: the last s with sec_start[s] <= j (sec_start[0] = 0, sec_start[n_sections] = n > j; an empty section is never the last such s) */
__device__ __forceinline__ u32 kff_section_of(const u64 *__restrict__ sec_start, u32 n_sections, u64 j)
{
	u32 lo = 0, hi = n_sections;
	while (hi - lo > 1) {
		const u32 mid = (lo + hi) >> 1;
		if (sec_start[mid] <= j)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

/* bytes [0, bytes) from src to dst, where src and dst have the same residue modulo 16: the bytes in front of the first aligned piece and behind the last one go
 * one by one, the rest as whole 16-byte pieces. Nothing outside [0, bytes) is read or written. */
__device__ __forceinline__ void kff_copy_aligned(uint8_t *dst, const uint8_t *src, u32 mis /* that residue */, u32 bytes, u32 tid)
{
	const u32 head = bytes < ((16u - mis) & 15u) ? bytes : ((16u - mis) & 15u), n_vec = (bytes - head) / 16, tail0 = head + n_vec * 16;
	for (u32 i = tid; i < head; i += KFF_THREADS)
		dst[i] = src[i];
	const TrVec16 *src16 = reinterpret_cast<const TrVec16 *>(src + head);
	TrVec16 *dst16 = reinterpret_cast<TrVec16 *>(dst + head);
	for (u32 i = tid; i < n_vec; i += KFF_THREADS)
		dst16[i] = src16[i];
	for (u32 i = tail0 + tid; i < bytes; i += KFF_THREADS)
		dst[i] = src[i];
}

/* a - b over kbytes big-endian bytes: < 0, 0, > 0 */
__device__ __forceinline__ int kff_compare(const uint8_t *a, const uint8_t *b, u32 kbytes)
{
	int c = 0;
#pragma unroll 1
	for (u32 q = 0; q < kbytes && !c; ++q)
		c = (int)a[q] - (int)b[q];
	return c;
}

/* entries [q0, q1) of seg = v. Every lane of a wave calls this together: a run of up to KFF_GAP entries is written by its own lane, a longer one — the records of a small
 * file under a wide LUT lie thousands of entries apart — by the whole wave, 64 neighbouring entries a round. */
__device__ __forceinline__ void kff_fill(u64 *seg, u32 q0, u32 q1, u64 v)
{
	const bool longer = q0 < q1 && q1 - q0 > KFF_GAP;
	if (!longer) {
#pragma unroll 1
		for (u32 q = q0; q < q1; ++q)
			seg[q] = v;
	}
	u64 todo = __ballot(longer);
	while (todo) {
		const int leader = __ffsll(todo) - 1;
		u64 *lseg = reinterpret_cast<u64 *>(__shfl((u64)(size_t)seg, leader));
		const u32 a = __shfl(q0, leader), b = __shfl(q1, leader);
		const u64 lv = __shfl(v, leader);
#pragma unroll 1
		for (u32 q = a + (threadIdx.x & 63); q < b; q += 64)
			lseg[q] = lv;
		todo &= todo - 1;
	}
}

/* Workgroups [0, n_tiles): tile t = records [t x tile, (t + 1) x tile) of kff -> out (records of sbytes + cbytes bytes) and the LUT entries the tile's records bound.
 * A thread takes ipt consecutive records: the section of its first one by bisection of sec_start, the following ones by walking on. Record j of section s with prefix
 * x, its predecessor in the section with prefix w (none: the entries from 0 on): lut[s x 4^p + q] = j for q in (w, x]; the section's last record: j + 1 for q in (x, 4^p).
 * A run of more than KFF_GAP entries is written by the record's whole wave (kff_fill). Workgroups [n_tiles, gridDim.x): the 4^p entries of every EMPTY section
 * (= its start) and the closing entry. Every entry is written exactly once. */
__global__ void __launch_bounds__(KFF_THREADS) k_kff_repack(const uint8_t *__restrict__ kff, u64 n, const u64 *__restrict__ sec_start /* [n_sections + 1] */, KffGeo g, u32 n_tiles,
                                                            uint8_t *__restrict__ out, u64 *__restrict__ lut, u64 *__restrict__ bad)
{
	KMC_DYN_LDS(uint8_t, s_img);
	const u32 tid = threadIdx.x, n_pref = 1u << (2 * g.p);
	if (blockIdx.x >= n_tiles) {
		const u32 fb = blockIdx.x - n_tiles, nf = gridDim.x - n_tiles;
		for (u32 s = fb; s < g.n_sections; s += nf) {
			const u64 a = sec_start[s];
			if (sec_start[s + 1] != a)
				continue;
			for (u32 q = tid; q < n_pref; q += KFF_THREADS)
				lut[(u64)s * n_pref + q] = a;
		}
		if (g.closing && fb == 0 && tid == 0)
			lut[(u64)g.n_sections * n_pref] = n;
		return;
	}
	const u32 tile = KFF_THREADS * g.ipt, rb_in = g.kbytes + g.cbytes, rb_out = g.sbytes + g.cbytes, pbytes = g.kbytes - g.sbytes;
	const u64 j0 = (u64)blockIdx.x * tile;
	const u32 len = (u32)(n - j0 < (u64)tile ? n - j0 : (u64)tile), halo = j0 ? 1u : 0u;
	const uint8_t *src = kff + (j0 - halo) * rb_in;
	uint8_t *dst = out + j0 * rb_out;
	/* both images at the byte offset their first byte has inside its 16 bytes of HBM */
	const u32 mis_in = (u32)((size_t)src & 15), mis_out = (u32)((size_t)dst & 15);
	uint8_t *img_in = s_img + mis_in, *img_out = s_img + kff_in_lds_bytes(tile, rb_in) + mis_out;
	kff_copy_aligned(img_in, src, mis_in, (len + halo) * rb_in, tid);
	__syncthreads();
	const u32 m0 = tid * g.ipt < len ? tid * g.ipt : len, m1 = m0 + g.ipt < len ? m0 + g.ipt : len;
	u32 s = m0 < m1 ? kff_section_of(sec_start, g.n_sections, j0 + m0) : 0u;
	u64 worst = KFF_NONE;
	for (u32 it = 0; it < g.ipt; ++it) { /* every thread makes every round: the wave fills long runs of LUT entries together */
		const u32 m = m0 + it;
		u64 *seg = lut;
		u64 j = 0;
		u32 qa = 0, qx = 0, qe = 0; /* entries [qa, qx) = j, [qx, qe) = j + 1 */
		if (m < m1) {
			j = j0 + m;
#pragma unroll 1
			while (sec_start[s + 1] <= j)
				++s;
			const uint8_t *r = img_in + (size_t)(m + halo) * rb_in, *prev = r - rb_in;
			const bool first = j == sec_start[s];
			u32 x = 0, w = 0;
#pragma unroll 1
			for (u32 q = 0; q < pbytes; ++q) {
				x = (x << 8) | r[q];
				if (!first)
					w = (w << 8) | prev[q];
			}
			bool wrong = x >= n_pref; /* a padding bit, or a prefix the LUT has no entry for */
			if (!first && kff_compare(r, prev, g.kbytes) <= 0)
				wrong = true;
			uint8_t *o = img_out + (size_t)m * rb_out;
#pragma unroll 1
			for (u32 q = 0; q < g.sbytes; ++q)
				o[q] = r[pbytes + q];
#pragma unroll 1
			for (u32 q = 0; q < g.cbytes; ++q)
				o[g.sbytes + q] = r[g.kbytes + g.cbytes - 1 - q];
			if (x < n_pref) {
				seg = lut + (u64)s * n_pref;
				qa = first ? 0u : (w < x ? w + 1 : x + 1); /* w >= x: none (w is in range where the records ascend) */
				qx = x + 1;
				qe = j + 1 == sec_start[s + 1] ? n_pref : qx;
			}
			if (wrong && j < worst)
				worst = j;
		}
		kff_fill(seg, qa, qx, j);
		kff_fill(seg, qx, qe, j + 1);
	}
	if (worst != KFF_NONE)
		atomicMin(bad, worst);
	__syncthreads();
	kff_copy_aligned(dst, img_out, mis_out, len * rb_out, tid);
}

/* ---- the inverse: a database body framed as KFF records (CKFFDbWriter<SIZE>::add_kmer, kmc_tools/kff_db_writer.h:98-118) ---- */
constexpr u32 KFF_WALK = 4; /* LUT entries a thread walks from one record's prefix towards the next one's before it bisects what is left */
struct KffFrame {
	u32 p, kbytes /* ceil(k / 4) */, sbytes /* (k - p) / 4 */, cbytes /* the body's counter bytes */, dbytes /* the file's data_size >= cbytes */;
	u32 n_entries; /* of the LUT: segments x 4^p (the closing entry of a segmented LUT is not counted) */
	u32 ipt;
};
/* the image of the records read, up to 15 bytes of alignment slack, a multiple of 16; behind it the image of the records written and its slack */
constexpr size_t kff_frame_in_lds_bytes(u32 tile, u32 rb_in) { return (((size_t)tile * rb_in + 16) + 15) & ~(size_t)15; }
constexpr size_t kff_frame_lds_bytes(u32 tile, u32 rb_in, u32 rb_out) { return kff_frame_in_lds_bytes(tile, rb_in) + (size_t)tile * rb_out + 16; }

/* the last entry of lut[lo .. hi) that is <= j, where lut[lo] <= j */
__device__ __forceinline__ u32 kff_last_entry(const u64 *__restrict__ lut, u32 lo, u32 hi, u64 j)
{
	while (hi - lo > 1) {
		const u32 mid = lo + ((hi - lo) >> 1);
		if (lut[mid] <= j)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}
/* the same by doubling steps from lo and a bisection of the last step: O(log distance) loads — one or two where the answer lies next to lo */
__device__ __forceinline__ u32 kff_last_entry_near(const u64 *__restrict__ lut, u32 lo, u32 hi, u64 j)
{
	u32 step = 1;
	while (hi - lo > step && lut[lo + step] <= j) {
		lo += step;
		step <<= 1;
	}
	return kff_last_entry(lut, lo, hi - lo > step ? lo + step : hi, j);
}

/* Workgroup t: records [first + t x tile, first + (t + 1) x tile) of the body (sbytes suffix bytes, cbytes counter bytes least significant first) -> records t x tile ..
 * of out: pbytes = kbytes - sbytes prefix bytes most significant first, the suffix bytes verbatim, dbytes - cbytes zero bytes, the counter bytes reversed. The prefix of
 * record j is the index of the last LUT entry <= j, modulo 4^p under a segmented LUT (kmc2_db_reader.h:1776-1791); with (k - p) % 4 == 0 its value below 4^p leaves the
 * padding bits of the first byte zero. The search has two levels. Every thread bisects the whole LUT for the TILE's first record and steps on from there to the tile's
 * last one: the addresses are the same in all lanes (block index and kernel arguments only), so these are scalar loads, and the upper levels of the bisection are the
 * same words for every tile. A thread then takes ipt consecutive records: it bisects the tile's slice of the LUT for the first one — a word or two where the LUT is
 * dense —; for each following one it walks at most KFF_WALK entries and bisects the rest of the slice where that was not enough. So a record costs O(log entries) loads
 * whether the LUT is dense or five records lie under 4^9 entries (the walk gives up, the bisection is over what is left). Both images lie in LDS at the byte offset they
 * have inside their 16 bytes of HBM and move as whole aligned pieces (kff_copy_aligned). Nothing outside out[0 .. count x (kbytes + dbytes)) is written. No wave-wide
 * step: a thread without records does nothing between the two barriers. */
__global__ void __launch_bounds__(KFF_THREADS) k_kff_frame(const uint8_t *__restrict__ recs, const u64 *__restrict__ lut, u64 first, u64 count, KffFrame g, uint8_t *__restrict__ out)
{
	KMC_DYN_LDS(uint8_t, s_img);
	const u32 tid = threadIdx.x, tile = KFF_THREADS * g.ipt, rb_in = g.sbytes + g.cbytes, rb_out = g.kbytes + g.dbytes, pbytes = g.kbytes - g.sbytes, pad = g.dbytes - g.cbytes;
	const u64 l0 = (u64)blockIdx.x * tile;
	const u32 len = (u32)(count - l0 < (u64)tile ? count - l0 : (u64)tile);
	/* the tile's slice of the LUT: entries [t_lo, t_end), t_lo the entry of its first record, t_end - 1 the entry of its last one (len >= 1: the grid has no empty tile) */
	const u32 t_lo = kff_last_entry(lut, 0u, g.n_entries, first + l0);
	const u32 t_end = kff_last_entry_near(lut, t_lo, g.n_entries, first + l0 + len - 1) + 1;
	const uint8_t *src = recs + (first + l0) * rb_in;
	uint8_t *dst = out + l0 * rb_out;
	const u32 mis_in = (u32)((size_t)src & 15), mis_out = (u32)((size_t)dst & 15);
	uint8_t *img_in = s_img + mis_in, *img_out = s_img + kff_frame_in_lds_bytes(tile, rb_in) + mis_out;
	kff_copy_aligned(img_in, src, mis_in, len * rb_in, tid);
	__syncthreads();
	const u32 m0 = tid * g.ipt < len ? tid * g.ipt : len, m1 = m0 + g.ipt < len ? m0 + g.ipt : len;
	if (m0 < m1) {
		const u32 pmask = (1u << (2 * g.p)) - 1;
		u32 lo = kff_last_entry(lut, t_lo, t_end, first + l0 + m0);
		for (u32 m = m0; m < m1; ++m) {
			const u64 j = first + l0 + m;
			u32 w = 0;
#pragma unroll 1
			while (w < KFF_WALK && lo + 1 < t_end && lut[lo + 1] <= j)
				++lo, ++w;
			if (w == KFF_WALK)
				lo = kff_last_entry(lut, lo, t_end, j);
			const uint8_t *r = img_in + (size_t)m * rb_in;
			uint8_t *o = img_out + (size_t)m * rb_out;
			const u32 x = lo & pmask;
#pragma unroll 1
			for (u32 q = 0; q < pbytes; ++q)
				o[q] = (uint8_t)(x >> (8 * (pbytes - 1 - q)));
#pragma unroll 1
			for (u32 q = 0; q < g.sbytes; ++q)
				o[pbytes + q] = r[q];
#pragma unroll 1
			for (u32 q = 0; q < pad; ++q)
				o[g.kbytes + q] = 0;
#pragma unroll 1
			for (u32 q = 0; q < g.cbytes; ++q)
				o[g.kbytes + pad + q] = r[g.sbytes + g.cbytes - 1 - q];
		}
	}
	__syncthreads();
	kff_copy_aligned(dst, img_out, mis_out, len * rb_out, tid);
}

/* records [kbytes k-mer bytes, most significant first, right-aligned][cbytes count bytes, most significant first] -> (SIZE k-mer words, 1 count word), as k_db_unpack
 * leaves them; the padding bits and the order inside every section verified as k_kff_repack does */
template <int SIZE>
__global__ void __launch_bounds__(256) k_kff_unpack(const uint8_t *__restrict__ kff, u64 n, const u64 *__restrict__ sec_start, u32 n_sections, u32 k, u32 kbytes, u32 cbytes,
                                                   u64 *__restrict__ out /* [n][SIZE + 1] */, u64 *__restrict__ bad)
{
	const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
	if (j >= n)
		return;
	const u32 s = kff_section_of(sec_start, n_sections, j), rb = kbytes + cbytes;
	const uint8_t *r = kff + j * (u64)rb;
	u64 x[SIZE];
#pragma unroll
	for (int w = 0; w < SIZE; ++w)
		x[w] = 0;
	for (u32 q = 0; q < kbytes; ++q) { /* byte kbytes-1-q of the k-mer */
		const u32 pb = kbytes - 1 - q;
#pragma unroll
		for (int w = 0; w < SIZE; ++w)
			if ((pb >> 3) == (u32)w)
				x[w] |= (u64)r[q] << ((pb & 7) * 8);
	}
	u64 c = 0;
	for (u32 q = 0; q < cbytes; ++q)
		c = (c << 8) | r[kbytes + q];
	bool wrong = (k & 3) && (r[0] >> (2 * (k & 3)));
	if (j != sec_start[s] && kff_compare(r, r - rb, kbytes) <= 0)
		wrong = true;
	u64 *o = out + j * (u64)(SIZE + 1);
#pragma unroll
	for (int w = 0; w < SIZE; ++w)
		o[w] = x[w];
	o[SIZE] = c;
	if (wrong)
		atomicMin(bad, j);
}

/* the sorted records of all sections: *bad = the smallest i with recs[i - 1] >= recs[i] */
template <int SIZE> __global__ void __launch_bounds__(256) k_kff_verify(const u64 *__restrict__ recs /* [n][SIZE + 1] */, u64 n, u64 *__restrict__ bad)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x + 1;
	if (i >= n)
		return;
	if (!so_less<SIZE>(recs + (i - 1) * (u64)(SIZE + 1), recs + i * (u64)(SIZE + 1)))
		atomicMin(bad, i);
}

#endif
