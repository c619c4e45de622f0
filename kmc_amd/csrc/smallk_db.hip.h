/*
 * kmc_amd/csrc/smallk_db.hip.h — the small-k table (k <= 13: 4^k 64-bit counters, kmc_hip_smallk_open / k_s1_smallk_count) as a database body on the device (gfx950,
 * wave64): what CSmallKCompleter::CompleteKMCFormat and CompleteKFFFormat do on the CPU (kmc_core/kb_completer.h:149-378), single-threaded, over a table that had to
 * come down over the host link first.
 *
 * The table index IS the k-mer, so the table order is the database order: no sort and no key comparison, only a stream compaction that frames what it keeps.
 *   k_sk_tally   per tile of SK_THREADS x ipt entries: the entries the cutoffs keep -> tile_counts[tile]; non-zero / below cutoff_min / above cutoff_max -> stats[0..2]
 *                (a workgroup walks several tiles where there are more than SK_TALLY_WGS)
 *   k_db_cumsum  (order_db.hip.h) scans tile_counts
 *   k_sk_emit    classifies again, ranks the kept entries of the tile in index order, frames each into an LDS image of the tile's output, copies the image out as whole
 *                aligned 16-byte pieces (kff_copy_aligned), and writes the KMC1 LUT: entry e with e % 4^(k - p) == 0 writes lut[e / 4^(k - p)] = kept entries in front of e
 * No workgroup waits for another one: the three launches are ordered by the stream alone.
 *
 * Who reads what. A wave takes 64 x ipt consecutive entries, a round of 128 (PAIR: lane l the entries 2l and 2l + 1 of the round, one 16-byte load) or of 64 (an odd ipt,
 * or a table that is not 16-byte aligned: one 8-byte load). A wave instruction therefore reads 1 KiB (512 B) of consecutive table; the up to eight values of a thread stay
 * in registers (every loop over them is unrolled to its compile-time bound and guarded by the round count, which is uniform: no indexed register array, no scratch). The
 * rank of an entry is (kept in the waves in front, through LDS) + (kept in the wave's earlier rounds) + (kept in lower lanes of this round: ballot and popcount): it
 * depends on the table alone.
 *
 * The image. Kept entries of neighbouring lanes have neighbouring ranks, so the 32 lanes of a half-wave write one byte each at a distance of record_bytes (1..8): at
 * most 256 bytes, two bank rows of the 32-dword write banking — two lanes on a bank at 5..8 bytes, none below. (k_kff_frame's first layout had the lanes ipt records
 * apart and put 16 of them on one bank.) 2048 records x 8 bytes + 16 is the largest image: 16 KiB, so LDS never bounds the occupancy before the 256 threads do.
 */
#ifndef KMC_AMD_SMALLK_DB_HIP_H
#define KMC_AMD_SMALLK_DB_HIP_H

#include "kff_db.hip.h"

#ifndef SK_THREADS
#define SK_THREADS 256 /* threads of a k_sk_* workgroup (kff_copy_aligned strides by KFF_THREADS) */
#endif
static_assert(SK_THREADS == KFF_THREADS, "k_sk_emit moves its image with kff_copy_aligned");
constexpr u32 SK_IPT_MAX = 8;     /* entries per thread: a tile is SK_THREADS x ipt entries */
constexpr u32 SK_IPT_DEFAULT = 8; /* 2048 entries, 16 KiB of table per tile */
constexpr u32 SK_TALLY_WGS = 2048; /* workgroups of k_sk_tally at most: eight on each of the 256 CUs, each with its three atomics at the end */
enum : u32 { SK_FRAME_KMC1 = 0, SK_FRAME_KFF = 1 };
enum : u32 { SK_ST_UNIQUE = 0, SK_ST_BELOW = 1, SK_ST_ABOVE = 2, SK_ST_KEPT = 3 };

struct SkCut {
	u64 cutoff_min, cutoff_max, counter_max;
};
struct SkFrame {
	u32 key_bytes; /* k-mer bytes of a record, most significant first: KMC1 (k - p) / 4 (0..3), KFF ceil(k / 4) */
	u32 cnt_bytes; /* counter bytes: KMC1 counter_size, least significant first; KFF data_size, most significant first */
	u32 cnt_msb_first;
	u32 span_log2; /* KMC1: 2 (k - p), an entry whose low span_log2 bits are zero owns a LUT word */
};
constexpr size_t sk_emit_lds_bytes(u32 tile, u32 rec_bytes) { return (size_t)tile * rec_bytes + 16; }

/* CompleteKMCFormat's rule for one counter, in 64-bit arithmetic (kb_completer.h:232-246): 0 absent, 1 below cutoff_min, 2 above cutoff_max, 3 kept */
__device__ __forceinline__ u32 sk_classify(u64 v, const SkCut &cut) { return !v ? 0u : v < cut.cutoff_min ? 1u : v > cut.cutoff_max ? 2u : 3u; }

/* the wave's entries into v[0..8): round r < rounds, lane l: PAIR v[2r], v[2r + 1] = entries wave0 + (64r + l) x 2 and the next one; else v[r] = entry wave0 + 64r + l.
 * An entry behind the table (a table smaller than the tile) reads as 0: absent. n is even (4^k), so a pair lies inside the table or behind it. */
template <bool PAIR> __device__ __forceinline__ void sk_load(const u64 *__restrict__ table, u64 n, u64 wave0, u32 rounds, u32 lane, u64 (&v)[SK_IPT_MAX])
{
	constexpr u32 E = PAIR ? 2 : 1, MAXR = SK_IPT_MAX / E;
#pragma unroll
	for (u32 r = 0; r < MAXR; ++r) {
		const u64 e = wave0 + (u64)(r * 64 + lane) * E;
		const bool in = r < rounds && e < n;
		if (PAIR) {
			TrVec16 t = {0, 0};
			if (in)
				t = *reinterpret_cast<const TrVec16 *>(table + e);
			v[2 * r] = t.a;
			v[2 * r + 1] = t.b;
		} else
			v[r] = in ? table[e] : 0;
	}
}

/* tile_counts[tile] = entries of the tile the cutoffs keep; stats[SK_ST_UNIQUE / _BELOW / _ABOVE] += the tallies. A workgroup takes tiles blockIdx.x, + gridDim.x, ...
 * (the host launches at most SK_TALLY_WGS workgroups) and keeps its tallies in registers over all of them: per wave by shuffles, per workgroup through LDS, at most one
 * atomic per tally that is not zero at the end. (One workgroup per tile and so three atomics per tile on the same three words took 404 us for the 32 768 tiles of k = 13,
 * four times the emit kernel's pass over the same table: profiles/r15/smallk_view_kernel_trace_first.json.) The tile's kept count goes through LDS slots that alternate
 * with the tile's parity, so one barrier a tile is enough: a wave is at most one tile ahead of the thread that reads the slots. */
template <bool PAIR>
__global__ void __launch_bounds__(SK_THREADS) k_sk_tally(const u64 *__restrict__ table, u64 n, u32 ipt, u32 n_tiles, SkCut cut, u64 *__restrict__ tile_counts, u64 *__restrict__ stats)
{
	__shared__ u32 s_kept[2][SK_THREADS / 64];
	__shared__ u32 s_red[SK_THREADS / 64][3];
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	u32 unique = 0, below = 0, above = 0, parity = 0;
	for (u32 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x, parity ^= 1) {
		const u64 wave0 = ((u64)tile * SK_THREADS + wave * 64) * ipt;
		u64 v[SK_IPT_MAX];
		sk_load<PAIR>(table, n, wave0, PAIR ? ipt / 2 : ipt, lane, v);
		u32 kept = 0;
#pragma unroll
		for (u32 i = 0; i < SK_IPT_MAX; ++i) {
			const u32 cls = sk_classify(v[i], cut);
			unique += cls != 0;
			below += cls == 1;
			above += cls == 2;
			kept += cls == 3;
		}
		kept = wave_sum<u32>(kept);
		if (lane == 0)
			s_kept[parity][wave] = kept;
		__syncthreads();
		if (tid == 0) {
			u32 sum = 0;
#pragma unroll
			for (u32 w = 0; w < SK_THREADS / 64; ++w)
				sum += s_kept[parity][w];
			tile_counts[tile] = sum;
		}
	}
	unique = wave_sum<u32>(unique); /* a thread sees at most ceil(n_tiles / gridDim.x) x 8 entries: far below 2^32 */
	below = wave_sum<u32>(below);
	above = wave_sum<u32>(above);
	if (lane == 0) {
		s_red[wave][SK_ST_UNIQUE] = unique;
		s_red[wave][SK_ST_BELOW] = below;
		s_red[wave][SK_ST_ABOVE] = above;
	}
	__syncthreads();
	if (tid < 3) {
		u32 sum = 0;
#pragma unroll
		for (u32 w = 0; w < SK_THREADS / 64; ++w)
			sum += s_red[w][tid];
		if (sum)
			atomicAdd(stats + tid, (u64)sum);
	}
}

/* the low `bytes` (0..4) bytes of x, most significant first, as the low bytes of the result in memory order */
__device__ __forceinline__ u32 sk_msb_first(u32 x, u32 bytes) { return bytes ? __builtin_bswap32(x) >> (8 * (4 - bytes)) : 0u; }

/* The kept entries of tile blockIdx.x, framed, to out + tile_base[tile] x record bytes, in index order; lut (KMC1; NULL: none) as described at the top. Nothing outside
 * out[tile_base[tile] x rb .. tile_base[tile + 1] x rb) and lut[0 .. 4^p) is written. */
template <bool PAIR>
__global__ void __launch_bounds__(SK_THREADS) k_sk_emit(const u64 *__restrict__ table, u64 n, u32 ipt, SkCut cut, SkFrame f, const u64 *__restrict__ tile_base, uint8_t *__restrict__ out,
                                                        u64 *__restrict__ lut)
{
	KMC_DYN_LDS(uint8_t, s_img);
	__shared__ u32 s_wave[SK_THREADS / 64];
	constexpr u32 E = PAIR ? 2 : 1, MAXR = SK_IPT_MAX / E;
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rounds = PAIR ? ipt / 2 : ipt, rb = f.key_bytes + f.cnt_bytes;
	const u64 wave0 = ((u64)blockIdx.x * SK_THREADS + wave * 64) * ipt;
	u64 v[SK_IPT_MAX];
	sk_load<PAIR>(table, n, wave0, rounds, lane, v);
	u32 rank[MAXR], running = 0;
#pragma unroll
	for (u32 r = 0; r < MAXR; ++r) {
		rank[r] = 0;
		if (r < rounds) { /* uniform: the whole wave votes */
			const u64 b0 = __ballot(sk_classify(v[E * r], cut) == 3), b1 = PAIR ? __ballot(sk_classify(v[E * r + E - 1], cut) == 3) : 0ull;
			rank[r] = running + __builtin_amdgcn_mbcnt_hi((u32)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((u32)b0, 0u)) +
			          __builtin_amdgcn_mbcnt_hi((u32)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((u32)b1, 0u));
			running += (u32)__popcll(b0) + (u32)__popcll(b1);
		}
	}
	if (lane == 0)
		s_wave[wave] = running;
	__syncthreads();
	u32 wave_off = 0, total = 0;
#pragma unroll
	for (u32 w = 0; w < SK_THREADS / 64; ++w) {
		const u32 c = s_wave[w];
		wave_off += w < wave ? c : 0u;
		total += c;
	}
	const u64 base = tile_base[blockIdx.x];
	uint8_t *dst = out + base * rb;
	const u32 mis = (u32)((size_t)dst & 15);
	uint8_t *img = s_img + mis; /* the image at the byte offset its first byte has inside its 16 bytes of HBM */
	const u64 span_mask = ((u64)1 << f.span_log2) - 1;
#pragma unroll
	for (u32 r = 0; r < MAXR; ++r) {
		if (r < rounds) {
			u32 at = wave_off + rank[r];
#pragma unroll
			for (u32 q = 0; q < E; ++q) {
				const u64 e = wave0 + (u64)(r * 64 + lane) * E + q, c64 = v[E * r + q];
				if (lut && e < n && !(e & span_mask))
					lut[e >> f.span_log2] = base + at;
				if (sk_classify(c64, cut) == 3) {
					const u32 c = (u32)(c64 > cut.counter_max ? cut.counter_max : c64); /* kept: at most cutoff_max, and the smaller of the two bounds fits cnt_bytes */
					const u64 rec = (u64)sk_msb_first((u32)e, f.key_bytes) | ((u64)(f.cnt_msb_first ? sk_msb_first(c, f.cnt_bytes) : c) << (8 * f.key_bytes));
					uint8_t *o = img + (size_t)at * rb;
#pragma unroll 1
					for (u32 b = 0; b < rb; ++b)
						o[b] = (uint8_t)(rec >> (8 * b));
					++at;
				}
			}
		}
	}
	__syncthreads();
	kff_copy_aligned(dst, img, mis, total * rb, tid);
}

#endif
