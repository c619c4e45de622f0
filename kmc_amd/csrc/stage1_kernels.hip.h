/*
 * kmc_amd/csrc/stage1_kernels.hip.h — the kernels of KMC's STAGE 1 on gfx950 (docs/history/DESIGN_rounds_1_to_5.md §9): text of a FASTA/FASTQ part ->
 * codes -> minimizer signatures -> super-k-mers -> bin records + the collector's sums. Reachable through kmc_hip_split_part (one part, host
 * text -> host records: the engine of the stage-1 worker plug-in), kmc_hip_split_reads_plan/_emit (codes in HBM -> bins in HBM in the layout
 * kmc_hip_process_bins_device takes) and the test hook kmc_hip_debug_split_reads. The signature -> bin map is an input (stage 0 stays the
 * reference's). GPU-validated against the reference's restatement, per part (tests/test_gpu_stage1_parts.py and the per-variant files beside it) and per
 * kernel (tests/test_gpu_stage1.py): every kernel of this file, at signature lengths 5..11, minimum windows of 1..252 m-mers and k up to 256.
 *
 * What the reference does (kmc_core/splitter.cpp:557-672, CSplitter::ProcessReads) is a sequential scan per read with a two-variable state
 * (current signature, its position). Its RESULT has a data-parallel description, which oracle/stage1_oracle.c's line-by-line restatement
 * confirms on every test (tests/test_stage1_emulated.py):
 *   - symbols are codes 0..3, anything else (N, read boundaries: the host joins reads with a separator) is "invalid";
 *   - the signature of the k-mer at q is the MINIMUM of norm[m-mer] over the k - m + 1 m-mers inside it (norm: kmc_api/mmer.h:39-95,
 *     the smaller strand among the allowed m-mers, 4^m if none) — the reference's tie and fall-out rules only decide WHICH occurrence it
 *     remembers, never the value;
 *   - a super-k-mer is a maximal run of consecutive valid k-mers with one signature value, cut into pieces of 256 k-mers counted from the
 *     run's start (one byte holds the number of extra symbols, splitter.cpp:651-658); its bin record is kb_collector.cpp:57-71.
 *
 *   k_s1_signatures : codes -> signature per k-mer position (0xFFFFFFFF where no valid k-mer starts); only the test hook stores them
 *   k_s1_cut<FUSED> : signatures (from memory, or computed by the tile itself) -> the super-k-mers in position order: first symbol,
 *                     length in symbols, signature
 *   k_s1_bin_totals / k_s1_bin_layout / k_s1_emit : super-k-mers -> bin records, scattered into per-bin byte streams (see below)
 * Both are tile-parallel; k_s1_cut carries "where did the current run start" and "how many super-k-mers so far" across workgroups with two
 * decoupled look-backs (latest non-zero, and sum) over 64-bit status words.
 */
#ifndef KMC_AMD_STAGE1_KERNELS_HIP_H
#define KMC_AMD_STAGE1_KERNELS_HIP_H

#include "kernels.hip.h"

constexpr int S1_BLOCK = 256, S1_PER = 4, S1_TILE = S1_BLOCK * S1_PER; /* positions per workgroup */
constexpr int S1_MAX_K = 256;
constexpr u32 S1_NOSIG = 0xFFFFFFFFu;
/* A line of mem_part_pmm_reads symbols or more reaches CSplitter::ProcessReads in pieces that overlap by k - 1 symbols (splitter.cpp:141-145,
 * :226-231; a long-read part likewise, GetSeqLongRead :80-84), and every piece starts its super-k-mers afresh: the k-mer that starts at a
 * multiple of stride = mem_part_pmm_reads - k + 1 (counted from the line's first symbol) never shares a super-k-mer with the k-mer before it.
 * k_s1_check_records / k_s1_mark_raw put this bit into the code of those positions (codes are 0..3 or negative: every consumer masks with 3
 * or tests the sign), k_s1_cut starts a run there. The k-mers — and so the database — do not depend on it; "Total no. of super-k-mers" does. */
constexpr int8_t S1_PIECE_MARK = 0x40;

/* norm of an m-mer (kmc_api/mmer.h:39-95: the smaller of the m-mer and its reverse complement among the ALLOWED ones, 4^m if neither is)
 * computed, not looked up: the reference's table is 1 MB at m = 9, and one gather per position from it made the L2 -> L1 path the limit of
 * the first version of these kernels (4.4 ms per 300 M positions, profiles/r02/s1_bench_v2_*). */
__host__ __device__ __forceinline__ bool s1_allowed(u32 x, u32 m) /* mmer.h:39-64 */
{
	if ((x & 0x3f) == 0x3f || (x & 0x3f) == 0x3b || (x & 0x3c) == 0x3c) /* ends with TTT or TGT, or has TT in front of its last symbol */
		return false;
	const u32 is_a = ~(x | (x >> 1)) & 0x55555555u & ((1u << (2 * m)) - 1u); /* bit 2j: symbol j (from the end) is A */
	const u32 aa = is_a & (is_a >> 2);                                      /* bit 2j: symbols j and j + 1 are both A */
	if (aa & ((1u << (2 * (m - 2))) - 1u))                                  /* AA anywhere but in the two leading symbols */
		return false;
	return (x >> (2 * (m - 3))) != 0x04u; /* does not start with ACA */
}
__host__ __device__ __forceinline__ u32 s1_revcomp(u32 x, u32 m) /* mmer.h:69-80 */
{
	u32 y = ~x;
	y = ((y & 0x33333333u) << 2) | ((y >> 2) & 0x33333333u); /* reverse the sixteen 2-bit groups of the word */
	y = ((y & 0x0F0F0F0Fu) << 4) | ((y >> 4) & 0x0F0F0F0Fu);
	y = ((y & 0x00FF00FFu) << 8) | ((y >> 8) & 0x00FF00FFu);
	y = (y << 16) | (y >> 16);
	return y >> (32 - 2 * m);
}
__host__ __device__ __forceinline__ u32 s1_norm(u32 x, u32 m)
{
	const u32 special = 1u << (2 * m), r = s1_revcomp(x, m);
	const u32 a = s1_allowed(x, m) ? x : special, b = s1_allowed(r, m) ? r : special;
	return a < b ? a : b;
}

/* Signatures of the k-mers that start at positions base .. base + cnt - 1 (base may be -1; a position outside [0, n) has none) into
 * s_sig[0 .. cnt), cnt <= S1_TILE + 2. All threads of the block call; the result is visible to all of them on return.
 * A thread owns S1_SIG_PER CONSECUTIVE positions in both steps (an odd number: its LDS accesses are bank-conflict free): the m-mer is rolled
 * from one position to the next (2 byte reads instead of m), and the minimum over the k - m + 1 m-mers of a k-mer is put together from what
 * the thread's windows share, a suffix of the first S1_SIG_PER - 1 values and a prefix of the last ones (w + 4 reads for 5 windows instead
 * of 5 w). A k-mer is valid iff all its m-mers are: the maximum over the same window tells (S1_NOSIG marks an m-mer with an invalid symbol). */
constexpr int S1_SIG_PER = 5;
static_assert(S1_BLOCK * S1_SIG_PER >= S1_TILE + 2 + S1_MAX_K - 5, "one round covers every m-mer of the span");
struct S1SigLds {
	int8_t c[(S1_TILE + 2 + S1_MAX_K + 3) / 4 * 4]; /* symbols of the span: cnt + k - 1 */
	u32 mm[S1_BLOCK * S1_SIG_PER + S1_MAX_K + 8];   /* norm of the m-mer at each position of the span (reads run past the last one, unused) */
};
struct S1MinMax {
	u32 mn, mx;
	__device__ __forceinline__ void add(u32 v)
	{
		mn = v < mn ? v : mn;
		mx = v > mx ? v : mx;
	}
	__device__ __forceinline__ void add(const S1MinMax &o)
	{
		mn = o.mn < mn ? o.mn : mn;
		mx = o.mx > mx ? o.mx : mx;
	}
};
__device__ __forceinline__ void s1_signatures_to_lds(const int8_t *__restrict__ codes, u64 n, long long base, u32 cnt, u32 k, u32 m, S1SigLds &L, u32 *s_sig)
{
	const u32 tid = threadIdx.x;
	const u32 span = cnt + k - 1; /* symbols looked at */
	for (u32 i = tid; i < span; i += S1_BLOCK) {
		const long long p = base + (long long)i;
		L.c[i] = (p >= 0 && (u64)p < n) ? codes[p] : (int8_t)-1;
	}
	__syncthreads();
	/* norm of every m-mer that starts at one of the cnt positions or in the k - m positions after them */
	const u32 n_mm = cnt + k - m, i0 = tid * S1_SIG_PER;
	if (i0 < n_mm) {
		const u32 mask = (1u << (2 * m)) - 1u;
		u32 x = 0, bad = 0;
		for (u32 j = 0; j < m; ++j) {
			const int8_t c = L.c[i0 + j];
			bad += c < 0 ? 1u : 0u;
			x = (x << 2) | (u32)(c & 3);
		}
#pragma unroll
		for (u32 jj = 0; jj < (u32)S1_SIG_PER; ++jj) {
			const u32 i = i0 + jj;
			if (i >= n_mm)
				break;
			L.mm[i] = bad ? S1_NOSIG : s1_norm(x & mask, m);
			if (i + 1 < n_mm) {
				const int8_t cin = L.c[i + m], cout = L.c[i];
				bad += (cin < 0 ? 1u : 0u) - (cout < 0 ? 1u : 0u);
				x = (x << 2) | (u32)(cin & 3);
			}
		}
	}
	__syncthreads();
	const u32 w = k - m + 1;
	if (i0 < cnt) {
		if (w >= (u32)S1_SIG_PER) {
			S1MinMax mid{S1_NOSIG, 0u};
			for (u32 j = S1_SIG_PER - 1; j < w; ++j) /* shared by the thread's windows */
				mid.add(L.mm[i0 + j]);
			u32 a[S1_SIG_PER - 1], b[S1_SIG_PER - 1];
#pragma unroll
			for (int j = 0; j < S1_SIG_PER - 1; ++j) {
				a[j] = L.mm[i0 + j];
				b[j] = L.mm[i0 + w + j]; /* past the span for the last positions: only windows that do not exist use those */
			}
#pragma unroll
			for (int i = 0; i < S1_SIG_PER; ++i) {
				S1MinMax r = mid;
#pragma unroll
				for (int j = i; j < S1_SIG_PER - 1; ++j)
					r.add(a[j]);
#pragma unroll
				for (int j = 0; j < i; ++j)
					r.add(b[j]);
				if (i0 + i < cnt)
					s_sig[i0 + i] = r.mx == S1_NOSIG ? S1_NOSIG : r.mn;
			}
		} else { /* k within 3 of the signature length */
			for (u32 i = i0; i < i0 + S1_SIG_PER && i < cnt; ++i) {
				S1MinMax r{S1_NOSIG, 0u};
				for (u32 j = 0; j < w; ++j)
					r.add(L.mm[i + j]);
				s_sig[i] = r.mx == S1_NOSIG ? S1_NOSIG : r.mn;
			}
		}
	}
	__syncthreads();
}

/* test hook path: the signature of every position to global memory */
__global__ void __launch_bounds__(S1_BLOCK) k_s1_signatures(const int8_t *__restrict__ codes, u64 n, u32 k, u32 m, u32 *__restrict__ sig)
{
	__shared__ S1SigLds L;
	__shared__ u32 s_sig[S1_TILE + 2];
	const u64 t0 = (u64)blockIdx.x * S1_TILE;
	s1_signatures_to_lds(codes, n, (long long)t0, S1_TILE, k, m, L, s_sig);
	for (u32 i = threadIdx.x; i < (u32)S1_TILE; i += S1_BLOCK)
		if (t0 + i < n)
			sig[t0 + i] = s_sig[i];
}

/* decoupled look-back like lookback64, but the combination is "the latest non-zero value" (value = position + 1 of the last run start):
 * returns the last run start + 1 before this tile (0 = none), valid in lane 0 */
__device__ __forceinline__ u64 lookback64_last(u64 *status, u32 tile, u64 own_last1, u32 lane, u32 *err)
{
	if (tile == 0) {
		if (lane == 0)
			st_agent(&status[0], ST64_PREFIX | own_last1);
		return 0;
	}
	if (lane == 0)
		st_agent(&status[tile], ST64_AGG | own_last1);
	long long tbase = (long long)tile - 1;
	u64 found = 0;
	LbWatch watch;
	while (true) {
		const long long t = tbase - (long long)lane;
		const u64 v = t >= 0 ? ld_agent(&status[t]) : ST64_PREFIX;
		const u64 flag = v & ~ST64_MASK;
		const u64 m_pref = __ballot(flag == ST64_PREFIX);
		const u64 m_zero = __ballot(flag == 0);
		const int pl = m_pref ? (__ffsll(m_pref) - 1) : 64;
		const u64 need = pl < 63 ? ((2ull << pl) - 1) : ~0ull;
		if (m_zero & need) {
			if (lb_blocked(watch, err)) {
				if (lane == 0)
					lb_gave_up(watch, err, KERR_WATCHDOG | KERR_AT_STAGE1, lane, tile, tbase, 0u);
				break;
			}
			__builtin_amdgcn_s_sleep(1);
			continue;
		}
		/* the nearest tile (lowest lane <= pl) with a non-zero value wins */
		const u64 m_has = __ballot((int)lane <= pl && (v & ST64_MASK) != 0);
		if (m_has) {
			const int src = __ffsll(m_has) - 1;
			found = __shfl(v & ST64_MASK, src);
			break;
		}
		if (pl < 64)
			break;
		tbase -= 64;
	}
	if (lane == 0)
		st_agent(&status[tile], ST64_PREFIX | (own_last1 ? own_last1 : found));
	return found;
}

/* One workgroup cuts S1_SUB consecutive tiles (S1_WG_TILE positions): one ticket and one pair of look-backs per workgroup — with one tile per
 * workgroup the kernel ran at the rate of its same-address ticket atomic (50 tiles/us: 5.9 ms per 300 M positions, profiles/r02/s1_bench_v1*).
 * status_last / status_cnt: one zeroed u64 per WORKGROUP tile each (s1_cut_tiles(n) of them). sk_* receive the super-k-mers in position order;
 * *n_sk their number (written by the last tile). sk_cap bounds the writes (KERR_CAPACITY beyond it).
 * FUSED = false: signatures come from `sig` (k_s1_signatures ran before; codes, m unused). FUSED = true: the workgroup computes the
 * signatures it needs in LDS itself (sig unused): 1 byte per symbol read instead of 4 written + 4 read. */
#ifndef S1_SUB_N
#define S1_SUB_N 4
#endif
constexpr int S1_SUB = S1_SUB_N, S1_WG_TILE = S1_TILE * S1_SUB;
static_assert(S1_PER == 4, "the pieces of a thread's positions are packed into one 32-bit word");
__host__ __device__ inline u64 s1_cut_tiles(u64 n) { return (n + S1_WG_TILE - 1) / S1_WG_TILE; }

template <bool FUSED>
__global__ void __launch_bounds__(S1_BLOCK) k_s1_cut(const u32 *__restrict__ sig, const int8_t *__restrict__ codes, u32 m, u64 n, u32 k,
                                                      u64 *status_last, u64 *status_cnt, u32 *ticket_ctr, u64 *__restrict__ sk_pos, u32 *__restrict__ sk_len,
                                                      u32 *__restrict__ sk_sig, u64 sk_cap, u64 *n_sk, const u64 *has_marks, u32 *err)
{
	__shared__ u32 s_sig[S1_WG_TILE + 2]; /* signatures of positions w0 - 1 .. w0 + S1_WG_TILE */
	__shared__ u32 s_mark;
	__shared__ u64 s_tmp64[S1_BLOCK / 64 + 1];
	__shared__ u32 s_tmp32[S1_BLOCK / 64 + 1];
	__shared__ u64 s_carry_last1, s_carry_cnt;
	__shared__ u32 s_ticket;
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	if (tid == 0)
		s_ticket = atomicAdd(ticket_ctr, 1u);
	__syncthreads();
	const u32 tile = s_ticket;
	const u32 num_tiles = (u32)s1_cut_tiles(n);
	if (tile >= num_tiles)
		return;
	const u64 w0 = (u64)tile * S1_WG_TILE;
	if constexpr (FUSED) {
		__shared__ S1SigLds L;
#pragma unroll 1
		for (int sub = 0; sub < S1_SUB; ++sub)
			s1_signatures_to_lds(codes, n, (long long)w0 - 1 + (long long)sub * S1_TILE, sub == S1_SUB - 1 ? S1_TILE + 2 : S1_TILE, k, m, L, s_sig + sub * S1_TILE);
	} else {
		for (u32 i = tid; i < (u32)S1_WG_TILE + 2; i += S1_BLOCK) {
			const long long q = (long long)w0 - 1 + (long long)i;
			s_sig[i] = (q >= 0 && (u64)q < n) ? sig[q] : S1_NOSIG;
		}
		__syncthreads();
	}
	if (FUSED && has_marks && *has_marks) {
		/* S1_PIECE_MARK somewhere in the part (uniform, rare: a line of mem_part_pmm_reads symbols or more): a marked position starts a run whatever
		 * the signatures say. Marks are >= stride positions apart and the host refuses a stride within a workgroup's window, so the window holds at
		 * most one: the signatures from it on get bit 31 — they then differ from the one before the mark and from nothing else they are compared with. */
		if (tid == 0)
			s_mark = 0xFFFFFFFFu;
		__syncthreads();
		for (u32 i = tid; i < (u32)S1_WG_TILE + 2; i += S1_BLOCK) {
			const long long q = (long long)w0 - 1 + (long long)i;
			if (q >= 0 && (u64)q < n && (codes[q] & 0xC0) == S1_PIECE_MARK)
				atomicMin(&s_mark, i);
		}
		__syncthreads();
		const u32 mk = s_mark;
		if (mk != 0xFFFFFFFFu)
			for (u32 i = tid; i < (u32)S1_WG_TILE + 2; i += S1_BLOCK)
				if (i >= mk && s_sig[i] != S1_NOSIG)
					s_sig[i] |= 0x80000000u;
		__syncthreads();
	}
	/* Pass A, per sub-tile: run starts inside this thread's S1_PER positions (valid, and the k-mer before is invalid or has another
	 * signature); the last one before the thread inside the sub-tile; the sub-tile's own last one. */
	u64 before1[S1_SUB], sub_last1[S1_SUB]; /* position + 1, 0 = none */
#pragma unroll
	for (int sub = 0; sub < S1_SUB; ++sub) {
		const u32 l0 = (u32)sub * S1_TILE + tid * S1_PER; /* index of position t0 - 1 in s_sig */
		const u64 t0 = w0 + l0;
		u64 last1 = 0;
#pragma unroll
		for (int j = 0; j < S1_PER; ++j)
			if (s_sig[l0 + j + 1] != S1_NOSIG && s_sig[l0 + j] != s_sig[l0 + j + 1])
				last1 = t0 + j + 1;
		before1[sub] = block_excl_max<S1_BLOCK / 64, u64>(last1, s_tmp64);
		u64 mx = wave_incl_max<u64>(last1, lane);
		if (lane == 63)
			s_tmp64[wave] = mx;
		__syncthreads();
		u64 w = 0;
#pragma unroll
		for (int i = 0; i < S1_BLOCK / 64; ++i)
			w = s_tmp64[i] > w ? s_tmp64[i] : w;
		sub_last1[sub] = w;
		__syncthreads();
	}
	if (wave == 0) {
		u64 w = 0;
#pragma unroll
		for (int sub = 0; sub < S1_SUB; ++sub)
			w = sub_last1[sub] ? sub_last1[sub] : w; /* positions grow with sub: the last non-zero one */
		const u64 carry = lookback64_last(status_last, tile, w, lane, err);
		if (lane == 0)
			s_carry_last1 = carry;
	}
	__syncthreads();
	/* Pass B: ends. A super-k-mer ends at q if q is valid and the next k-mer is invalid / has another signature / q is the 256th k-mer of its
	 * piece (pieces are counted from the run's start, wherever that was). */
	u64 carry_last1 = s_carry_last1; /* the last run start before the sub-tile at hand */
	u32 end_bits[S1_SUB], pieces[S1_SUB], off[S1_SUB], wg_ends = 0;
#pragma unroll
	for (int sub = 0; sub < S1_SUB; ++sub) {
		const u32 l0 = (u32)sub * S1_TILE + tid * S1_PER;
		const u64 t0 = w0 + l0;
		u64 cur1 = before1[sub] ? before1[sub] : carry_last1;
		u32 n_end = 0;
		end_bits[sub] = 0, pieces[sub] = 0;
#pragma unroll
		for (int j = 0; j < S1_PER; ++j) {
			const u64 q = t0 + j;
			const u32 prev = s_sig[l0 + j], me = s_sig[l0 + j + 1], next = s_sig[l0 + j + 2];
			if (me != S1_NOSIG) {
				if (prev != me)
					cur1 = q + 1; /* a run starts here */
				const u32 in_piece = (u32)((q - (cur1 - 1)) & 255u); /* k-mers of this piece before q */
				if (next != me || in_piece == 255u) {
					end_bits[sub] |= 1u << j;
					pieces[sub] |= in_piece << (8 * j);
					++n_end;
				}
			}
		}
		u32 sub_ends;
		off[sub] = wg_ends + block_excl_sum<S1_BLOCK / 64, u32>(n_end, s_tmp32, sub_ends);
		wg_ends += sub_ends;
		carry_last1 = sub_last1[sub] ? sub_last1[sub] : carry_last1;
	}
	if (wave == 0) {
		const u64 excl = lookback64(status_cnt, tile, (u64)wg_ends, lane, err, KERR_WATCHDOG | KERR_AT_STAGE1);
		if (lane == 0) {
			s_carry_cnt = excl;
			if (tile == num_tiles - 1)
				*n_sk = excl + wg_ends;
		}
	}
	__syncthreads();
	/* Pass C: the super-k-mers, in position order */
#pragma unroll
	for (int sub = 0; sub < S1_SUB; ++sub) {
		const u32 l0 = (u32)sub * S1_TILE + tid * S1_PER;
		const u64 t0 = w0 + l0;
		u64 idx = s_carry_cnt + off[sub];
#pragma unroll
		for (int j = 0; j < S1_PER; ++j)
			if (end_bits[sub] & (1u << j)) {
				const u32 piece = (pieces[sub] >> (8 * j)) & 255u;
				if (idx < sk_cap) {
					sk_pos[idx] = t0 + j - piece;
					sk_len[idx] = k + piece;
					sk_sig[idx] = s_sig[l0 + j + 1] & 0x7FFFFFFFu;
				} else
					atomicOr(err, KERR_CAPACITY);
				++idx;
			}
	}
}

/* ------------------------------------------------------------------------------------------------ bin scatter
 * super-k-mers -> bin records ([len - k][ceil(len/4) bytes of 2-bit symbols, first symbol in bits 7:6], kb_collector.cpp:57-71) in per-bin
 * byte streams laid out one after the other in ONE buffer, each with the list of expander-pack boundaries stage 2 wants: what
 * kmc_hip_process_bins_device takes as kmc_hip_bin_desc {d_superkmers, size, n_rec, d_pack_start, n_packs}.
 *   k_s1_bin_totals : bytes, super-k-mers and k-mers per bin (LDS counters per workgroup, one global atomic per bin a workgroup touched)
 *   k_s1_bin_layout : one workgroup: bin_base[b] (256-byte aligned; stage 2 stages the image with aligned 16-byte loads), the bin's slice of
 *                     the pack-start array (ceil(bytes / S1_PACK_BYTES) packs + the closing entry), cursors at the bases
 *   k_s1_emit       : a workgroup reserves, per bin it touches, ONE contiguous segment for its tile's records (global cursor atomic) and
 *                     writes the records of the tile into their segments in arbitrary order. A segment starts on a record boundary, so the
 *                     segment that covers the j-th multiple of S1_PACK_BYTES of its bin supplies pack boundary j (queues.h:376-396: a pack
 *                     is any run of whole records): one boundary per multiple, none missing, packs of at most 2 S1_PACK_BYTES.
 * The order of super-k-mers inside a bin is therefore not the read order. The reference's is not either with more than one splitter thread
 * (each thread flushes its own buffers, kb_collector.cpp:88-106), and stage 2 sees only the multiset of k-mers. */
#ifndef S1_SK_TILE_N
#define S1_SK_TILE_N 1024
#endif
#ifndef S1_PACK_BYTES_N
#define S1_PACK_BYTES_N (1u << 18)
#endif
constexpr int S1_SK_TILE = S1_SK_TILE_N;      /* super-k-mers per workgroup of k_s1_bin_totals / k_s1_emit */
constexpr int S1_MAX_BINS = 2048;             /* KMC allows -n up to 2000 bins */
constexpr u32 S1_PACK_BYTES = S1_PACK_BYTES_N; /* > the bytes one tile can put into one bin (1024 records of <= 1 + (256 + 255 + 3) / 4 bytes): a
                                                * segment covers at most one multiple */
constexpr u32 S1_BIN_ALIGN = 256;
static_assert((u32)S1_SK_TILE * (1u + ((u32)S1_MAX_K + 255u + 3u) / 4u) < S1_PACK_BYTES, "a tile's segment must cover at most one pack boundary");

__global__ void __launch_bounds__(256) k_s1_bin_totals(const u32 *__restrict__ sk_len, const u32 *__restrict__ sk_sig, u64 n_sk, u32 k, const int *__restrict__ sig_to_bin,
                                                        u32 n_bins, u64 *__restrict__ bin_bytes, u64 *__restrict__ bin_sk, u64 *__restrict__ bin_kmers, u32 *err)
{
	__shared__ u32 s_bytes[S1_MAX_BINS], s_cnt[S1_MAX_BINS], s_km[S1_MAX_BINS];
	for (u32 b = threadIdx.x; b < n_bins; b += 256)
		s_bytes[b] = s_cnt[b] = s_km[b] = 0;
	__syncthreads();
	const u64 i0 = (u64)blockIdx.x * S1_SK_TILE;
	for (u32 j = threadIdx.x; j < (u32)S1_SK_TILE; j += 256) {
		const u64 i = i0 + j;
		if (i < n_sk) {
			const int b = sig_to_bin[sk_sig[i]];
			if (b < 0 || (u32)b >= n_bins)
				atomicOr(err, KERR_CORRUPT); /* a signature the map does not know */
			else {
				atomicAdd(&s_bytes[b], 1u + (sk_len[i] + 3u) / 4u);
				atomicAdd(&s_cnt[b], 1u);
				atomicAdd(&s_km[b], sk_len[i] - k + 1u);
			}
		}
	}
	__syncthreads();
	for (u32 b = threadIdx.x; b < n_bins; b += 256)
		if (s_cnt[b]) {
			atomicAdd(&bin_bytes[b], (u64)s_bytes[b]);
			atomicAdd(&bin_sk[b], (u64)s_cnt[b]);
			atomicAdd(&bin_kmers[b], (u64)s_km[b]);
		}
}

/* one workgroup of 256. bin_base[b]: first byte of bin b in the buffer, bin_base[n_bins]: bytes the buffer needs (incl. 256 B of readable slack
 * behind the last bin); pack_base[b]: first entry of bin b in the pack-start array (bin b owns packs + 1 entries, the last one = its size),
 * pack_base[n_bins]: entries in all. pack_start may be NULL (sizing call). */
__global__ void __launch_bounds__(256) k_s1_bin_layout(const u64 *__restrict__ bin_bytes, u32 n_bins, u64 *__restrict__ bin_base, u64 *__restrict__ pack_base,
                                                        u64 *__restrict__ cursor, u64 *__restrict__ pack_start)
{
	__shared__ u64 s_tmp[5];
	const u32 per = (n_bins + 255) / 256, lo = threadIdx.x * per;
	u64 sum = 0, packs = 0;
	for (u32 j = 0; j < per; ++j)
		if (lo + j < n_bins) {
			const u64 by = bin_bytes[lo + j];
			sum += (by + S1_BIN_ALIGN - 1) / S1_BIN_ALIGN * S1_BIN_ALIGN;
			packs += (by + S1_PACK_BYTES - 1) / S1_PACK_BYTES + 1;
		}
	u64 total, total_packs;
	u64 run = block_excl_sum<4, u64>(sum, s_tmp, total);
	u64 prun = block_excl_sum<4, u64>(packs, s_tmp, total_packs);
	for (u32 j = 0; j < per; ++j)
		if (lo + j < n_bins) {
			const u64 by = bin_bytes[lo + j], np = (by + S1_PACK_BYTES - 1) / S1_PACK_BYTES;
			bin_base[lo + j] = run;
			cursor[lo + j] = run;
			pack_base[lo + j] = prun;
			if (pack_start)
				pack_start[prun + np] = by;
			run += (by + S1_BIN_ALIGN - 1) / S1_BIN_ALIGN * S1_BIN_ALIGN;
			prun += np + 1;
		}
	if (threadIdx.x == 0) {
		bin_base[n_bins] = total + S1_BIN_ALIGN;
		pack_base[n_bins] = total_packs;
	}
}

__global__ void __launch_bounds__(256) k_s1_emit(const int8_t *__restrict__ codes, const u64 *__restrict__ sk_pos, const u32 *__restrict__ sk_len,
                                                  const u32 *__restrict__ sk_sig, u64 n_sk, u32 k, const int *__restrict__ sig_to_bin, u32 n_bins,
                                                  const u64 *__restrict__ bin_base, const u64 *__restrict__ pack_base, u64 *cursor, uint8_t *__restrict__ out,
                                                  u64 *__restrict__ pack_start)
{
	__shared__ u32 s_bytes[S1_MAX_BINS]; /* bytes of this tile per bin, then the running offset inside the tile's segment */
	__shared__ u64 s_base[S1_MAX_BINS];  /* where the tile's segment of each bin starts in `out` */
	for (u32 b = threadIdx.x; b < n_bins; b += 256)
		s_bytes[b] = 0;
	__syncthreads();
	const u64 i0 = (u64)blockIdx.x * S1_SK_TILE;
	for (u32 j = threadIdx.x; j < (u32)S1_SK_TILE; j += 256) {
		const u64 i = i0 + j;
		if (i < n_sk) {
			const int b = sig_to_bin[sk_sig[i]];
			if (b >= 0 && (u32)b < n_bins)
				atomicAdd(&s_bytes[b], 1u + (sk_len[i] + 3u) / 4u);
		}
	}
	__syncthreads();
	for (u32 b = threadIdx.x; b < n_bins; b += 256) {
		const u32 bytes = s_bytes[b];
		if (bytes) {
			const u64 at = atomicAdd(&cursor[b], (u64)bytes);
			s_base[b] = at;
			const u64 rel = at - bin_base[b], j = (rel + S1_PACK_BYTES - 1) / S1_PACK_BYTES;
			if (j * S1_PACK_BYTES < rel + bytes) /* this segment covers the j-th multiple of the pack size: its start is pack boundary j */
				pack_start[pack_base[b] + j] = rel;
		}
		s_bytes[b] = 0;
	}
	__syncthreads();
	for (u32 j = threadIdx.x; j < (u32)S1_SK_TILE; j += 256) {
		const u64 i = i0 + j;
		if (i >= n_sk)
			continue;
		const int b = sig_to_bin[sk_sig[i]];
		if (b < 0 || (u32)b >= n_bins)
			continue;
		const u32 len = sk_len[i], bytes = 1u + (len + 3u) / 4u;
		uint8_t *dst = out + s_base[b] + atomicAdd(&s_bytes[b], bytes);
		const int8_t *src = codes + sk_pos[i];
		dst[0] = (uint8_t)(len - k);
		/* four symbols per byte, first one in bits 7:6. Eight symbols per (unaligned) 8-byte load while they last: one load per symbol made
		 * this kernel wait for its 36 scattered byte loads per record */
		u32 q = 0;
		for (; 8u * (q / 2u) + 8u <= len; q += 2) {
			u64 w8;
			__builtin_memcpy(&w8, src + 4u * q, 8);
			const u32 lo = (u32)w8, hi = (u32)(w8 >> 32);
			dst[1 + q] = (uint8_t)(((lo & 3u) << 6) | (((lo >> 8) & 3u) << 4) | (((lo >> 16) & 3u) << 2) | ((lo >> 24) & 3u));
			dst[2 + q] = (uint8_t)(((hi & 3u) << 6) | (((hi >> 8) & 3u) << 4) | (((hi >> 16) & 3u) << 2) | ((hi >> 24) & 3u));
		}
		for (; q < (len + 3u) / 4u; ++q) { /* the last 1 - 7 symbols; missing ones are zero */
			u32 v = 0;
#pragma unroll
			for (u32 t = 0; t < 4; ++t) {
				const u32 p = 4 * q + t;
				v = (v << 2) | (p < len ? (u32)(src[p] & 3) : 0u);
			}
			dst[1 + q] = (uint8_t)v;
		}
	}
}

/* ------------------------------------------------------------------------------------------------ text -> codes, k+x-mer sums
 * The front of the part chain (stage1_chain.h, s1_front_part) and the third per-bin sum: launched by kmc_hip_split_part for every plain FASTA / FASTQ part.
 * Tested under emulation (tests/test_stage1_emulated.py, tests/test_stage1_parts_emulated.py) and on the device (tests/test_gpu_stage1_parts.py).
 *
 * k_s1_text_to_codes: one part of FASTA (lines_per_record 2) or FASTQ (4) text as the reference's readers cut it — it starts at a record's
 * title (fastq_reader.cpp) — to the code stream the kernels above take: the symbols of every sequence line (splitter.cpp:41-47: ACGT acgt ->
 * 0..3, anything else negative) followed by ONE negative byte where the line ends. A line ends at '\n'; a '\r' right in front of it is
 * dropped. Line number = number of '\n' before the byte (sum look-back over tiles), sequence lines are those with number = 1 mod
 * lines_per_record, the output position of a byte = number of bytes kept before it (second look-back). nl_pos[i] = position of the i-th '\n'.
 * This is CSplitter::GetSeq (splitter.cpp:92-303) for the inputs it is meant for; what GetSeq does with anything else (blank lines, a lone
 * '\r', a quality line of another length than its sequence: it skips quality by LENGTH, :281) is not reproduced — k_s1_check_records
 * recognises every such part, and the engine must hand those to the reference splitter. */
constexpr int S1_TXT_PER = 16, S1_TXT_TILE = S1_BLOCK * S1_TXT_PER;
constexpr u32 S1_TEXT_BAD = 0x1000u; /* error bit: the part is outside what k_s1_text_to_codes reproduces (its own bit: 0x10 is KERR_PEER) */

__device__ __forceinline__ int8_t s1_symbol_code(uint8_t c)
{
	const uint8_t l = c | 0x20u;
	return l == 'a' ? 0 : l == 'c' ? 1 : l == 'g' ? 2 : l == 't' ? 3 : -1;
}

__global__ void __launch_bounds__(S1_BLOCK) k_s1_text_to_codes(const uint8_t *__restrict__ text, u64 n, u32 lines_per_record, u64 *status_lines, u64 *status_out,
                                                                u32 *ticket_ctr, int8_t *__restrict__ codes, u64 *__restrict__ nl_pos, u64 nl_cap, u64 *__restrict__ seq_start,
                                                                u64 *totals, u32 *err)
{
	__shared__ u32 s_tmp[S1_BLOCK / 64 + 1];
	__shared__ u64 s_carry;
	__shared__ u32 s_ticket;
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	if (tid == 0)
		s_ticket = atomicAdd(ticket_ctr, 1u);
	__syncthreads();
	const u32 tile = s_ticket;
	const u32 num_tiles = (u32)((n + S1_TXT_TILE - 1) / S1_TXT_TILE);
	if (tile >= num_tiles)
		return;
	const u64 p0 = (u64)tile * S1_TXT_TILE + (u64)tid * S1_TXT_PER;
	uint8_t c[S1_TXT_PER + 1]; /* the thread's bytes and the one after them ('\r' looks ahead) */
	static_assert(S1_TXT_PER == 16, "one 16-byte load per thread");
	if (p0 + S1_TXT_PER <= n) {
		u32 w[4];
		__builtin_memcpy(w, text + p0, 16); /* one 16-byte load instead of sixteen byte loads */
#pragma unroll
		for (int j = 0; j < S1_TXT_PER; ++j)
			c[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
	} else {
#pragma unroll
		for (int j = 0; j < S1_TXT_PER; ++j)
			c[j] = p0 + j < n ? text[p0 + j] : (uint8_t)0;
	}
	c[S1_TXT_PER] = p0 + S1_TXT_PER < n ? text[p0 + S1_TXT_PER] : (uint8_t)0;
	if (lines_per_record == 0) {
		/* a LONG-READ part behind its title (queues.h:40; CSplitter::GetSeqLongRead, splitter.cpp:70-86): no lines, no records — every byte is a
		 * symbol, the ends of line among them (their code is negative like any other byte that is not ACGT) */
		if (tile == num_tiles - 1 && tid == 0)
			totals[1] = n;
#pragma unroll
		for (int j = 0; j < S1_TXT_PER; ++j)
			if (p0 + j < n)
				codes[p0 + j] = s1_symbol_code(c[j]);
		return;
	}
	u32 my_nl = 0;
#pragma unroll
	for (int j = 0; j < S1_TXT_PER; ++j)
		my_nl += (p0 + j < n && c[j] == '\n') ? 1u : 0u;
	u32 tile_nl;
	const u32 nl_before = block_excl_sum<S1_BLOCK / 64, u32>(my_nl, s_tmp, tile_nl);
	if (wave == 0) {
		const u64 excl = lookback64(status_lines, tile, (u64)tile_nl, lane, err, KERR_WATCHDOG | KERR_AT_STAGE1);
		if (lane == 0) {
			s_carry = excl;
			if (tile == num_tiles - 1)
				totals[0] = excl + tile_nl; /* '\n' in the part */
		}
	}
	__syncthreads();
	const u64 line0 = s_carry + nl_before;
	u64 line = line0;
	__syncthreads();
	/* which bytes are kept: every byte of a sequence line except a '\r' (which must be followed by '\n'), the '\n' included (it becomes the separator) */
	u32 keep = 0, n_keep = 0;
#pragma unroll
	for (int j = 0; j < S1_TXT_PER; ++j) {
		if (p0 + j >= n)
			break;
		const bool is_nl = c[j] == '\n';
		if (c[j] == '\r' && !(p0 + j + 1 < n && c[j + 1] == '\n'))
			atomicOr(err, S1_TEXT_BAD);
		if (c[j] < 32 && !is_nl && c[j] != '\r')
			atomicOr(err, S1_TEXT_BAD); /* GetSeq swallows a control character behind a title's end of line (splitter.cpp:119-123) */
		if ((line & (u64)(lines_per_record - 1)) == 1 && c[j] != '\r') { /* lines_per_record is 2 or 4 */
			keep |= 1u << j;
			++n_keep;
		}
		if (is_nl) {
			if (line < nl_cap)
				nl_pos[line] = p0 + j;
			else
				atomicOr(err, KERR_CAPACITY);
			++line;
		}
	}
	u32 tile_keep;
	const u32 keep_before = block_excl_sum<S1_BLOCK / 64, u32>(n_keep, s_tmp, tile_keep);
	if (wave == 0) {
		const u64 excl = lookback64(status_out, tile, (u64)tile_keep, lane, err, KERR_WATCHDOG | KERR_AT_STAGE1);
		if (lane == 0) {
			s_carry = excl;
			if (tile == num_tiles - 1)
				totals[1] = excl + tile_keep; /* bytes of the code stream */
		}
	}
	__syncthreads();
	u64 at = s_carry + keep_before;
	line = line0;
#pragma unroll
	for (int j = 0; j < S1_TXT_PER; ++j) {
		if (keep & (1u << j))
			codes[at++] = c[j] == '\n' ? (int8_t)-1 : s1_symbol_code(c[j]);
		if (p0 + j < n && c[j] == '\n') {
			/* the end of a title line: the record's sequence starts at the next code (k_s1_check_records marks the pieces of an over-long line from there) */
			if ((line & (u64)(lines_per_record - 1)) == 0 && line < nl_cap)
				seq_start[line / lines_per_record] = at;
			++line;
		}
	}
}

/* The piece starts of a long-read part (see S1_PIECE_MARK): every stride-th position of the raw code stream. One workgroup. */
__global__ void __launch_bounds__(256) k_s1_mark_raw(int8_t *__restrict__ codes, u64 n, u64 stride, u64 *has_marks)
{
	for (u64 p = ((u64)threadIdx.x + 1) * stride; p < n; p += 256 * stride) {
		if (codes[p] >= 0)
			codes[p] |= S1_PIECE_MARK;
		*has_marks = 1;
	}
}

/* One thread per record (n_lines / lines_per_record of them; a FASTA part may end inside its last sequence line): the title starts with the
 * marker, the third line of a FASTQ record with '+', sequence and quality have one length, the sequence is shorter than line_cap
 * (mem_part_pmm_reads: GetSeq cuts longer lines into overlapping pieces). Raises S1_TEXT_BAD. */
__global__ void __launch_bounds__(256) k_s1_check_records(const uint8_t *__restrict__ text, u64 n, const u64 *__restrict__ nl_pos, u64 n_lines, u32 lines_per_record,
                                                            u64 line_cap, u64 stride, const u64 *__restrict__ seq_start, int8_t *__restrict__ codes, u64 *has_marks, u32 *err)
{
	const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
	const u64 first = r * lines_per_record; /* number of the record's title line */
	if (first > n_lines || (first == n_lines && (n_lines == 0 ? n == 0 : nl_pos[n_lines - 1] + 1 >= n)))
		return; /* no such record: the text ends with the previous one */
	const u64 start = first ? nl_pos[first - 1] + 1 : 0;
	const uint8_t marker = lines_per_record == 4 ? '@' : '>';
	bool bad = text[start] != marker;
	auto line_len = [&](u64 ln) -> u64 { /* without its '\r' */
		const u64 b = ln ? nl_pos[ln - 1] + 1 : 0, e = nl_pos[ln];
		return e - b - ((e > b && text[e - 1] == '\r') ? 1 : 0);
	};
	u64 seq_len = 0;
	if (lines_per_record == 4) {
		if (first + 4 > n_lines)
			bad = true; /* a FASTQ record must be whole, every line terminated (GetSeq drops it otherwise, splitter.cpp:222-223, :283-284) */
		else {
			bad = bad || text[nl_pos[first + 1] + 1] != '+';
			seq_len = line_len(first + 1);
			bad = bad || seq_len != line_len(first + 3);
		}
	} else if (first + 1 > n_lines)
		bad = true; /* a FASTA title without its end of line */
	else {
		const u64 b = nl_pos[first] + 1, e = first + 1 < n_lines ? nl_pos[first + 1] : n;
		seq_len = e - b - ((e > b && text[e - 1] == '\r') ? 1 : 0);
	}
	if (bad) {
		atomicOr(err, S1_TEXT_BAD);
		return;
	}
	if (seq_len >= line_cap) { /* GetSeq hands such a line out in overlapping pieces (splitter.cpp:141-145, :226-231): S1_PIECE_MARK */
		const u64 s0 = seq_start[r];
		for (u64 p = stride; p < seq_len; p += stride)
			if (codes[s0 + p] >= 0)
				codes[s0 + p] |= S1_PIECE_MARK;
		*has_marks = 1;
	}
}

/* ------------------------------------------------------------------------------------------------ multi-line FASTA (-fm)
 * What reaches the splitter from CFastqReader::GetPartFromMultilneFasta (fastq_reader.cpp:399-468, ReadType::na :579-583) is simpler than single-line
 * FASTA: a title keeps its whole run of end-of-line bytes (SkipNextEOL :917-929), every other '\n' / '\r' is gone, and a part starts at a title or,
 * when the previous part held one sequence only, inside a sequence (its last k - 1 symbols carried over). CSplitter::GetSeq, branch MULTILINE_FASTA
 * (splitter.cpp:304-323), walks it with three states, written here for any text:
 *   SEQ       '>' starts a title (one read counted) -> TITLE; any other byte is a symbol (an end of line too: a negative code)
 *   TITLE     up to and including the first '\n' / '\r' every byte is the title's: that end of line -> TITLE_EOL
 *   TITLE_EOL an end of line is dropped (-> SEQ); '>' starts a title; any other byte is a symbol (-> SEQ)
 * The state in front of a byte is data-parallel: it is TITLE exactly when the last '>' or end of line before the byte is a '>' (a title runs from its
 * '>' to its first end of line, and a '>' inside it changes nothing). TITLE_EOL and SEQ differ only on an end of line, and both go to the same state
 * after any byte, so the state in front of byte p0 follows from "TITLE or not" in front of byte p0 - 1 and byte p0 - 1 itself. That is why a thread's
 * share of the latest-event scan is bytes p0 - 1 .. p0 + 14, one byte behind the bytes it classifies: the exclusive scan then answers for p0 - 1. */
enum : u32 { S1_ML_SEQ = 0, S1_ML_TITLE = 1, S1_ML_TITLE_EOL = 2 };

/* k_s1_ml_text_to_codes: one multi-line FASTA part -> the code stream of the kernels above. A title (its '>', the text, its first end of line and one more
 * end of line right behind it) becomes ONE negative separator: the '>' is kept and s1_symbol_code gives it -1. seq_start[i] = where sequence i starts in the
 * code stream (sequence 0 starts at 0 when the part starts inside a sequence, the others behind their separator), seq_cap entries (a title takes two bytes
 * at least: size / 2 + 2 suffice). totals[0] = titles (CSplitter::n_reads), totals[1] = bytes of the code stream. A part that ends inside a title line
 * (GetSeq would read past the part) raises S1_TEXT_BAD. Three decoupled look-backs per tile: the latest event (lookback64_last over (position + 1) << 1 |
 * is '>'), then kept bytes and titles (two sums, one wave each). status: 3 zeroed u64 per tile. */
__global__ void __launch_bounds__(S1_BLOCK) k_s1_ml_text_to_codes(const uint8_t *__restrict__ text, u64 n, u64 *status_ev, u64 *status_keep, u64 *status_titles,
                                                                   u32 *ticket_ctr, int8_t *__restrict__ codes, u64 *__restrict__ seq_start, u64 seq_cap, u64 *totals,
                                                                   u32 *err)
{
	__shared__ u64 s_tmp64[S1_BLOCK / 64 + 1];
	__shared__ u32 s_tmp[S1_BLOCK / 64 + 1];
	__shared__ u64 s_carry_ev, s_carry_keep, s_carry_titles;
	__shared__ u32 s_ticket;
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	if (tid == 0)
		s_ticket = atomicAdd(ticket_ctr, 1u);
	__syncthreads();
	const u32 tile = s_ticket;
	const u32 num_tiles = (u32)((n + S1_TXT_TILE - 1) / S1_TXT_TILE);
	if (tile >= num_tiles)
		return;
	const u64 p0 = (u64)tile * S1_TXT_TILE + (u64)tid * S1_TXT_PER;
	uint8_t c[S1_TXT_PER];
	static_assert(S1_TXT_PER == 16, "one 16-byte load per thread");
	if (p0 + S1_TXT_PER <= n) {
		u32 w[4];
		__builtin_memcpy(w, text + p0, 16);
#pragma unroll
		for (int j = 0; j < S1_TXT_PER; ++j)
			c[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
	} else {
#pragma unroll
		for (int j = 0; j < S1_TXT_PER; ++j)
			c[j] = p0 + j < n ? text[p0 + j] : (uint8_t)0;
	}
	const uint8_t cb = p0 < n && p0 > 0 ? text[p0 - 1] : (uint8_t)0; /* the byte in front: the last one of the thread before */
	auto is_eol = [](uint8_t x) { return x == '\n' || x == '\r'; };
	/* ---- the latest '>' or end of line among bytes p0 - 1 .. p0 + 14 */
	u64 ev = 0;
	if (p0 > 0 && p0 < n && (cb == '>' || is_eol(cb)))
		ev = (p0 << 1) | (cb == '>' ? 1u : 0u); /* (position + 1) << 1 of byte p0 - 1 */
#pragma unroll
	for (int j = 0; j < S1_TXT_PER - 1; ++j)
		if (p0 + j < n && (c[j] == '>' || is_eol(c[j])))
			ev = ((p0 + j + 1) << 1) | (c[j] == '>' ? 1u : 0u);
	const u64 ev_before = block_excl_max<S1_BLOCK / 64, u64>(ev, s_tmp64);
	const u64 ev_incl = wave_incl_max<u64>(ev, lane);
	if (lane == 63)
		s_tmp64[wave] = ev_incl;
	__syncthreads();
	if (wave == 0) {
		u64 tile_ev = 0;
#pragma unroll
		for (int i = 0; i < S1_BLOCK / 64; ++i)
			tile_ev = s_tmp64[i] > tile_ev ? s_tmp64[i] : tile_ev;
		const u64 carry = lookback64_last(status_ev, tile, tile_ev, lane, err);
		if (lane == 0)
			s_carry_ev = carry;
	}
	__syncthreads();
	const u64 last_ev = ev_before ? ev_before : s_carry_ev; /* in front of byte p0 - 1 (tiles before this one hold only earlier positions) */
	u32 st = (last_ev & 1u) ? S1_ML_TITLE : S1_ML_SEQ;
	if (p0 > 0 && p0 < n) /* byte p0 - 1 moves the state: TITLE_EOL and SEQ go the same way on every byte */
		st = cb == '>' ? S1_ML_TITLE : (st == S1_ML_TITLE ? (is_eol(cb) ? S1_ML_TITLE_EOL : S1_ML_TITLE) : S1_ML_SEQ);
	/* ---- the bytes of this thread: kept (code stream) and title starts */
	u32 keep = 0, title = 0, n_keep = 0, n_title = 0;
#pragma unroll
	for (int j = 0; j < S1_TXT_PER; ++j) {
		if (p0 + j >= n)
			break;
		const uint8_t x = c[j];
		if (st == S1_ML_TITLE) {
			if (is_eol(x))
				st = S1_ML_TITLE_EOL;
		} else if (x == '>') {
			keep |= 1u << j;
			title |= 1u << j;
			++n_keep, ++n_title;
			st = S1_ML_TITLE;
		} else if (st == S1_ML_TITLE_EOL && is_eol(x))
			st = S1_ML_SEQ;
		else {
			keep |= 1u << j;
			++n_keep;
			st = S1_ML_SEQ;
		}
		if (p0 + j == n - 1 && st == S1_ML_TITLE)
			atomicOr(err, S1_TEXT_BAD); /* the part ends inside a title line */
	}
	u32 tile_packed; /* at most S1_TXT_TILE of each per tile: 16 bits apiece */
	const u32 before_packed = block_excl_sum<S1_BLOCK / 64, u32>(n_keep | (n_title << 16), s_tmp, tile_packed);
	if (wave < 2) {
		const u64 agg = wave == 0 ? (u64)(tile_packed & 0xFFFFu) : (u64)(tile_packed >> 16);
		const u64 excl = lookback64(wave == 0 ? status_keep : status_titles, tile, agg, lane, err, KERR_WATCHDOG | KERR_AT_STAGE1);
		if (lane == 0) {
			(wave == 0 ? s_carry_keep : s_carry_titles) = excl;
			if (tile == num_tiles - 1)
				totals[wave == 0 ? 1 : 0] = excl + agg;
		}
	}
	__syncthreads();
	u64 at = s_carry_keep + (before_packed & 0xFFFFu);
	/* sequence numbers: titles before this one, + 1 when the part starts inside a sequence (which is sequence 0) */
	u64 seq = s_carry_titles + (before_packed >> 16) + (text[0] != '>' ? 1u : 0u);
	if (p0 == 0 && text[0] != '>')
		seq_start[0] = 0;
#pragma unroll
	for (int j = 0; j < S1_TXT_PER; ++j) {
		if (!(keep & (1u << j)))
			continue;
		codes[at] = s1_symbol_code(c[j]);
		++at;
		if (title & (1u << j)) {
			if (seq < seq_cap)
				seq_start[seq] = at; /* behind the separator */
			else
				atomicOr(err, KERR_CAPACITY);
			++seq;
		}
	}
}

/* The piece starts (S1_PIECE_MARK) of the sequences of a multi-line part: one thread per sequence (n_titles + 1 threads at least; sequence i runs from
 * seq_start[i] to the separator in front of seq_start[i + 1], the last one to the end of the n codes). GetSeq takes at most line_cap symbols per call and
 * steps back k - 1 when the cap stopped it, so its pieces start at start + j * stride (stride = line_cap - k + 1), as on a long single line. It does not
 * step back when a '>' or the end of the part is next: then the sequence has exactly (j + 1) * stride + k - 1 symbols, the last k-mer starts at
 * (j + 1) * stride - 1, and a mark at (j + 1) * stride or beyond lies where no k-mer of this sequence starts — so marking every multiple of the stride
 * inside a sequence of line_cap symbols or more gives the reference's piece starts at every position where a k-mer can start. */
__global__ void __launch_bounds__(256) k_s1_ml_marks(const uint8_t *__restrict__ text, u64 n, const u64 *__restrict__ seq_start, u64 n_titles, u64 line_cap, u64 stride,
                                                       int8_t *__restrict__ codes, u64 *has_marks)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	const u64 n_seq = n_titles + (text[0] != '>' ? 1u : 0u);
	if (i >= n_seq)
		return;
	const u64 s0 = seq_start[i], e = i + 1 < n_seq ? seq_start[i + 1] - 1 : n;
	const u64 len = e - s0;
	if (len >= line_cap) {
		for (u64 p = stride; p < len; p += stride)
			if (codes[s0 + p] >= 0)
				codes[s0 + p] |= S1_PIECE_MARK;
		*has_marks = 1;
	}
}

/* ------------------------------------------------------------------------------------------------ homopolymer compression (-hc)
 * CSplitter::ProcessReads calls HomopolymerCompressSeq (splitter.cpp:424-435, :575-581) on every buffer GetSeq returns, before the super-k-mer loop: the
 * first symbol stays, and every symbol whose CODE differs from the one before it ("aAaA" is one symbol, every invalid symbol is the same -1). A return of
 * GetSeq is a whole line, or ONE PIECE of a line of line_cap symbols or more / of a long-read part / of a multi-line sequence: pieces are compressed one
 * by one, so the k - 1 raw symbols two neighbours share are compressed twice, and a piece keeps its first symbol whatever stood in front of it. This is not
 * "compress the line, then cut": a run across a piece start, or inside the overlap, changes which k-mers exist.
 *
 * k_s1_hc_compact: the code stream (codes 0..3 or negative, sequences joined by a negative separator, piece starts carrying S1_PIECE_MARK) -> the stream
 * of the compressed returns, in which PIECES ARE SEQUENCES: no code carries the mark (k_s1_cut runs without has_marks), and a marked position M becomes
 *     ... main codes before M | codes of [M, M + k - 1) once more, as the tail of the piece that ends there (compared with the code in front, M - 1
 *     included) | one separator (-1) | main codes from M on, the one at M kept unconditionally.
 * The tail is taken as it stands up to M + k - 1 or the end of the stream; where the line ends earlier the surplus is fewer than k symbols in front of a
 * separator and makes no k-mer. A mark that fell on an invalid code was never set (the markers skip negative codes): harmless, because an invalid symbol at a
 * piece start leaves fewer than k symbols of the duplicated tail behind it, and the symbol after it starts a run anyway. Runs of invalid codes ARE
 * compressed (N runs and the separator next to them become one -1): the k-mers, super-k-mers and sums do not depend on it, and it keeps one rule for all codes.
 * Marks are more than S1_TXT_TILE positions apart (stride > S1_WG_TILE, stage1_chain.h), so a tile holds at most one, and the tile that holds the mark
 * emits the whole tail (up to k - 1 <= 255 codes, read again from memory: they may lie in the next tile). One decoupled look-back over kept codes + tail +
 * separator gives the tile's output offset; the tile's output is put together in LDS and leaves in 16-byte stores. status: one zeroed u64 per tile.
 * *n_out = codes written (<= n + marks * k; out_cap bounds the stores, KERR_CAPACITY beyond it). */
constexpr u32 S1_HC_NONE = 0xFFFFFFFFu;
__device__ __forceinline__ u32 s1_hc_key(int8_t c) { return c < 0 ? 4u : (u32)(c & 3); }

__global__ void __launch_bounds__(S1_BLOCK) k_s1_hc_compact(const int8_t *__restrict__ codes, u64 n, u32 k, u64 *status, u32 *ticket_ctr, int8_t *__restrict__ out,
                                                             u64 out_cap, u64 *n_out, u32 *err)
{
	__shared__ __attribute__((aligned(16))) int8_t s_out[S1_TXT_TILE + S1_MAX_K + 32]; /* 15 bytes of alignment + the tile's codes + tail + separator */
	__shared__ u32 s_tmp[S1_BLOCK / 64 + 1];
	__shared__ u64 s_carry;
	__shared__ u32 s_ticket, s_mark, s_mark_rank;
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	if (tid == 0) {
		s_ticket = atomicAdd(ticket_ctr, 1u);
		s_mark = S1_HC_NONE;
	}
	__syncthreads();
	const u32 tile = s_ticket;
	const u32 num_tiles = (u32)((n + S1_TXT_TILE - 1) / S1_TXT_TILE);
	if (tile >= num_tiles)
		return;
	const u64 tile0 = (u64)tile * S1_TXT_TILE, p0 = tile0 + (u64)tid * S1_TXT_PER;
	int8_t c[S1_TXT_PER];
	static_assert(S1_TXT_PER == 16, "one 16-byte load per thread");
	if (p0 + S1_TXT_PER <= n) {
		u32 w[4];
		__builtin_memcpy(w, codes + p0, 16);
#pragma unroll
		for (int j = 0; j < S1_TXT_PER; ++j)
			c[j] = (int8_t)(w[j >> 2] >> (8 * (j & 3)));
	} else {
#pragma unroll
		for (int j = 0; j < S1_TXT_PER; ++j)
			c[j] = p0 + j < n ? codes[p0 + j] : (int8_t)-1;
	}
	/* ---- main role: the code differs from the one in front, or is the first of the stream, or starts a piece */
	u32 prev = p0 > 0 && p0 < n ? s1_hc_key(codes[p0 - 1]) : 5u; /* 5: nothing in front */
	u32 keep = 0, my_mark = S1_HC_NONE;
#pragma unroll
	for (int j = 0; j < S1_TXT_PER; ++j) {
		if (p0 + j >= n)
			break;
		const u32 key = s1_hc_key(c[j]);
		const bool marked = (c[j] & 0xC0) == S1_PIECE_MARK;
		if (key != prev || marked)
			keep |= 1u << j;
		if (marked)
			my_mark = (u32)j;
		prev = key;
	}
	u32 tile_keep;
	const u32 keep_before = block_excl_sum<S1_BLOCK / 64, u32>((u32)__popc(keep), s_tmp, tile_keep);
	if (my_mark != S1_HC_NONE) { /* one thread of the tile at most */
		s_mark = tid * S1_TXT_PER + my_mark;
		s_mark_rank = keep_before + (u32)__popc(keep & ((1u << my_mark) - 1u));
	}
	__syncthreads();
	/* ---- tail role (rare, tile-uniform): thread t takes position M + t of [M, M + k - 1); ranks from the waves' ballots */
	const u32 mk = s_mark;
	u32 tail_cnt = 0, tail_rank = 0, extra = 0;
	bool tail_keep = false;
	int8_t tail_code = -1;
	if (mk != S1_HC_NONE) {
		const u64 q = tile0 + mk + tid;
		if (tid + 1 < k && q < n) {
			const int8_t a = codes[q];
			tail_keep = s1_hc_key(a) != (q > 0 ? s1_hc_key(codes[q - 1]) : 5u);
			tail_code = a < 0 ? (int8_t)-1 : (int8_t)(a & 3);
		}
		const u64 bal = __ballot(tail_keep);
		const u32 below = __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u));
		if (lane == 0)
			s_tmp[wave] = (u32)__popcll(bal);
		__syncthreads();
#pragma unroll
		for (u32 i = 0; i < (u32)S1_BLOCK / 64; ++i) {
			tail_rank += i < wave ? s_tmp[i] : 0u;
			tail_cnt += s_tmp[i];
		}
		tail_rank += below;
		extra = tail_cnt + 1; /* + the separator */
	}
	const u32 tile_out = tile_keep + extra;
	if (wave == 0) {
		const u64 excl = lookback64(status, tile, (u64)tile_out, lane, err, KERR_WATCHDOG | KERR_AT_STAGE1);
		if (lane == 0) {
			s_carry = excl;
			if (tile == num_tiles - 1)
				*n_out = excl + tile_out;
		}
	}
	__syncthreads();
	const u64 at0 = s_carry;
	if (at0 + tile_out > out_cap) { /* tile-uniform; cannot happen with the chain's sizing */
		if (tid == 0)
			atomicOr(err, KERR_CAPACITY);
		return;
	}
	/* ---- the tile's output in LDS, shifted by the misalignment of its place in `out`: 16-byte chunks of s_out are 16-byte chunks of `out` */
	const u32 mis = (u32)((uintptr_t)(out + at0) & 15u);
	u32 idx = mis + keep_before + (tid * S1_TXT_PER > mk && mk != S1_HC_NONE ? extra : 0u);
#pragma unroll
	for (int j = 0; j < S1_TXT_PER; ++j) {
		if (tid * S1_TXT_PER + (u32)j == mk)
			idx += extra; /* the tail and its separator go in front of the marked code */
		if (keep & (1u << j))
			s_out[idx++] = c[j] < 0 ? (int8_t)-1 : (int8_t)(c[j] & 3);
	}
	if (mk != S1_HC_NONE) {
		if (tail_keep)
			s_out[mis + s_mark_rank + tail_rank] = tail_code;
		if (tid == 0)
			s_out[mis + s_mark_rank + tail_cnt] = (int8_t)-1;
	}
	__syncthreads();
	int8_t *dst = out + at0 - mis; /* 16-byte aligned */
	const u32 lo_valid = mis, hi_valid = mis + tile_out;
	for (u32 ch = tid; ch * 16u < hi_valid; ch += S1_BLOCK) {
		const u32 lo = ch * 16u;
		if (lo >= lo_valid && lo + 16u <= hi_valid) {
			uint4 v;
			__builtin_memcpy(&v, __builtin_assume_aligned(s_out + lo, 16), 16);
			__builtin_memcpy(__builtin_assume_aligned(dst + lo, 16), &v, 16);
		} else
			for (u32 i = lo > lo_valid ? lo : lo_valid; i < lo + 16u && i < hi_valid; ++i)
				dst[i] = s_out[i];
	}
}

/* ------------------------------------------------------------------------------------------------ BAM records (-fbam)
 * The reference's BAM readers inflate BGZF on the host, take the file header off and hand the splitter parts that hold whole alignment records only
 * (fastq_reader.cpp:191-362, ReadType::na). CSplitter::GetSeq's BAM branch (splitter.cpp:326-419) walks them: a record is
 *     block_size:i32 | refID pos | bin_mq_nl:u32 | flag_nc:u32 | l_seq:i32 | next_refID next_pos tlen | name | cigar | (l_seq + 1) / 2 nibble bytes | qualities | tags
 * and the next one starts 4 + block_size bytes on. l_read_name is the low byte of bin_mq_nl, n_cigar_op the low half of flag_nc, the flags its high half. A
 * record with flag 0x100 or 0x800 is skipped (not counted); any other is one read, its bases decoded from "=ACMGRSVTWYHKDBN" (A C G T -> 0..3, all else
 * invalid), first base in the high nibble; without both_strands a record with flag 0x10 is written back to front and complemented.
 * The reference writes a record's bases into a buffer of line_cap symbols without a bound, so an included record with l_seq >= line_cap has no result to
 * reproduce: S1_TEXT_BAD, as is a chain that does not end exactly at the part's end, a block_size below 32 + name + cigar + bases + qualities (a negative one
 * included), a negative l_seq and a header that runs past the part. Every byte read is inside [0, n); no piece marks are made.
 *
 * k_s1_bam_chain finds the record starts. The chain has no entry points but offset 0, and one lane hopping through global memory costs about a microsecond per
 * record (see k_parse_packs in kernels.hip.h). Ticketed tiles of S1_BAM_TILE bytes: a tile first resolves in LDS, for EVERY byte offset o of the tile taken
 * as a record start, where the chain from o leaves the tile and after how many records — one 64-bit entry per offset (low half: offset relative to the tile,
 * S1_BAM_BAD when the chain meets a block_size below 32 or runs past the part; high half: hops), by pointer doubling: a hop is 36 bytes at least, so the
 * S1_BAM_TILE / 36 hops a tile can hold are done in S1_BAM_ROUNDS rounds, fewer when no chain is left inside (real records are hundreds of bytes). Only then
 * does it wait for the tile in front, which hands over the true entry offset and the number of records before it in ONE relaxed agent-scope 64-bit word that
 * is flag, count and offset at once (nothing else is communicated, so nothing needs ordering); one LDS read later the tile publishes its own word. A record
 * longer than a tile passes through the tiles it covers (entry at or past their end: they publish what they received). Off that critical path one lane then
 * walks the true chain through the tile's bytes in LDS and writes the record offsets, in order, to rec_off (u32: the chain refuses parts of 2 GiB and more).
 * A tile that finds its entry bad raises S1_TEXT_BAD and publishes n, so that no later tile waits or walks. totals[0] = records. status: one zeroed u64 per tile. */
constexpr int S1_BAM_PER = 32, S1_BAM_TILE = S1_BLOCK * S1_BAM_PER;
constexpr u32 S1_BAM_MIN_HOP = 36; /* the block_size word + the 32 fixed bytes behind it */
constexpr int S1_BAM_ROUNDS = 8;
static_assert((1 << S1_BAM_ROUNDS) >= S1_BAM_TILE / (int)S1_BAM_MIN_HOP + 1, "pointer doubling covers the longest chain inside a tile");
constexpr u32 S1_BAM_BAD = 0xFFFFFFFFu;
constexpr u64 S1_BAM_MAX_PART = 1ull << 31;
constexpr u64 S1_BAM_ST_FLAG = 1ull << 63, S1_BAM_ST_OFF_MASK = (1ull << 36) - 1; /* [63] published | [62:36] records before | [35:0] entry offset in the part */

/* the little-endian 32-bit word at byte `at` of an LDS array that is readable up to the aligned word behind it */
__device__ __forceinline__ u32 s1_bam_lds_word(const uint8_t *s, u32 at)
{
	const u32 *w = reinterpret_cast<const u32 *>(s);
	const u64 both = ((u64)w[(at >> 2) + 1] << 32) | w[at >> 2];
	return (u32)(both >> (8u * (at & 3u)));
}
/* where the record at offset o of the tile ends, relative to the tile; S1_BAM_BAD if it cannot be one */
__device__ __forceinline__ u32 s1_bam_hop(const uint8_t *s_b, u32 o, u64 tile0, u64 n)
{
	if (tile0 + o + 4 > n)
		return S1_BAM_BAD;
	const int bs = (int)s1_bam_lds_word(s_b, o);
	if (bs < 32 || tile0 + o + 4 + (u64)bs > n)
		return S1_BAM_BAD;
	return o + 4u + (u32)bs;
}

__global__ void __launch_bounds__(S1_BLOCK) k_s1_bam_chain(const uint8_t *__restrict__ text, u64 n, u64 *status, u32 *ticket_ctr, u32 *__restrict__ rec_off, u64 rec_cap,
                                                            u64 *totals, u32 *err)
{
	__shared__ __attribute__((aligned(16))) uint8_t s_b[S1_BAM_TILE + 16]; /* the tile and the bytes a block_size word at its end reaches into */
	__shared__ u64 s_j[S1_BAM_TILE];
	__shared__ u32 s_ticket, s_moved[2];
	__shared__ u64 s_entry, s_first;
	const u32 tid = threadIdx.x;
	if (tid == 0) {
		s_ticket = atomicAdd(ticket_ctr, 1u);
		s_moved[0] = s_moved[1] = 0;
	}
	__syncthreads();
	const u32 tile = s_ticket;
	const u32 num_tiles = (u32)((n + S1_BAM_TILE - 1) / S1_BAM_TILE);
	if (tile >= num_tiles)
		return;
	const u64 tile0 = (u64)tile * S1_BAM_TILE;
	const u32 tlen = n - tile0 < (u64)S1_BAM_TILE ? (u32)(n - tile0) : (u32)S1_BAM_TILE;
	static_assert(S1_BAM_PER % 16 == 0, "16-byte loads");
#pragma unroll
	for (u32 i = 0; i < (u32)S1_BAM_PER / 16 + 1; ++i) {
		const u32 off = (i * S1_BLOCK + tid) * 16;
		if (off >= (u32)S1_BAM_TILE + 16)
			break;
		const u64 p = tile0 + off;
		uint4 v;
		if (p + 16 <= n)
			__builtin_memcpy(&v, text + p, 16);
		else {
			uint8_t b[16];
#pragma unroll
			for (int j = 0; j < 16; ++j)
				b[j] = p + j < n ? text[p + j] : (uint8_t)0;
			__builtin_memcpy(&v, b, 16);
		}
		__builtin_memcpy(__builtin_assume_aligned(s_b + off, 16), &v, 16);
	}
	__syncthreads();
	/* one hop from every offset (thread t takes offsets t, t + 256, ...: neighbouring lanes, neighbouring LDS words) */
#pragma unroll 4
	for (u32 j = 0; j < (u32)S1_BAM_PER; ++j) {
		const u32 o = j * S1_BLOCK + tid;
		s_j[o] = (1ull << 32) | (o < tlen ? s1_bam_hop(s_b, o, tile0, n) : S1_BAM_BAD);
	}
	__syncthreads();
	for (u32 r = 0; r < (u32)S1_BAM_ROUNDS; ++r) {
		u64 v[S1_BAM_PER];
		bool moved = false;
#pragma unroll
		for (u32 j = 0; j < (u32)S1_BAM_PER; ++j) {
			u64 a = s_j[j * S1_BLOCK + tid];
			if ((u32)a < tlen) { /* still inside: take the hops of where it stands */
				const u64 b = s_j[(u32)a];
				a = (((a >> 32) + (b >> 32)) << 32) | (u32)b;
				moved = true;
			}
			v[j] = a;
		}
		if (moved)
			s_moved[r & 1] = 1;
		__syncthreads();
#pragma unroll
		for (u32 j = 0; j < (u32)S1_BAM_PER; ++j)
			s_j[j * S1_BLOCK + tid] = v[j];
		if (tid == 0)
			s_moved[(r + 1) & 1] = 0;
		__syncthreads();
		if (!s_moved[r & 1])
			break;
	}
	/* ---- the entry from the tile in front, this tile's word */
	if (tid == 0) {
		u64 entry = 0, before = 0;
		if (tile) {
			LbWatch watch;
			u64 v;
			while (!((v = ld_agent(&status[tile - 1])) & S1_BAM_ST_FLAG)) {
				if (lb_blocked(watch, err)) {
					lb_gave_up(watch, err, KERR_WATCHDOG | KERR_AT_STAGE1, 0u, tile, (long long)tile - 1, num_tiles);
					v = n; /* nothing to walk, here and behind */
					break;
				}
				__builtin_amdgcn_s_sleep(1);
			}
			entry = v & S1_BAM_ST_OFF_MASK;
			before = (v & ~S1_BAM_ST_FLAG) >> 36;
		}
		u64 exit_at = entry, here = 0;
		bool bad = false;
		if (entry < tile0 + tlen) { /* tile0 <= entry: it is where a chain left the tiles in front */
			const u64 a = s_j[(u32)(entry - tile0)];
			if ((u32)a == S1_BAM_BAD || (u32)a < tlen)
				bad = true;
			else {
				exit_at = tile0 + (u32)a;
				here = a >> 32;
			}
		}
		if (tile == num_tiles - 1 && exit_at != n)
			bad = true; /* the chain ends exactly at the end of the part (an entry beyond it arrives here too) */
		if (bad) {
			atomicOr(err, S1_TEXT_BAD);
			exit_at = n;
			here = 0;
		}
		st_agent(&status[tile], S1_BAM_ST_FLAG | ((before + here) << 36) | exit_at);
		if (tile == num_tiles - 1)
			totals[0] = before + here;
		s_entry = bad ? n : entry;
		s_first = before;
	}
	__syncthreads();
	/* ---- the true starts of this tile, in order */
	if (tid == 0) {
		u64 idx = s_first;
		for (u64 q = s_entry; q < tile0 + tlen && idx < rec_cap; ++idx) {
			const u32 to = s1_bam_hop(s_b, (u32)(q - tile0), tile0, n);
			if (to == S1_BAM_BAD)
				break; /* reported above */
			rec_off[idx] = (u32)q;
			q = tile0 + to;
		}
	}
}

/* k_s1_bam_decode: the records at rec_off[0 .. n_rec) -> the code stream of the kernels above: for every included record with bases ONE negative separator
 * and its l_seq codes (k_s1_ml_text_to_codes's convention for a title: the separator stands in front of its sequence); an included record without bases is
 * counted and writes nothing. Ticketed tiles of S1_BLOCK records: a thread checks one record's header (the rules in the comment above), one block sum + one
 * decoupled look-back over (codes | included records << 34) give the tile's place in the stream, then the tile's bases are decoded by all threads in units of
 * 16 codes = one ALIGNED 16-byte store: a unit finds its record by bisection over the tile's unit counts in LDS, loads the 8 or 9 nibble bytes under it at once
 * and turns them in registers (back to front and complemented for a reversed record). Units at the ends of a record store bytes.
 * totals[0] = reads, totals[1] = codes; out_cap bounds the stores (2 n + 16 always suffices: a record's 36 bytes pay for its separator). status: one zeroed
 * u64 per tile. */
constexpr u64 S1_BAM_CNT_SHIFT = 34, S1_BAM_LEN_MASK = (1ull << S1_BAM_CNT_SHIFT) - 1;

__device__ __forceinline__ u32 s1_bam_u32(const uint8_t *p)
{
	u32 v;
	__builtin_memcpy(&v, p, 4);
	return v;
}

__global__ void __launch_bounds__(S1_BLOCK) k_s1_bam_decode(const uint8_t *__restrict__ text, u64 n, const u32 *__restrict__ rec_off, u64 n_rec, u32 both_strands, u64 line_cap,
                                                             u64 *status, u32 *ticket_ctr, int8_t *__restrict__ codes, u64 out_cap, u64 *totals, u32 *err)
{
	__shared__ u64 s_tmp64[S1_BLOCK / 64 + 1];
	__shared__ u32 s_tmp[S1_BLOCK / 64 + 1];
	__shared__ u64 s_carry;
	__shared__ u32 s_ticket;
	__shared__ u32 s_src[S1_BLOCK], s_len[S1_BLOCK], s_unit0[S1_BLOCK + 1]; /* first nibble byte | l_seq, bit 31: reversed | units before the record */
	__shared__ u64 s_at[S1_BLOCK];                                            /* the record's first code in the stream */
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	if (tid == 0)
		s_ticket = atomicAdd(ticket_ctr, 1u);
	__syncthreads();
	const u32 tile = s_ticket;
	const u32 num_tiles = (u32)((n_rec + S1_BLOCK - 1) / S1_BLOCK);
	if (tile >= num_tiles)
		return;
	const u64 r = (u64)tile * S1_BLOCK + tid;
	u32 l_seq = 0, src = 0, rev = 0, included = 0;
	if (r < n_rec) {
		const u64 off = rec_off[r];
		bool bad = off + S1_BAM_MIN_HOP > n; /* the header runs past the part */
		if (!bad) {
			const int bs = (int)s1_bam_u32(text + off), ls = (int)s1_bam_u32(text + off + 20);
			const u32 bin_mq_nl = s1_bam_u32(text + off + 12), flag_nc = s1_bam_u32(text + off + 16);
			const u32 l_name = bin_mq_nl & 255u, n_cigar = flag_nc & 0xFFFFu, flags = flag_nc >> 16;
			bad = bs < 32 || ls < 0;
			if (!bad) {
				const u64 front = 32ull + l_name + 4ull * n_cigar, need = front + ((u64)ls + 1) / 2 + (u64)ls;
				bad = (u64)bs < need || off + 4 + (u64)bs > n;
				if (!bad && !(flags & 0x900u)) { /* neither secondary nor supplementary */
					if ((u64)ls >= line_cap)
						bad = true; /* the reference's buffer holds line_cap symbols */
					else {
						included = 1;
						l_seq = (u32)ls;
						src = (u32)(off + 4 + front);
						rev = !both_strands && (flags & 0x10u) ? 1u : 0u;
					}
				}
			}
		}
		if (bad) {
			atomicOr(err, S1_TEXT_BAD);
			included = l_seq = 0;
		}
	}
	const u64 mine = (l_seq ? (u64)l_seq + 1 : 0ull) | ((u64)included << S1_BAM_CNT_SHIFT);
	u64 tile_sum;
	const u64 before = block_excl_sum<S1_BLOCK / 64, u64>(mine, s_tmp64, tile_sum);
	if (wave == 0) {
		const u64 excl = lookback64(status, tile, tile_sum, lane, err, KERR_WATCHDOG | KERR_AT_STAGE1);
		if (lane == 0) {
			s_carry = excl;
			if (tile == num_tiles - 1) {
				totals[0] = (excl + tile_sum) >> S1_BAM_CNT_SHIFT;
				totals[1] = (excl + tile_sum) & S1_BAM_LEN_MASK;
			}
		}
	}
	__syncthreads();
	const u64 tile_at = s_carry & S1_BAM_LEN_MASK;
	if (tile_at + (tile_sum & S1_BAM_LEN_MASK) > out_cap) { /* tile-uniform; cannot happen with the chain's sizing */
		if (tid == 0)
			atomicOr(err, KERR_CAPACITY);
		return;
	}
	const u64 at = tile_at + (before & S1_BAM_LEN_MASK) + 1; /* behind the separator */
	u32 units = 0;
	if (l_seq) {
		codes[at - 1] = (int8_t)-1;
		const uintptr_t a = (uintptr_t)(codes + at);
		units = (u32)((((a + l_seq + 15) & ~(uintptr_t)15) - (a & ~(uintptr_t)15)) >> 4);
	}
	u32 tile_units;
	const u32 unit0 = block_excl_sum<S1_BLOCK / 64, u32>(units, s_tmp, tile_units);
	s_src[tid] = src;
	s_len[tid] = l_seq | (rev << 31); /* l_seq < 2^31 */
	s_at[tid] = at;
	s_unit0[tid] = unit0;
	if (tid == 0)
		s_unit0[S1_BLOCK] = tile_units;
	__syncthreads();
	for (u32 u = tid; u < tile_units; u += S1_BLOCK) {
		u32 lo = 0, hi = S1_BLOCK; /* the record with s_unit0[rec] <= u < s_unit0[rec + 1] */
#pragma unroll
		for (int step = 0; step < 8; ++step) {
			const u32 mid = (lo + hi) >> 1;
			if (s_unit0[mid] <= u)
				lo = mid;
			else
				hi = mid;
		}
		static_assert(S1_BLOCK == 256, "eight halvings");
		const u32 len = s_len[lo] & 0x7FFFFFFFu;
		const bool back = (s_len[lo] >> 31) != 0;
		const u64 rec_at = s_at[lo];
		int8_t *unit = (int8_t *)((((uintptr_t)(codes + rec_at)) & ~(uintptr_t)15) + 16 * (uintptr_t)(u - s_unit0[lo])); /* 16-byte aligned */
		const long long j0 = (long long)(unit - (codes + rec_at));                                                       /* the base the unit's first byte holds; < 0 in a record's first unit */
		const u32 j_lo = j0 < 0 ? 0u : (u32)j0, j_hi = j0 + 16 < (long long)len ? (u32)(j0 + 16) : len;                  /* bases [j_lo, j_hi) */
		const u32 i_min = back ? len - j_hi : j_lo, i_max = back ? len - 1 - j_lo : j_hi - 1;                            /* as the record stores them */
		const u32 b0 = i_min >> 1;
		const u64 p = (u64)s_src[lo] + b0;
		u64 w = 0;
		u32 w8 = 0;
		if (p + 9 <= n) {
			__builtin_memcpy(&w, text + p, 8);
			w8 = text[p + 8];
		} else
			for (u32 t = 0; t <= (i_max >> 1) - b0; ++t) {
				const u64 byte = p + t < n ? text[p + t] : 0u;
				if (t < 8)
					w |= byte << (8 * t);
				else
					w8 = (u32)byte;
			}
		int8_t c[16];
#pragma unroll
		for (int t = 0; t < 16; ++t) {
			const long long j = j0 + t;
			const u32 i = back ? len - 1 - (u32)j : (u32)j;
			const u32 bi = (i >> 1) - b0;
			const u32 byte = bi < 8 ? (u32)(w >> (8 * bi)) & 255u : w8;
			const u32 nib = (i & 1u) ? byte & 15u : byte >> 4;
			const int code = (nib & (nib - 1u)) == 0 && nib ? __ffs((int)nib) - 1 : -1; /* 1 2 4 8 = A C G T */
			c[t] = (int8_t)(code < 0 ? -1 : back ? 3 - code : code);
		}
		if (j_lo == (u32)j0 && j0 >= 0 && j_hi == (u32)j0 + 16u) {
			uint4 v;
			__builtin_memcpy(&v, c, 16);
			__builtin_memcpy(__builtin_assume_aligned(unit, 16), &v, 16);
		} else {
#pragma unroll
			for (int t = 0; t < 16; ++t)
				if (j0 + t >= (long long)j_lo && j0 + t < (long long)j_hi)
					unit[t] = c[t];
		}
	}
}

/* ------------------------------------------------------------------------------------------------ histogram estimate while counting (--opt-out-size)
 * With --opt-out-size the reference hashes every k-mer of every buffer GetSeq returns a second time (CntHashEstimator::Process, called at splitter.cpp:576-577
 * in front of the homopolymer compression) and counts a sample of the hashes in two arrays of 2^r 32-bit counters; stage 2 picks lut_prefix_len from the
 * histogram estimated from them (kmc.h:1436-1468), so the database's bytes depend on the counters. Restated as a function of one window of k valid symbols
 * c_0 .. c_(k-1) (codes 0..3 = A C G T):
 *     fh = XOR_j rot^(k-1-j)(seed[c_j])      rh = XOR_j rot^j(seed[3 - c_j])      h = min(fh, rh)
 * where rot turns the low 33 bits and the high 31 bits of a word left by one, each on their own. With pref = h >> (63 - s): pref == 1 adds one to
 * counters[0][h & (2^r - 1)], (pref >> 1) == 2^(s-1) - 1 adds one to counters[1][same] (both at s = 1 when the two top bits are 0 1); counters wrap at 2^32.
 * The reference's rolling form is that function and nothing else (an invalid symbol empties its window). The pieces of an over-long line, of a long-read part
 * and of a multi-line sequence overlap by k - 1 symbols, so every window lies in exactly one return: the estimate is over EVERY window of k valid codes of the
 * RAW code stream (before k_s1_hc_compact), S1_PIECE_MARK is ignored (a marked code is a valid symbol), separators and N are invalid.
 *
 * k_s1_nthash_estimate: one workgroup per tile of S1_TXT_TILE start positions (the tile index is the block index: nothing is carried from tile to tile, a window
 * depends on k codes), the tile and its k - 1 halo codes in LDS (16 bytes per thread, as the neighbours load). A thread owns a strip of L consecutive start
 * positions and streams over its L + k - 1 codes as the reference does over a read: the first k - 1 steps fill the window, every later step takes one code in
 * and one out; an invalid code empties the window, which fills again behind it. A step is 97 instructions in the gfx950 build (scalar ones and the two LDS
 * byte reads included; the adds of a wave with an accepted lane come on top), with the reference's seeds picked per code from kernel arguments (four tables of four
 * words: the seeds as they enter fh and rh and as they leave them; two 4-way selects are cheaper than one 16-way select from the reference's out-by-in
 * table). L = 16 up to k = 64: all 256 threads work, (16 + k - 1) / 16 steps per k-mer = 2.6 at k = 27, about 255 instructions per k-mer. Beyond, L = 64 and
 * one wave works: fewer, longer strips cost fewer instructions whenever a whole wave is busy (4 x (15 + k) wave-steps per tile with L = 16 against 63 + k
 * with L = 64), and at k = 255 that is 318 / 64 = 5.0 steps, about 480 instructions per k-mer instead of 1 640. 35 VGPRs, no scratch.
 * The accepted hashes (2^-s of the k-mers per counter array) of a wave's step are added per distinct index (s1_nt_count): one relaxed agent-scope atomic add
 * of the number of lanes that hold it; counters: type 0 first, 2^r entries each. */
struct S1NtSeeds {
	u64 in_f[4], in_r[4], out_f[4], out_r[4]; /* by code: what an incoming symbol adds to fh, and to rh in front of its turn back; what the outgoing one takes away */
};
__host__ __device__ __forceinline__ u64 s1_nt_rot(u64 v)
{
	const u64 lo = v & 0x1FFFFFFFFull, hi = v >> 33;
	return (((lo << 1) | (lo >> 32)) & 0x1FFFFFFFFull) | ((((hi << 1) | (hi >> 30)) & 0x7FFFFFFFull) << 33);
}
__host__ __device__ __forceinline__ u64 s1_nt_rot_back(u64 v)
{
	const u64 lo = v & 0x1FFFFFFFFull, hi = v >> 33;
	return ((lo >> 1) | ((lo & 1) << 32)) | (((hi >> 1) | ((hi & 1) << 30)) << 33);
}
/* the four base seeds of ntHash (A, C, G, T); everything else is generated from them */
static inline S1NtSeeds s1_nt_seeds(u32 k)
{
	const u64 seed[4] = {0x3c8bfbb395c60474ull, 0x3193c18562a02b4cull, 0x20323ed082572324ull, 0x295549f54be24456ull};
	S1NtSeeds T;
	for (u32 c = 0; c < 4; ++c) {
		u64 turned = seed[c];
		for (u32 i = 0; i < k; ++i)
			turned = s1_nt_rot(turned);
		T.in_f[c] = seed[c];
		T.out_f[c] = turned;
		T.in_r[3 - c] = turned;
		T.out_r[3 - c] = seed[c];
	}
	return T;
}
__device__ __forceinline__ u64 s1_nt_pick(const u64 (&t)[4], u32 c)
{
	const u64 a = c & 1u ? t[1] : t[0], b = c & 1u ? t[3] : t[2];
	return c & 2u ? b : a;
}

/* one add per DISTINCT accepted index of the wave, of the number of lanes that hold it: the lanes of a wave walk neighbouring strips, and inside a homopolymer or a
 * short tandem repeat they all hold the same k-mer. Left to 64 single adds, a k-mer with 2 M copies costs 11.4 ns per copy (measured): ten times the
 * rest of its part. Called by whole waves only. */
__device__ __forceinline__ void s1_nt_count(u32 *__restrict__ counters, u32 idx, bool hit)
{
	u64 todo = __ballot(hit);
	while (todo) { /* wave-uniform */
		const u32 leader = (u32)__ffsll((unsigned long long)todo) - 1u;
		const u32 at = __shfl(idx, (int)leader);
		const u64 same = __ballot(hit && idx == at); /* holds the leader's bit: the loop ends */
		if ((threadIdx.x & 63u) == leader)
			__hip_atomic_fetch_add(counters + at, (u32)__popcll((unsigned long long)same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		todo &= ~same;
	}
}

__global__ void __launch_bounds__(S1_BLOCK) k_s1_nthash_estimate(const int8_t *__restrict__ codes, u64 n, u32 k, u32 s, u32 r, S1NtSeeds T, u32 *__restrict__ counters)
{
	__shared__ __attribute__((aligned(16))) int8_t s_c[S1_TXT_TILE + S1_MAX_K];
	static_assert(S1_TXT_PER == 16 && S1_MAX_K % 16 == 0, "16-byte loads: the tile by all threads, the halo by the first S1_MAX_K / 16");
	const u32 tid = threadIdx.x;
	const u64 tile0 = (u64)blockIdx.x * S1_TXT_TILE;
#pragma unroll
	for (u32 part = 0; part < 2; ++part) {
		if (part && tid >= (u32)S1_MAX_K / 16)
			break;
		const u32 off = part * S1_TXT_TILE + tid * 16;
		const u64 p0 = tile0 + off;
		uint4 v;
		if (p0 + 16 <= n)
			__builtin_memcpy(&v, codes + p0, 16);
		else {
			int8_t b[16];
#pragma unroll
			for (int j = 0; j < 16; ++j)
				b[j] = p0 + j < n ? codes[p0 + j] : (int8_t)-1;
			__builtin_memcpy(&v, b, 16);
		}
		__builtin_memcpy(__builtin_assume_aligned(s_c + off, 16), &v, 16);
	}
	__syncthreads();
	const u32 L = k <= 64 ? 16u : 64u;
	if (tid >= (u32)S1_TXT_TILE / L)
		return;
	const u32 q0 = tid * L, q1 = q0 + L + k - 1; /* q1 <= S1_TXT_TILE + S1_MAX_K - 1 */
	const u32 idx_mask = (1u << r) - 1u, top_shift = 31u - s, ones = (1u << (s - 1)) - 1u;
	u64 fh = 0, rh = 0;
	u32 len = 0; /* valid codes in the window, k at most */
	for (u32 q = q0; q < q1; ++q) {
		const int8_t cin = s_c[q];
		const bool ok = cin >= 0, full = len == k;
		const u32 c = (u32)cin & 3u, o = (u32)s_c[full ? q - k : q] & 3u; /* a full window began at q - k >= q0 */
		u64 f = s1_nt_rot(fh) ^ s1_nt_pick(T.in_f, c), rv = rh ^ s1_nt_pick(T.in_r, c);
		if (full) {
			f ^= s1_nt_pick(T.out_f, o);
			rv ^= s1_nt_pick(T.out_r, o);
		}
		fh = ok ? f : 0ull;
		rh = ok ? s1_nt_rot_back(rv) : 0ull;
		len = ok ? (full ? k : len + 1u) : 0u;
		/* every lane of the wave is here (the strips of a wave are equally long, a wave works whole or not at all) */
		const u64 h = fh < rh ? fh : rh;
		const u32 pref = (u32)(h >> 32) >> top_shift, idx = (u32)h & idx_mask;
		s1_nt_count(counters, idx, len == k && pref == 1u);
		s1_nt_count(counters + ((size_t)1 << r), idx, len == k && (pref >> 1) == ones);
	}
}

/* ------------------------------------------------------------------------------------------------ small k (k <= 13)
 * With k <= 13 the reference takes its "small k optimization" whenever it fits in memory (CKMC::AdjustMemoryLimitsSmallK, kmc.h:677-750; always when
 * k < signature_len): no signatures, no bins. CSplitter::ProcessReadsSmallK (splitter.cpp:682-805) rolls the k-mer and its reverse complement over every buffer
 * GetSeq returns (after HomopolymerCompressSeq with -hc) and does ++buf[kmer], ++total_kmers, kmer = min(forward, reverse complement) as 2k-bit integers with
 * both_strands, the forward k-mer without. Its omit_next_n_kmers bookkeeping: an invalid symbol at i < k - 1 sets it to i + 1 and the counting loop, which
 * starts at symbol k - 1, then skips the windows that end at k - 1 .. k - 1 + i — those that start at 0 .. i, all that hold symbol i; an invalid symbol at
 * i >= k - 1 sets it to k and skips the windows that end at i .. i + k - 1, again all that hold it; a later invalid symbol only ever raises the count that
 * is left. So: a window is counted iff it holds no invalid code, a return shorter than k adds nothing, and k = 1 is legal. The pieces of over-long lines, of
 * long-read parts and of multi-line sequences overlap by k - 1 symbols: every window of a line lies in exactly one piece, and the windows of the returns are
 * the windows of the RAW code stream with S1_PIECE_MARK ignored (as for k_s1_nthash_estimate) or, with -hc, of the stream k_s1_hc_compact leaves.
 *
 * k_s1_smallk_count<LDS_K>: direct-address counting into 4^k 64-bit counters in HBM (8 bytes at k = 1, 512 MB at k = 13). Workgroups are persistent: a
 * workgroup takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of S1_TXT_TILE start positions; tile and k - 1 <= 12 halo codes in LDS (16 bytes per
 * thread, the halo by thread 0), a strip of 16 consecutive start positions per thread, the forward and the reverse-complement k-mer rolled in one 32-bit
 * register each (26 bits at most), the number of valid codes since the strip's start (k at most) decides validity. Equal k-mers that follow each other in a
 * strip are merged before they are added: a homopolymer is one add of 16 per strip, not 16 adds to one address.
 *   LDS_K > 0 (k <= LDS_K): a workgroup-private table of 4^LDS_K 32-bit counters in LDS, filled with LDS atomics and flushed ONCE per workgroup, non-zero
 *     entries only, by relaxed agent-scope 64-bit adds. A workgroup walks at most S1_SMALLK_MAX_TILES_PER_WG tiles (2^31 windows: no counter wraps).
 *   LDS_K = 0: 64-bit adds without return straight into the table. The lanes of a wave walk neighbouring strips and inside a homopolymer or a tandem repeat whose
 *     period divides 16 they all hold one k-mer: the lanes that hold the k-mer of the first adding lane are added once, by that lane (one round of the
 *     per-distinct-index aggregation of s1_nt_count, whose full loop would cost random text 64 rounds per step); the others add for themselves.
 * *total += the windows counted: one add per workgroup. No look-back, no spin loop. */
constexpr u32 S1_SMALLK_MAX_K = 13, S1_SMALLK_LDS_K = 7, S1_SMALLK_WGS = 1024;
constexpr u64 S1_SMALLK_MAX_TILES_PER_WG = 1ull << 19;
static_assert(S1_SMALLK_MAX_K - 1 <= 16 && S1_TXT_PER == 16, "the halo is one 16-byte load; a strip is a thread's 16 positions");

/* called by whole waves only. T: the table's counters (u64: the small-k table; u32: k_s1_sig_stats's, which wrap like the reference's). REPEAT: another round for
 * as long as the last one merged lanes — a satellite puts the lanes of a wave on two signatures, and the second one's lanes would add one by one; random text, where
 * the first adding lane is alone with its index, still pays one round */
template <class T, bool REPEAT = false> __device__ __forceinline__ void s1_smallk_add(T *__restrict__ table, u32 idx, u32 cnt, bool emit)
{
	const u32 lane = threadIdx.x & 63u;
	for (;;) {
		const u64 todo = __ballot(emit);
		if (!todo) /* wave-uniform */
			return;
		const u32 leader = (u32)__ffsll((unsigned long long)todo) - 1u;
		const u32 at = __shfl(idx, (int)leader);
		const bool mine = emit && idx == at;
		const u64 same = __ballot(mine);
		if (__popcll((unsigned long long)same) > 1) { /* wave-uniform */
			const u32 sum = __shfl(wave_sum<u32>(mine ? cnt : 0u), 0);
			if (lane == leader)
				__hip_atomic_fetch_add(table + at, (T)sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			emit = emit && !mine;
			if (REPEAT)
				continue;
		}
		break;
	}
	if (emit)
		__hip_atomic_fetch_add(table + idx, (T)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int LDS_K>
__global__ void __launch_bounds__(S1_BLOCK) k_s1_smallk_count(const int8_t *__restrict__ codes, u64 n, u32 k, u32 both_strands, u64 *__restrict__ table, u64 *total)
{
	static_assert(LDS_K >= 0 && LDS_K <= 7, "4^LDS_K 32-bit counters beside the tile");
	constexpr u32 TAB = LDS_K ? 1u << (2 * LDS_K) : 1u;
	__shared__ __attribute__((aligned(16))) int8_t s_c[S1_TXT_TILE + 16];
	__shared__ u32 s_tab[TAB];
	__shared__ u64 s_sum[S1_BLOCK / 64];
	const u32 tid = threadIdx.x;
	const u64 num_tiles = (n + S1_TXT_TILE - 1) / S1_TXT_TILE;
	const u32 entries = 1u << (2 * k), mask = entries - 1u, rev_shift = 2 * (k - 1); /* k <= 13 (and <= LDS_K where there is one): the launcher's promise */
	if (LDS_K)
		for (u32 i = tid; i < entries && i < TAB; i += S1_BLOCK)
			s_tab[i] = 0;
	u32 counted = 0;
	for (u64 tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) { /* the same trips for every thread of the workgroup */
		const u64 tile0 = tile * S1_TXT_TILE;
		__syncthreads(); /* the strips of the tile before are walked (first trip: the table is zero) */
#pragma unroll
		for (u32 part = 0; part < 2; ++part) {
			if (part && tid)
				break;
			const u32 off = part * S1_TXT_TILE + tid * 16;
			const u64 p0 = tile0 + off;
			uint4 v;
			if (p0 + 16 <= n)
				__builtin_memcpy(&v, codes + p0, 16);
			else {
				int8_t b[16];
#pragma unroll
				for (int j = 0; j < 16; ++j)
					b[j] = p0 + j < n ? codes[p0 + j] : (int8_t)-1;
				__builtin_memcpy(&v, b, 16);
			}
			__builtin_memcpy(__builtin_assume_aligned(s_c + off, 16), &v, 16);
		}
		__syncthreads();
		const u32 q0 = tid * 16, q1 = q0 + 16 + k - 1; /* q1 <= S1_TXT_TILE + 12 */
		u32 f = 0, r = 0, len = 0, pidx = 0, pcnt = 0; /* pcnt copies of k-mer pidx wait to be added */
		for (u32 q = q0; q < q1; ++q) {
			const int8_t cin = s_c[q];
			const u32 c = (u32)cin & 3u; /* S1_PIECE_MARK masked off; what an invalid code leaves in f and r is pushed out by the k valid codes a window needs */
			f = ((f << 2) | c) & mask;
			r = (r >> 2) | ((3u - c) << rev_shift);
			len = cin >= 0 ? (len < k ? len + 1u : k) : 0u;
			const bool hit = len == k; /* k valid codes since q0: the window starts at q - k + 1, inside the strip */
			const u32 idx = both_strands && r < f ? r : f;
			const bool emit = hit && pcnt && idx != pidx;
			if (LDS_K) {
				if (emit)
					atomicAdd(&s_tab[pidx], pcnt);
			} else
				s1_smallk_add(table, pidx, pcnt, emit); /* every lane of the wave is here: the strips are equally long */
			if (hit) {
				pcnt = pcnt && idx == pidx ? pcnt + 1u : 1u;
				pidx = idx;
				++counted;
			}
		}
		if (LDS_K) {
			if (pcnt)
				atomicAdd(&s_tab[pidx], pcnt);
		} else
			s1_smallk_add(table, pidx, pcnt, pcnt != 0);
	}
	if (LDS_K) {
		__syncthreads();
		for (u32 i = tid; i < entries && i < TAB; i += S1_BLOCK) {
			const u32 v = s_tab[i];
			if (v)
				__hip_atomic_fetch_add(table + i, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
	const u64 wsum = wave_sum<u64>((u64)counted);
	if ((tid & 63u) == 0)
		s_sum[tid >> 6] = wsum;
	__syncthreads();
	if (tid == 0) {
		u64 all = 0;
#pragma unroll
		for (u32 w = 0; w < (u32)S1_BLOCK / 64; ++w)
			all += s_sum[w];
		if (all)
			__hip_atomic_fetch_add(total, all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

/* ------------------------------------------------------------------------------------------------ stage 0: signature statistics
 * CSplitter::CalcStats (splitter.cpp:439-533) walks the stage-0 sample as ProcessReads walks a part and adds 1 + len - kmer_len per super-k-mer to
 * _stats[signature] (uint32, wrapping). A super-k-mer is a maximal run of k-mers with one signature (the top of this file), so stats[s] is the number of valid
 * k-mer windows whose signature is s: a histogram over the code stream the front half leaves (the raw stream, or the -hc stream with -hc). The pieces of
 * over-long lines, long-read parts and multi-line sequences overlap by k - 1 symbols: every window lies in exactly one piece, S1_PIECE_MARK is ignored.
 *
 * k_s1_sig_stats<LDS_M>: 4^m + 1 32-bit counters in HBM, entry 4^m the special signature (no allowed m-mer in the window). Workgroups are persistent over tiles
 * of S1_STATS_TILE start positions (blockIdx.x, blockIdx.x + gridDim.x, ...); the tile's signatures come into LDS from s1_signatures_to_lds, S1_SUB calls of
 * S1_STATS_TILE / S1_SUB positions, each with its k - 1 halo codes — the m-mer, norm and window-minimum code of k_s1_signatures and k_s1_cut<true>. A thread then
 * walks a strip of S1_STATS_PER consecutive positions (an odd number: the lanes' LDS reads are bank-conflict free) and merges equal neighbours: neighbouring
 * k-mers share a signature for (k - m + 1) / 2 positions on average, and a run is one add of its length. Which positions of a strip a run came from does not
 * matter to the sum, so a pending run survives invalid positions and is added when another signature follows, or at the strip's end.
 *   LDS_M = 0: relaxed agent-scope adds without return straight into the table, behind the wave aggregation of s1_smallk_add, repeated while it merges lanes:
 *     inside a homopolymer or a satellite the lanes of a wave all hold one or two signatures, and each becomes one add; random text pays one round.
 *   LDS_M > 0 (m <= LDS_M): a workgroup-private table of 4^LDS_M + 1 counters in LDS, flushed once per workgroup, non-zero entries only. 32-bit and wrapping
 *     like the table itself: the result does not depend on the switch.
 * *total += the windows added, one add per workgroup. No look-back, no ticket, no spin loop. */
constexpr int S1_STATS_PER = 4 * S1_SUB - 1, S1_STATS_TILE = S1_BLOCK * S1_STATS_PER, S1_STATS_SUBTILE = S1_STATS_TILE / S1_SUB;
constexpr u32 S1_STATS_LDS_M = 7, S1_STATS_LDS_M_DEFAULT = 7, S1_STATS_WGS = 2048; /* _DEFAULT: the largest m that takes the LDS table unless the caller says otherwise */
static_assert(S1_STATS_SUBTILE * S1_SUB == S1_STATS_TILE && S1_STATS_SUBTILE <= S1_TILE + 2, "a sub-tile is one call of s1_signatures_to_lds");

template <int LDS_M>
__global__ void __launch_bounds__(S1_BLOCK) k_s1_sig_stats(const int8_t *__restrict__ codes, u64 n, u32 k, u32 m, u32 *__restrict__ table, u64 *total)
{
	static_assert(LDS_M == 0 || (LDS_M >= 5 && LDS_M <= (int)S1_STATS_LDS_M), "4^LDS_M + 1 32-bit counters beside the tile's signatures");
	constexpr u32 TAB = LDS_M ? (1u << (2 * LDS_M)) + 1u : 1u;
	__shared__ S1SigLds L;
	__shared__ u32 s_sig[S1_STATS_TILE];
	__shared__ u32 s_tab[TAB];
	__shared__ u64 s_sum[S1_BLOCK / 64];
	const u32 tid = threadIdx.x;
	const u32 entries = (1u << (2 * m)) + 1u; /* m <= LDS_M where there is an LDS table: the launcher's promise */
	const u64 n_pos = n - k + 1;              /* n >= k: the launcher's promise. A position behind n - k starts no window: its signature is S1_NOSIG */
	const u64 num_tiles = (n_pos + S1_STATS_TILE - 1) / S1_STATS_TILE;
	if (LDS_M)
		for (u32 i = tid; i < entries && i < TAB; i += S1_BLOCK)
			s_tab[i] = 0;
	u32 counted = 0;
	for (u64 tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) { /* the same trips for every thread of the workgroup */
		const u64 t0 = tile * S1_STATS_TILE;
		/* every call begins and ends with a barrier: the strips of the tile before are walked when s_sig is written (first trip: the table is zero) */
#pragma unroll 1
		for (int sub = 0; sub < S1_SUB; ++sub)
			s1_signatures_to_lds(codes, n, (long long)(t0 + (u64)sub * S1_STATS_SUBTILE), S1_STATS_SUBTILE, k, m, L, s_sig + sub * S1_STATS_SUBTILE);
		const u32 l0 = tid * S1_STATS_PER;
		u32 psig = 0, pcnt = 0; /* pcnt windows of signature psig wait to be added */
#pragma unroll
		for (int j = 0; j < S1_STATS_PER; ++j) {
			const u32 sg = s_sig[l0 + j];
			const bool hit = sg != S1_NOSIG;
			const bool emit = hit && pcnt && sg != psig;
			if (LDS_M) {
				if (emit)
					atomicAdd(&s_tab[psig], pcnt);
			} else
				s1_smallk_add<u32, true>(table, psig, pcnt, emit); /* every lane of the wave is here: the strips are equally long */
			if (hit) {
				pcnt = pcnt && sg == psig ? pcnt + 1u : 1u;
				psig = sg;
				++counted;
			}
		}
		if (LDS_M) {
			if (pcnt)
				atomicAdd(&s_tab[psig], pcnt);
		} else
			s1_smallk_add<u32, true>(table, psig, pcnt, pcnt != 0);
	}
	if (LDS_M) {
		__syncthreads();
		for (u32 i = tid; i < entries && i < TAB; i += S1_BLOCK) {
			const u32 v = s_tab[i];
			if (v)
				__hip_atomic_fetch_add(table + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
	const u64 wsum = wave_sum<u64>((u64)counted);
	if ((tid & 63u) == 0)
		s_sum[tid >> 6] = wsum;
	__syncthreads();
	if (tid == 0) {
		u64 all = 0;
#pragma unroll
		for (u32 w = 0; w < (u32)S1_BLOCK / 64; ++w)
			all += s_sum[w];
		if (all)
			__hip_atomic_fetch_add(total, all, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

/* n_plus_x_recs per bin: how many (k+x)-mer records the reference's stage 2 expands each super-k-mer into (kb_collector.cpp:83-100,
 * kb_collector.h:72-118) — the third sum a CKmerBinCollector keeps, which stage 2 sizes its arrays with. One thread per super-k-mer walks
 * its k-mers comparing the first four symbols of the k-mer with those of its reverse complement. */
__global__ void __launch_bounds__(256) k_s1_bin_plus_x(const int8_t *__restrict__ codes, const u64 *__restrict__ sk_pos, const u32 *__restrict__ sk_len,
                                                        const u32 *__restrict__ sk_sig, u64 n_sk, u32 k, u32 max_x, u32 both_strands, const int *__restrict__ sig_to_bin,
                                                        u32 n_bins, u64 *__restrict__ bin_plus_x)
{
	__shared__ u32 s_px[S1_MAX_BINS];
	for (u32 b = threadIdx.x; b < n_bins; b += 256)
		s_px[b] = 0;
	__syncthreads();
	const u64 i0 = (u64)blockIdx.x * S1_SK_TILE;
	for (u32 j = threadIdx.x; j < (u32)S1_SK_TILE && max_x; j += 256) {
		const u64 i = i0 + j;
		if (i >= n_sk)
			break;
		const int b = sig_to_bin[sk_sig[i]];
		if (b < 0 || (u32)b >= n_bins)
			continue;
		const u32 n = sk_len[i];
		u32 total;
		if (!both_strands)
			total = 1 + (n - k) / (max_x + 1);
		else {
			const int8_t *q = codes + sk_pos[i];
			/* & 3: a code may carry S1_PIECE_MARK */
			u32 fwd = ((u32)(q[0] & 3) << 6) | ((u32)(q[1] & 3) << 4) | ((u32)(q[2] & 3) << 2) | (u32)(q[3] & 3);
			u32 rc = ((3u - (q[k - 1] & 3)) << 6) | ((3u - (q[k - 2] & 3)) << 4) | ((3u - (q[k - 3] & 3)) << 2) | (3u - (q[k - 4] & 3));
			u32 state = fwd < rc ? 0u : (rc < fwd ? 1u : 2u), run = 0;
			total = 0;
			for (u32 t = 0; t + k < n; ++t) {
				rc = (rc >> 2) | ((3u - (q[k + t] & 3)) << 6);
				fwd = ((fwd << 2) & 0xFFu) | (u32)(q[4 + t] & 3);
				const u32 st = fwd < rc ? 0u : (rc < fwd ? 1u : 2u);
				if (st == state) {
					if (st == 2)
						++total;
					else
						++run;
				} else {
					state = st;
					total += 1 + run / (max_x + 1);
					run = 0;
				}
			}
			total += 1 + run / (max_x + 1);
		}
		atomicAdd(&s_px[b], total);
	}
	__syncthreads();
	for (u32 b = threadIdx.x; b < n_bins; b += 256)
		if (s_px[b])
			atomicAdd(&bin_plus_x[b], (u64)s_px[b]);
}

/* ------------------------------------------------------------------------------------------------ emit through a sort (alternative to k_s1_emit)
 * k_s1_emit claims output space with atomics: 512 partial-line write streams, ~2 records per bin and tile, 2.9 of the 6.1 ms of a 300 M symbol
 * part (profiles/r02/s1_bench_v3_*). The alternative orders the super-k-mers by bin first — k_s1_sort_keys makes 8-byte records
 * (index << 16) | bin, the EXISTING k_onesweep sorts them by their two low bytes (stable: a bin keeps read order, like the reference with one
 * splitter thread) — and k_s1_emit_sorted gives every record its final position from one exclusive scan of the record sizes in that order:
 *   position = bin_base[bin] + (bytes of all records before it in sorted order) - (bytes of all bins before its bin),
 * so consecutive threads write consecutive bytes. Tested under emulation and on the device (tests/test_gpu_stage1_parts.py: every bin byte for byte in read
 * order); not the default (S1PartParams::sorted_emit, $KMC_HIP_S1_SORTED_EMIT): to be measured first. */
__global__ void __launch_bounds__(256) k_s1_sort_keys(const u32 *__restrict__ sk_sig, u64 n_sk, const int *__restrict__ sig_to_bin, u32 n_bins, u64 *__restrict__ keys, u32 *err)
{
	const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
	if (i >= n_sk)
		return;
	const int b = sig_to_bin[sk_sig[i]];
	if (b < 0 || (u32)b >= n_bins) {
		atomicOr(err, KERR_CORRUPT);
		keys[i] = (i << 16) | 0xFFFFu;
	} else
		keys[i] = (i << 16) | (u64)b;
}

/* sorted: the keys in bin-major order; cum_bytes[b] = bytes of the records of all bins < b (no alignment). status: one zeroed u64 per tile. */
__global__ void __launch_bounds__(S1_BLOCK) k_s1_emit_sorted(const u64 *__restrict__ sorted, u64 n_sk, const int8_t *__restrict__ codes, const u64 *__restrict__ sk_pos,
                                                              const u32 *__restrict__ sk_len, u32 k, u32 n_bins, const u64 *__restrict__ bin_base,
                                                              const u64 *__restrict__ pack_base, const u64 *__restrict__ cum_bytes, u64 *status, u32 *ticket_ctr,
                                                              uint8_t *__restrict__ out, u64 *__restrict__ pack_start, u32 *err)
{
	__shared__ u32 s_tmp[S1_BLOCK / 64 + 1];
	__shared__ u64 s_carry;
	__shared__ u32 s_ticket;
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	if (tid == 0)
		s_ticket = atomicAdd(ticket_ctr, 1u);
	__syncthreads();
	const u32 tile = s_ticket;
	const u32 num_tiles = (u32)((n_sk + S1_TILE - 1) / S1_TILE);
	if (tile >= num_tiles)
		return;
	const u64 j0 = (u64)tile * S1_TILE + (u64)tid * S1_PER; /* this thread's S1_PER consecutive records of the sorted order */
	u64 idx[S1_PER];
	u32 bin[S1_PER], len[S1_PER], bytes[S1_PER], mine = 0;
#pragma unroll
	for (int t = 0; t < S1_PER; ++t) {
		bytes[t] = 0;
		if (j0 + t < n_sk) {
			const u64 key = sorted[j0 + t];
			idx[t] = key >> 16;
			bin[t] = (u32)(key & 0xFFFFu);
			if (bin[t] >= n_bins) { /* k_s1_sort_keys marked a signature without a bin (and raised the error) */
				atomicOr(err, KERR_CORRUPT);
				continue;
			}
			len[t] = sk_len[idx[t]];
			bytes[t] = 1u + (len[t] + 3u) / 4u;
			mine += bytes[t];
		}
	}
	u32 tile_bytes;
	const u32 before = block_excl_sum<S1_BLOCK / 64, u32>(mine, s_tmp, tile_bytes);
	if (wave == 0) {
		const u64 excl = lookback64(status, tile, (u64)tile_bytes, lane, err, KERR_WATCHDOG | KERR_AT_STAGE1);
		if (lane == 0)
			s_carry = excl;
	}
	__syncthreads();
	u64 g = s_carry + before; /* bytes of all records before this one in sorted order */
#pragma unroll
	for (int t = 0; t < S1_PER; ++t) {
		if (!bytes[t])
			continue;
		const u32 b = bin[t];
		const u64 rel = g - cum_bytes[b]; /* offset inside the bin's stream */
		g += bytes[t];
		const u64 m = (rel + S1_PACK_BYTES - 1) / S1_PACK_BYTES;
		if (m * S1_PACK_BYTES < rel + bytes[t]) /* the record that covers the m-th multiple of the pack size starts pack m */
			pack_start[pack_base[b] + m] = rel;
		uint8_t *dst = out + bin_base[b] + rel;
		const int8_t *src = codes + sk_pos[idx[t]];
		dst[0] = (uint8_t)(len[t] - k);
		u32 q = 0;
		for (; 4u * q + 8u <= len[t]; q += 2) {
			u64 w8;
			__builtin_memcpy(&w8, src + 4u * q, 8);
			const u32 lo = (u32)w8, hi = (u32)(w8 >> 32);
			dst[1 + q] = (uint8_t)(((lo & 3u) << 6) | (((lo >> 8) & 3u) << 4) | (((lo >> 16) & 3u) << 2) | ((lo >> 24) & 3u));
			dst[2 + q] = (uint8_t)(((hi & 3u) << 6) | (((hi >> 8) & 3u) << 4) | (((hi >> 16) & 3u) << 2) | ((hi >> 24) & 3u));
		}
		for (; q < (len[t] + 3u) / 4u; ++q) {
			u32 v = 0;
#pragma unroll
			for (u32 u = 0; u < 4; ++u) {
				const u32 p = 4 * q + u;
				v = (v << 2) | (p < len[t] ? (u32)(src[p] & 3) : 0u);
			}
			dst[1 + q] = (uint8_t)v;
		}
	}
}

#endif
