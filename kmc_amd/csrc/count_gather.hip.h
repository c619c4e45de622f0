/* kmc_amd/csrc/count_gather.hip.h — k_cnt_gather: the segmented copy of the counting session (host_count.hip.h; gfx950, wave64).
 *
 * What it replaces: CKmerBinStorer writing every collector's buffer behind its bin's file (kb_storer.cpp) and CKmerBinReader reading each file back as one bin image
 * (kb_reader.h:176-190). Here the parts' bin records stay in HBM, part-major as stage 1 left them, and this kernel moves every (part, bin) segment to its place in
 * the bin-major images stage 2 reads: every byte of bin records is read once and written once.
 *
 * table: n_segments x {source offset, destination offset, bytes} (u64), offsets from src_base / dst_base (the session passes 0 / 0 and addresses). Segments lie at
 * arbitrary byte offsets on both sides. A workgroup takes segments seg = blockIdx.x, + gridDim.x, ... (a persistent grid with a grid-stride loop: tiny and huge tables
 * use the same launch) and copies a segment with all its threads:
 *   head: the bytes in front of the destination's first 16-byte boundary, byte by byte;
 *   body: 16-byte pieces, stores aligned to the destination, consecutive lanes on consecutive pieces (1 KiB per wave instruction);
 *   tail: what is left behind the last whole piece, byte by byte.
 * Loads are aligned to the source as well. Where the two alignments differ by sh bytes a piece is the 32 bytes of the two aligned source blocks it lies in, SHIFTED
 * IN REGISTERS (four 64-bit shifts and two ors; sh is uniform over the segment, so the branch is too). Why registers and not LDS (as k_tr_dump<true> stages its text):
 * the copy has no reuse to keep — every byte is wanted by exactly one lane — so LDS would add a write, a barrier and a read per piece and cap the workgroups per CU,
 * while the second aligned load of a piece is the first one of the neighbouring lane: the same cache line in the same instruction, served once.
 * The first shifted piece's low block would begin in front of the segment when the head is shorter than sh: that piece then goes with the head (31 bytes at most).
 * Bounds: no byte outside [dst, dst + bytes) is written; no byte outside [src, src + bytes + 16) is read (the last piece's high block ends 16 - sh bytes behind the
 * last whole piece). No LDS, no barrier, no atomics, no communication between workgroups: nothing can wait. */
#ifndef KMC_COUNT_GATHER_HIP_H
#define KMC_COUNT_GATHER_HIP_H

constexpr int CG_THREADS = 256;
constexpr u32 CG_MAX_WGS = 2048;       /* the persistent grid: 256 CUs x 8 workgroups of 4 waves */
constexpr u64 CG_PIECE_BYTES = 1 << 18; /* the host cuts longer segments into table entries of this size, so that few long segments (few bins) still spread over the grid */

__device__ __forceinline__ ulonglong2 cg_shifted(const ulonglong2 lo, const ulonglong2 hi, u32 sh /* 1..15 bytes */)
{
	u64 w0 = lo.x, w1 = lo.y, w2 = hi.x;
	if (sh >= 8) {
		w0 = w1, w1 = w2, w2 = hi.y;
		sh -= 8;
	}
	if (!sh)
		return make_ulonglong2(w0, w1);
	const u32 b = 8 * sh;
	return make_ulonglong2((w0 >> b) | (w1 << (64 - b)), (w1 >> b) | (w2 << (64 - b)));
}

__global__ void __launch_bounds__(CG_THREADS) k_cnt_gather(const uint8_t *src_base, uint8_t *dst_base, const u64 *__restrict__ table, u64 n_segments)
{
	const u32 t = threadIdx.x;
	for (u64 seg = blockIdx.x; seg < n_segments; seg += gridDim.x) {
		const uint8_t *s = reinterpret_cast<const uint8_t *>(reinterpret_cast<u64>(src_base) + table[3 * seg]);
		uint8_t *d = reinterpret_cast<uint8_t *>(reinterpret_cast<u64>(dst_base) + table[3 * seg + 1]);
		const u64 len = table[3 * seg + 2];
		if (!len)
			continue;
		u64 head = (16 - (reinterpret_cast<u64>(d) & 15)) & 15;
		if (head > len)
			head = len;
		const u32 sh = (u32)((reinterpret_cast<u64>(s) + head) & 15);
		if (sh && head < sh && len - head >= 16)
			head += 16; /* the low block of the first shifted piece begins in front of the segment */
		const u64 n_vec = (len - head) >> 4;
		const u64 tail_at = head + (n_vec << 4);
		/* head (at most 31 bytes: lanes 0..30) and tail (at most 15: lanes 32..46), one byte per lane */
		if (t < head)
			d[t] = s[t];
		else if (t >= 32 && tail_at + (t - 32) < len)
			d[tail_at + (t - 32)] = s[tail_at + (t - 32)];
		ulonglong2 *dv = reinterpret_cast<ulonglong2 *>(d + head);
		if (!sh) {
			const ulonglong2 *sv = reinterpret_cast<const ulonglong2 *>(s + head);
#pragma unroll 4
			for (u64 i = t; i < n_vec; i += CG_THREADS)
				dv[i] = sv[i];
		} else {
			const ulonglong2 *sv = reinterpret_cast<const ulonglong2 *>(s + head - sh);
#pragma unroll 4
			for (u64 i = t; i < n_vec; i += CG_THREADS)
				dv[i] = cg_shifted(sv[i], sv[i + 1], sh);
		}
	}
}

#endif /* KMC_COUNT_GATHER_HIP_H */
