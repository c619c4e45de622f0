/* kmc_amd/csrc/bgzf.hip.h — part of kmc_hip.hip: BGZF members inflated on the device (what CFastqReader does member by member with zlib and a CRC check on one host
 * thread, kmc_core/fastq_reader.cpp:72-189). A BGZF file is a sequence of independent gzip members of at most 64 KiB of output each; the host walks their headers
 * (kmc_hip_bgzf_scan, host_bgzf.hip.h) and k_bgzf_inflate takes ONE MEMBER PER WAVE (one 64-thread workgroup).
 *
 * The decode loop is wave-uniform: every lane holds the same bit buffer and the same positions and takes the same branch, so there is no divergence and nothing to
 * communicate. What has width is done by the 64 lanes: the compressed bytes arrive as one dword per lane (256 bytes a load, the next 256 already in flight), literals are
 * collected one per lane and stored 64 at a time, a match is copied by all lanes (source index modulo the distance where distance < length: distance 1 is a run), the
 * decode tables are built by the wave (lengths counted with LDS atomics, codes ranked with ballots), the CRC is taken over 64 slices and combined by the x^n mod P shift,
 * and the output leaves as aligned 16-byte pieces.
 *
 * LDS of a workgroup (about 69 KiB: two workgroups per CU):
 *   s_win   64 KiB + 16  the member's whole output, at the residue modulo 16 that its place in the output buffer has; matches read it, never global memory
 *   s_ring  512 B        two 256-byte pieces of the compressed bytes
 *   s_lit / s_dist / s_cl  first-level tables of 10 / 8 / 7 bits: entry = symbol << 4 | code length, 0 = no code of at most that many bits starts like this
 *   s_cnt*, s_sym*       codes per length and the symbols in code order: longer codes are walked a bit at a time (canonical order), as are invalid ones to their end
 *   s_lens, s_cll        the code lengths of the block being set up
 * No table is a register array indexed at run time. No workgroup waits for another one.
 *
 * Fail closed: compressed bytes behind comp_len read as zero and the bits used are checked against comp_len after every symbol (every turn of every loop uses at least
 * one bit or ends the member, so a member ends after at most 8 x comp_len + 64 bits); every store into s_win is preceded by a check against isize <= 65536; table
 * indices are masked bit fields. The verdict on a member is zlib's: what inflate() rejects is an error here. */
#ifndef KMC_BGZF_HIP_H
#define KMC_BGZF_HIP_H

constexpr u32 BGZF_MAX_OUT = 65536;
constexpr u32 BGZF_LIT_BITS = 10, BGZF_DIST_BITS = 8, BGZF_CL_BITS = 7;
/* a member's error word; the host's messages are in host_bgzf.hip.h (bgzf_reason) */
constexpr u32 BGZF_E_BTYPE = 1;    /* block type 3 */
constexpr u32 BGZF_E_STORED = 2;   /* a stored block's LEN is not the complement of NLEN, or runs past the member */
constexpr u32 BGZF_E_CODESET = 3;  /* an over-subscribed set of code lengths, or an incomplete one that is not a single code of length 1 */
constexpr u32 BGZF_E_NO_EOB = 4;   /* no code for symbol 256 */
constexpr u32 BGZF_E_REPEAT = 5;   /* a repeat code with nothing before it, or one that runs past the lengths */
constexpr u32 BGZF_E_SYMBOL = 6;   /* bits that are no code; literal/length symbol 286 or 287; distance symbol 30 or 31; more than 286 / 30 codes announced */
constexpr u32 BGZF_E_DISTANCE = 7; /* a distance that reaches in front of the member's output */
constexpr u32 BGZF_E_OUT_SHORT = 8;
constexpr u32 BGZF_E_OUT_LONG = 9;
constexpr u32 BGZF_E_IN_LEFT = 10;
constexpr u32 BGZF_E_IN_SHORT = 11;
constexpr u32 BGZF_E_CRC = 12;
constexpr u32 BGZF_E_TABLE = 13;   /* a member table entry no BGZF member can have (isize above 64 KiB) */

struct BgzfMember { /* == kmc_hip_bgzf_member */
	u64 src_off, dst_off;
	u32 comp_len, isize, crc, reserved;
};

/* the compressed bytes of one member, read by the whole wave; every field is the same in all lanes but `pre` */
struct BgzfIn {
	const uint8_t *src;
	u32 comp_len;
	u32 base;    /* byte of the member that dword 0 of the ring stream starts at */
	u32 fetched; /* dwords taken into buf since base */
	u32 nchunk;  /* 256-byte pieces put into the ring since base */
	u32 pre;     /* this lane's dword of piece nchunk, loaded ahead */
	u64 buf;
	u32 cnt;
};

__device__ __forceinline__ void bgzf_load_ahead(BgzfIn &in, u32 lane)
{
	const u32 off = in.base + (in.nchunk * 64 + lane) * 4;
	u32 v = 0;
	if (off < in.comp_len) {
		if (in.comp_len - off >= 4)
			__builtin_memcpy(&v, in.src + off, 4);
		else
			for (u32 b = 0; b < in.comp_len - off; ++b)
				v |= (u32)in.src[off + b] << (8 * b);
	}
	in.pre = v;
}
__device__ __forceinline__ void bgzf_in_reset(BgzfIn &in, u32 pos, u32 lane)
{
	in.base = pos;
	in.fetched = 0;
	in.nchunk = 0;
	in.buf = 0;
	in.cnt = 0;
	bgzf_load_ahead(in, lane);
}
/* at least 32 bits in buf (zeros behind the member's end) */
__device__ __forceinline__ void bgzf_refill(BgzfIn &in, u32 *ring, u32 lane)
{
	if (in.cnt >= 32)
		return;
	if ((in.fetched >> 6) == in.nchunk) {
		__syncthreads(); /* the piece this one replaces has been read by every lane */
		ring[(in.nchunk & 1) * 64 + lane] = in.pre;
		__syncthreads();
		++in.nchunk;
		bgzf_load_ahead(in, lane);
	}
	in.buf |= (u64)ring[in.fetched & 127] << in.cnt;
	in.cnt += 32;
	++in.fetched;
}
__device__ __forceinline__ u32 bgzf_bits(BgzfIn &in, u32 n) /* n <= 16, cnt >= n */
{
	const u32 v = (u32)in.buf & ((1u << n) - 1);
	in.buf >>= n;
	in.cnt -= n;
	return v;
}
__device__ __forceinline__ u32 bgzf_used_bits(const BgzfIn &in) { return (in.base + 4 * in.fetched) * 8 - in.cnt; }
__device__ __forceinline__ bool bgzf_in_over(const BgzfIn &in) { return bgzf_used_bits(in) > in.comp_len * 8; }

__device__ __forceinline__ u32 bgzf_rev(u32 code, u32 len) /* the low `len` bits of code, first bit of the stream lowest */
{
	code = ((code & 0x5555u) << 1) | ((code >> 1) & 0x5555u);
	code = ((code & 0x3333u) << 2) | ((code >> 2) & 0x3333u);
	code = ((code & 0x0F0Fu) << 4) | ((code >> 4) & 0x0F0Fu);
	code = ((code & 0x00FFu) << 8) | ((code >> 8) & 0x00FFu);
	return code >> (16 - len);
}

/* The canonical code of lens[0 .. n) (0 = symbol unused), built by the wave: fast[] (1 << FAST entries), cnt[1 .. 15] codes per length, sym[] the symbols in code
 * order. `codes`: the code-length alphabet, which must be complete. Returns 0 or BGZF_E_CODESET — inflate_table's rules: no code at all is accepted here and fails at
 * the first symbol; an incomplete set only as one code of length 1. */
template <u32 FAST> __device__ u32 bgzf_build(const uint8_t *lens, u32 n, uint16_t *fast, u32 *cnt, uint16_t *sym, u32 lane, bool codes)
{
	__syncthreads(); /* nobody decodes with the tables any more; lens[] is written */
	for (u32 i = lane; i < (1u << FAST); i += 64)
		fast[i] = 0;
	if (lane < 16)
		cnt[lane] = 0;
	__syncthreads();
	for (u32 s = lane; s < n; s += 64)
		atomicAdd(&cnt[lens[s] & 15], 1u);
	__syncthreads();
	u32 c[16], next[16], offs[16], run[16];
	int left = 1;
	u32 maxlen = 0;
	bool over = false;
#pragma unroll
	for (u32 l = 1; l < 16; ++l) {
		c[l] = cnt[l];
		left = (left << 1) - (int)c[l];
		over = over || left < 0;
		if (c[l])
			maxlen = l;
	}
	if (over)
		return BGZF_E_CODESET;
	if (maxlen && left > 0 && (codes || maxlen != 1))
		return BGZF_E_CODESET;
	u32 code = 0, off = 0;
	c[0] = 0;
#pragma unroll
	for (u32 l = 1; l < 16; ++l) {
		code = (code + c[l - 1]) << 1;
		next[l] = code;
		offs[l] = off;
		off += c[l];
		run[l] = 0;
	}
	const u64 below = lane ? (~0ull >> (64 - lane)) : 0ull;
	for (u32 s0 = 0; s0 < n; s0 += 64) {
		const u32 s = s0 + lane, L = s < n ? (lens[s] & 15u) : 0u;
#pragma unroll
		for (u32 l = 1; l < 16; ++l) {
			if (!c[l])
				continue;
			const u64 m = __ballot(L == l);
			if (L == l) {
				const u32 k = run[l] + (u32)__popcll(m & below);
				sym[offs[l] + k] = (uint16_t)s;
				if (l <= FAST) {
					const uint16_t e = (uint16_t)((s << 4) | l);
					for (u32 j = bgzf_rev(next[l] + k, l); j < (1u << FAST); j += 1u << l)
						fast[j] = e;
				}
			}
			run[l] += (u32)__popcll(m);
		}
	}
	__syncthreads();
	return 0;
}

/* the symbol the bits of buf start with: symbol << 4 | length, or 0 where they are no code. The first level answers codes of at most FAST bits; the rest walks the
 * canonical order one bit at a time. */
template <u32 FAST> __device__ __forceinline__ u32 bgzf_symbol(u64 buf, const uint16_t *fast, const u32 *cnt, const uint16_t *sym)
{
	const u32 e = fast[(u32)buf & ((1u << FAST) - 1)];
	if (e)
		return e;
	int code = 0, first = 0, index = 0;
	for (u32 len = 1; len < 16; ++len) {
		code |= (int)((buf >> (len - 1)) & 1);
		const int count = (int)cnt[len];
		if (code - count < first)
			return len > FAST ? ((u32)sym[index + (code - first)] << 4) | len : 0u;
		index += count;
		first = (first + count) << 1;
		code <<= 1;
	}
	return 0;
}

/* a x b mod P on the reflected CRC-32 polynomial (bit 31 is x^0), and x^n mod P: how the CRCs of slices combine (zlib's crc32_combine does the same on the host) */
__device__ __forceinline__ u32 bgzf_mulmod(u32 a, u32 b)
{
	u32 p = 0;
	for (u32 i = 0; i < 32; ++i) {
		p ^= b & (0u - ((a >> (31 - i)) & 1u));
		b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
	}
	return p;
}
__device__ __forceinline__ u32 bgzf_xpow(u32 n)
{
	u32 r = 0x80000000u, sq = 0x40000000u;
	for (; n; n >>= 1) {
		if (n & 1)
			r = bgzf_mulmod(r, sq);
		sq = bgzf_mulmod(sq, sq);
	}
	return r;
}
__device__ __forceinline__ u32 bgzf_crc_byte(u32 crc, u32 byte)
{
	crc ^= byte;
#pragma unroll
	for (int b = 0; b < 8; ++b)
		crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
	return crc;
}

__global__ void __launch_bounds__(64) k_bgzf_inflate(const BgzfMember *__restrict__ members, u32 n_members, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                     u32 *__restrict__ err_of /* [n_members] */, u32 *__restrict__ first_bad)
{
	__shared__ __attribute__((aligned(16))) uint8_t s_win[BGZF_MAX_OUT + 16];
	__shared__ u32 s_ring[128];
	__shared__ uint16_t s_lit[1u << BGZF_LIT_BITS], s_dist[1u << BGZF_DIST_BITS], s_cl[1u << BGZF_CL_BITS];
	__shared__ u32 s_cnt_lit[16], s_cnt_dist[16], s_cnt_cl[16];
	__shared__ uint16_t s_sym_lit[288], s_sym_dist[32], s_sym_cl[32];
	__shared__ uint8_t s_lens[320], s_cll[32];

	const u32 mi = blockIdx.x, lane = threadIdx.x;
	if (mi >= n_members)
		return;
	const BgzfMember mem = members[mi];
	const u32 isize = mem.isize;
	uint8_t *const out = dst + mem.dst_off;
	const u32 mis = (u32)((size_t)out & 15);
	uint8_t *const win = s_win + mis;
	u32 err = isize > BGZF_MAX_OUT ? BGZF_E_TABLE : 0;

	BgzfIn in;
	in.src = src + mem.src_off;
	in.comp_len = mem.comp_len;
	bgzf_in_reset(in, 0, lane);
	u32 opos = 0, pend = 0, mylit = 0, last = 0;

	while (!err && !last) {
		bgzf_refill(in, s_ring, lane);
		last = bgzf_bits(in, 1);
		const u32 btype = bgzf_bits(in, 2);
		if (bgzf_in_over(in)) {
			err = BGZF_E_IN_SHORT;
			break;
		}
		if (btype == 3) {
			err = BGZF_E_BTYPE;
			break;
		}
		if (btype == 0) {
			bgzf_bits(in, in.cnt & 7); /* to the byte boundary (base and the dwords are whole bytes) */
			bgzf_refill(in, s_ring, lane);
			const u32 len = bgzf_bits(in, 16), nlen = bgzf_bits(in, 16);
			const u32 pos = bgzf_used_bits(in) / 8;
			if (pos > in.comp_len) { /* LEN and NLEN themselves lie behind the member's end */
				err = BGZF_E_IN_SHORT;
				break;
			}
			if ((len ^ nlen) != 0xFFFFu || len > in.comp_len - pos) {
				err = BGZF_E_STORED;
				break;
			}
			if (len > isize - opos) {
				err = BGZF_E_OUT_LONG;
				break;
			}
			for (u32 i = lane; i < len; i += 64)
				win[opos + i] = in.src[pos + i];
			opos += len;
			bgzf_in_reset(in, pos + len, lane);
			continue;
		}
		/* ---- the block's two codes */
		u32 n_lit = 288, n_dist = 32;
		if (btype == 1) {
			__syncthreads();
			for (u32 i = lane; i < 320; i += 64)
				s_lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
		} else {
			n_lit = bgzf_bits(in, 5) + 257;
			n_dist = bgzf_bits(in, 5) + 1;
			const u32 n_cl = bgzf_bits(in, 4) + 4;
			if (n_lit > 286 || n_dist > 30) {
				err = BGZF_E_SYMBOL;
				break;
			}
			__syncthreads();
			if (lane < 32)
				s_cll[lane] = 0;
			__syncthreads();
			/* the order of the code-length code's lengths, 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each */
			const u64 order_lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
			const u64 order_hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
			for (u32 i = 0; i < n_cl; ++i) {
				bgzf_refill(in, s_ring, lane);
				const u32 v = bgzf_bits(in, 3), at = (u32)((i < 12 ? order_lo >> (5 * i) : order_hi >> (5 * (i - 12))) & 31);
				if (lane == 0)
					s_cll[at] = (uint8_t)v;
			}
			if (bgzf_in_over(in)) {
				err = BGZF_E_IN_SHORT;
				break;
			}
			if ((err = bgzf_build<BGZF_CL_BITS>(s_cll, 19, s_cl, s_cnt_cl, s_sym_cl, lane, true)))
				break;
			const u32 total = n_lit + n_dist;
			u32 i = 0, prev = 0;
			bool eob = false;
			while (i < total) {
				bgzf_refill(in, s_ring, lane);
				const u32 e = bgzf_symbol<BGZF_CL_BITS>(in.buf, s_cl, s_cnt_cl, s_sym_cl);
				if (!e) {
					err = BGZF_E_SYMBOL;
					break;
				}
				bgzf_bits(in, e & 15);
				const u32 s = e >> 4;
				u32 val = s, rep = 1;
				if (s == 16) {
					if (i == 0) {
						err = BGZF_E_REPEAT;
						break;
					}
					val = prev;
					rep = 3 + bgzf_bits(in, 2);
				} else if (s == 17) {
					val = 0;
					rep = 3 + bgzf_bits(in, 3);
				} else if (s == 18) {
					val = 0;
					rep = 11 + bgzf_bits(in, 7);
				}
				if (rep > total - i) {
					err = BGZF_E_REPEAT;
					break;
				}
				if (bgzf_in_over(in)) {
					err = BGZF_E_IN_SHORT;
					break;
				}
				for (u32 j = lane; j < rep; j += 64)
					s_lens[i + j] = (uint8_t)val;
				eob = eob || (val && i <= 256 && 256 < i + rep);
				prev = val;
				i += rep;
			}
			if (err)
				break;
			if (!eob) {
				err = BGZF_E_NO_EOB;
				break;
			}
		}
		if ((err = bgzf_build<BGZF_LIT_BITS>(s_lens, n_lit, s_lit, s_cnt_lit, s_sym_lit, lane, false)))
			break;
		if ((err = bgzf_build<BGZF_DIST_BITS>(s_lens + n_lit, n_dist, s_dist, s_cnt_dist, s_sym_dist, lane, false)))
			break;
		/* ---- the block's symbols */
		for (;;) {
			bgzf_refill(in, s_ring, lane);
			const u32 e = bgzf_symbol<BGZF_LIT_BITS>(in.buf, s_lit, s_cnt_lit, s_sym_lit);
			if (!e) {
				err = BGZF_E_SYMBOL;
				break;
			}
			bgzf_bits(in, e & 15);
			if (bgzf_in_over(in)) {
				err = BGZF_E_IN_SHORT;
				break;
			}
			const u32 s = e >> 4;
			if (s < 256) {
				if (opos >= isize) {
					err = BGZF_E_OUT_LONG;
					break;
				}
				mylit = lane == pend ? s : mylit;
				++pend;
				++opos;
				if (pend == 64) {
					win[opos - 64 + lane] = (uint8_t)mylit;
					pend = 0;
				}
			} else if (s == 256) {
				break;
			} else {
				if (s > 285) {
					err = BGZF_E_SYMBOL;
					break;
				}
				const u32 lx = s < 265 || s == 285 ? 0u : (s - 261) >> 2;
				const u32 len = (s < 265 ? s - 254 : s == 285 ? 258u : 3 + ((4 + ((s - 261) & 3)) << lx)) + bgzf_bits(in, lx);
				bgzf_refill(in, s_ring, lane);
				const u32 d = bgzf_symbol<BGZF_DIST_BITS>(in.buf, s_dist, s_cnt_dist, s_sym_dist);
				if (!d || (d >> 4) > 29) {
					err = BGZF_E_SYMBOL;
					break;
				}
				bgzf_bits(in, d & 15);
				const u32 ds = d >> 4, dx = ds < 4 ? 0u : (ds >> 1) - 1;
				const u32 dist = (ds < 4 ? ds + 1 : 1 + ((2 + (ds & 1)) << dx)) + bgzf_bits(in, dx);
				if (bgzf_in_over(in)) {
					err = BGZF_E_IN_SHORT;
					break;
				}
				if (dist > opos) {
					err = BGZF_E_DISTANCE;
					break;
				}
				if (len > isize - opos) {
					err = BGZF_E_OUT_LONG;
					break;
				}
				if (lane < pend)
					win[opos - pend + lane] = (uint8_t)mylit;
				pend = 0;
				__syncthreads(); /* what the match reads has been written, by whichever lane */
				const uint8_t *from = win + (opos - dist);
				if (dist >= len) {
					for (u32 i = lane; i < len; i += 64)
						win[opos + i] = from[i];
				} else {
					/* the source repeats with period dist; i mod dist by a multiplication: m = floor(2^22 / dist) + 1 is exact for i < 2^22 / dist, and i < 258 + 64, dist < 258 */
					const u32 m = (1u << 22) / dist + 1;
					for (u32 i = lane; i < len; i += 64)
						win[opos + i] = from[i - ((i * m) >> 22) * dist];
				}
				opos += len;
			}
		}
		if (lane < pend && !err)
			win[opos - pend + lane] = (uint8_t)mylit;
		pend = 0;
	}
	if (!err) {
		const u32 used = (bgzf_used_bits(in) + 7) / 8;
		if (opos != isize)
			err = BGZF_E_OUT_SHORT;
		else if (used > in.comp_len)
			err = BGZF_E_IN_SHORT;
		else if (used < in.comp_len)
			err = BGZF_E_IN_LEFT;
	}
	__syncthreads();
	if (!err && isize) {
		/* CRC-32 of win[0 .. isize): the aligned dwords of s_win that hold it in 64 slices, one per lane; slice i's register, started from 0 (from ~0 for the slice with
		 * the first byte), times x^(8 x bytes behind the slice), all XORed */
		const u32 end = mis + isize, per = ((end + 3) / 4 + 63) / 64 * 4;
		const u32 lo = lane * per < mis ? mis : lane * per, hi = (lane + 1) * per < end ? (lane + 1) * per : end;
		u32 crc = 0;
		if (lo < hi) {
			crc = lo == mis ? 0xFFFFFFFFu : 0u;
			u32 p = lo;
			for (; p < hi && (p & 3); ++p)
				crc = bgzf_crc_byte(crc, s_win[p]);
			for (; p + 4 <= hi; p += 4) {
				crc ^= *reinterpret_cast<const u32 *>(s_win + p);
#pragma unroll 8
				for (int b = 0; b < 32; ++b)
					crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
			}
			for (; p < hi; ++p)
				crc = bgzf_crc_byte(crc, s_win[p]);
			crc = bgzf_mulmod(crc, bgzf_xpow((end - hi) * 8));
		}
		for (u32 o = 32; o; o >>= 1)
			crc ^= __shfl_down(crc, o);
		crc = (u32)__shfl((int)crc, 0) ^ 0xFFFFFFFFu;
		if (crc != mem.crc)
			err = BGZF_E_CRC;
	} else if (!err && mem.crc != 0)
		err = BGZF_E_CRC;
	if (err) {
		if (lane == 0) {
			err_of[mi] = err;
			atomicMin(first_bad, mi);
		}
		return;
	}
	/* out and win have the same residue modulo 16: the edges byte by byte, the rest as whole aligned pieces; nothing outside out[0 .. isize) is written */
	const u32 head = isize < ((16u - mis) & 15u) ? isize : ((16u - mis) & 15u), n_vec = (isize - head) / 16, tail0 = head + n_vec * 16;
	for (u32 i = lane; i < head; i += 64)
		out[i] = win[i];
	const TrVec16 *w16 = reinterpret_cast<const TrVec16 *>(win + head);
	TrVec16 *o16 = reinterpret_cast<TrVec16 *>(out + head);
	for (u32 i = lane; i < n_vec; i += 64)
		o16[i] = w16[i];
	for (u32 i = tail0 + lane; i < isize; i += 64)
		out[i] = win[i];
}

#endif
