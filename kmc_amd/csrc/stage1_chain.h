/*
 * kmc_amd/csrc/stage1_chain.h — one part of input text through the stage-1 kernels, written ONCE for two backends:
 *   - HipBackend (kmc_hip.hip, kmc_hip_split_part): hipMalloc / hipLaunchKernelGGL / hipMemcpy on a stream
 *   - EmuBackend (tests/hipemu/emu_split_engine.cpp): host memory and the CPU emulation of the kernels
 * so that the order of launches, the grid and buffer sizes, the synchronisation points, the retry of the cutting kernel and the assembly of
 * the result are exercised inside the real KMC pipeline on the CPU (oracle/_ref/kmc_emu_s1, tests/test_stage1_plugin.py) before a GPU sees
 * them. Does for one part what CSplitter::ProcessReads + the n_bins CKmerBinCollectors do (splitter.cpp:557-672, kb_collector.cpp:34-106),
 * up to the bin-part buffers.
 *
 * A backend B provides:
 *   void *alloc(size_t bytes)                  zeroed device memory, owned by the backend until release()
 *   void *alloc_uninit(size_t bytes)           the same without the zeroing: for arrays that are written before they are read (super-k-mer lists, sort keys)
 *   void  zero(void *p, size_t bytes)          (stream-ordered)
 *   bool  d2h(void *dst, const void *src, size_t bytes)   copies and waits for everything launched before; false = device failure
 *   void  h2d(void *dst, const void *src, size_t bytes)   (the source may be reused when it returns)
 *   S1_LAUNCH(B, be, kernel, grid, block, args...)         launch `kernel` (a macro per backend: the emulator calls kernels as functions)
 *   u64  *sort_by_low16(u64 *keys, u64 *tmp, u64 n)         stable sort of 8-byte records by their two low bytes; returns where the result is
 *                                                           (the HIP backend runs the library's own radix passes, test backends sort on the host)
 */
#ifndef KMC_AMD_STAGE1_CHAIN_H
#define KMC_AMD_STAGE1_CHAIN_H

#include <vector>

#include "stage1_kernels.hip.h"

struct S1PartParams {
	u32 k, m, n_bins, max_x, both_strands, lines_per_record; /* lines_per_record: 2 = FASTA, 4 = FASTQ, 0 = the symbols of a long-read part (the caller
	                                                           * has taken the title off: d_text starts at its end of line, GetSeqLongRead splitter.cpp:70-86) */
	u64 line_cap;                                             /* mem_part_pmm_reads */
	const int *d_sig_to_bin;                                  /* device: 4^m + 1 entries */
	u64 sk_guess_div = 8;                                     /* first guess of the number of super-k-mers: symbols / this + 4096 */
	bool sorted_emit = false;                                 /* records through a sort by bin (k_s1_emit_sorted) instead of k_s1_emit: bins in read order */
	bool multiline_fasta = false;                             /* a multi-line FASTA part (ReadType::na, GetSeq splitter.cpp:304-323): k_s1_ml_text_to_codes;
	                                                           * lines_per_record is not used */
	bool bam = false;                                         /* a part of BAM alignment records (ReadType::na, GetSeq splitter.cpp:326-419): k_s1_bam_chain + k_s1_bam_decode;
	                                                           * lines_per_record is not used, no piece marks are made */
	bool homopolymer = false;                               /* -hc: every return of GetSeq — a line, or one PIECE of an over-long line / a long-read part — is
	                                                           * homopolymer-compressed on its own (splitter.cpp:424-435, :575-581): k_s1_hc_compact in front of the cut */
};
struct S1PartResult {
	const uint8_t *d_recs = nullptr; /* device: bin b's records at d_recs + bin_off[b], bin_bytes[b] of them */
	u64 recs_bytes = 0;
	std::vector<u64> bin_off, bin_bytes, bin_sk, bin_kmers, bin_plus_x;
	u64 n_reads = 0, n_symbols = 0, n_superkmers = 0;
	u32 device_error = 0;
	const int8_t *d_raw_codes = nullptr; /* device: the code stream as text -> codes (+ marks) left it, n_raw codes. With -hc the chain cuts another, compacted
	                                      * stream; this one stays allocated and unchanged: s1_estimate_part hashes it */
	u64 n_raw = 0;
};
enum { S1_CHAIN_OK = 0, S1_CHAIN_UNCOVERED = 1, S1_CHAIN_DEVICE_ERROR = -1, S1_CHAIN_BACKEND_FAILURE = -2 };

/* A long-read part (ReadType::long_read, queues.h:40; CSplitter::GetSeqLongRead, splitter.cpp:70-86): if it starts with the format's marker it carries the
 * read's title — one read counted, and the symbols start AT the title's end of line (that byte is a symbol like every other: an invalid one). Returns the
 * number of bytes to take off the front; the rest goes through s1_split_part with lines_per_record = 0. */
static inline u64 s1_long_read_title(const uint8_t *text, u64 size, u32 file_type /* 0 FASTA, 1 FASTQ */, u64 &n_reads)
{
	n_reads = 0;
	if (!size || text[0] != (file_type == 1 ? '@' : '>'))
		return 0;
	n_reads = 1;
	u64 p = 0;
	while (p < size && text[p] != '\n' && text[p] != '\r')
		++p;
	return p;
}

/* What the front half of the chain leaves behind for whoever goes on with the codes: the stream that is cut / counted (the -hc stream with -hc), the small
 * block and the words in it. R.d_raw_codes / n_raw, n_reads and n_symbols are set as well. */
struct S1Front {
	u64 *d_small = nullptr, *d_has_marks = nullptr;
	u32 *d_ticket = nullptr, *d_err = nullptr;
	const u64 *d_cut_marks = nullptr; /* nullptr: no code of d_codes carries S1_PIECE_MARK (the -hc stream: pieces are sequences of their own) */
	int8_t *d_codes = nullptr;
	u64 n = 0;
};

/* The part's error word (the high half of word `at` of what was read) against `uncovered`, the bits that mean "malformed in a way the kernels do not cover": such
 * a bit gives S1_CHAIN_UNCOVERED, any other one R.device_error and S1_CHAIN_DEVICE_ERROR. */
static inline int s1_classify(u32 err, u32 uncovered, S1PartResult &R)
{
	if (err & uncovered)
		return S1_CHAIN_UNCOVERED;
	if (err) {
		R.device_error = err;
		return S1_CHAIN_DEVICE_ERROR;
	}
	return S1_CHAIN_OK;
}
/* Reads N words from d_src (be.d2h: waits for everything launched before) and classifies the error word among them. */
template <class B, size_t N> int s1_read_errors(B &be, u64 (&dst)[N], const u64 *d_src, size_t at, u32 uncovered, S1PartResult &R)
{
	static_assert(N >= 1, "");
	if (!be.d2h(dst, d_src, sizeof dst))
		return S1_CHAIN_BACKEND_FAILURE;
	return s1_classify((u32)(dst[at] >> 32), uncovered, R);
}

/* The front half: text / BAM records / multi-line FASTA -> codes, piece marks, the record check, the -hc compaction, n_reads and n_symbols; the part's error
 * words -> S1_CHAIN_UNCOVERED. Uses of P: k, both_strands, lines_per_record, line_cap and the format switches, nothing of the bin path (m, n_bins, max_x, the map).
 * wait_for_errors: without -hc the record check runs beside whatever the caller launches next and its error word is read with that (the bin path: beside the
 * cut); a caller with nothing to launch that may fail (s1_smallk_part) waits for it here, so that S1_CHAIN_OK means the codes are those of a covered part. */
template <class B> int s1_front_part(B &be, const uint8_t *d_text, u64 size, bool text_ends_with_newline, const S1PartParams &P, S1PartResult &R, S1Front &F, bool wait_for_errors)
{
	const u32 lpr = P.lines_per_record;
	R = S1PartResult();
	F = S1Front();
	if (!size)
		return S1_CHAIN_OK;
	/* small block: [0] '\\n' count | [1] code bytes | [2] super-k-mers | [3] lo: ticket, hi: error word | [4] != 0: some code carries S1_PIECE_MARK |
	 * [5] code bytes after k_s1_hc_compact */
	u64 *d_small = (u64 *)be.alloc(64);
	u32 *d_ticket = (u32 *)(d_small + 3), *d_err = d_ticket + 1;
	u64 *d_has_marks = d_small + 4;
	u64 small[4];
	/* pieces of an over-long line start every `stride` symbols (S1_PIECE_MARK); k_s1_cut takes at most one mark per workgroup window */
	if (P.line_cap < (u64)P.k + S1_WG_TILE + 2)
		return S1_CHAIN_UNCOVERED;
	const u64 stride = P.line_cap - P.k + 1;
	u64 n;
	int8_t *d_codes;
	if (P.bam) {
		/* ---- BAM records -> codes: the record starts (one chain from offset 0 to the part's end), then the bases. No piece marks: a record of line_cap bases
		 * or more is not taken */
		if (size >= S1_BAM_MAX_PART)
			return S1_CHAIN_UNCOVERED; /* record offsets are 32-bit words; kmc_hip_split_part refuses such a call by name */
		const u32 tiles = (u32)((size + S1_BAM_TILE - 1) / S1_BAM_TILE);
		const u64 rec_cap = size / S1_BAM_MIN_HOP + 1, out_cap = 2 * size + 16;
		u32 *d_rec = (u32 *)be.alloc_uninit(rec_cap * 4);
		u64 *d_bstat = (u64 *)be.alloc((size_t)tiles * 8);
		d_codes = (int8_t *)be.alloc_uninit(out_cap + 16);
		S1_LAUNCH(B, be, k_s1_bam_chain, dim3(tiles), dim3(S1_BLOCK), d_text, size, d_bstat, d_ticket, d_rec, rec_cap, d_small, d_err);
		if (const int rc = s1_read_errors(be, small, d_small, 3, S1_TEXT_BAD | KERR_CAPACITY, R))
			return rc;
		const u64 n_rec = small[0];
		if (n_rec) {
			const u32 dt = (u32)((n_rec + S1_BLOCK - 1) / S1_BLOCK);
			u64 *d_dstat = (u64 *)be.alloc((size_t)dt * 8);
			be.zero(d_ticket, 4);
			S1_LAUNCH(B, be, k_s1_bam_decode, dim3(dt), dim3(S1_BLOCK), d_text, size, (const u32 *)d_rec, n_rec, P.both_strands, P.line_cap, d_dstat, d_ticket, d_codes, out_cap,
			          d_small, d_err);
			if (const int rc = s1_read_errors(be, small, d_small, 3, S1_TEXT_BAD | KERR_CAPACITY, R))
				return rc;
		}
		n = n_rec ? small[1] : 0;
		R.n_symbols = n;
		R.n_reads = n_rec ? small[0] : 0;
	} else if (P.multiline_fasta) {
		/* ---- text -> codes, multi-line FASTA: per-sequence arrays sized by titles (two bytes each at least), not by lines */
		const u64 seq_cap = size / 2 + 2;
		const u32 tiles = (u32)((size + S1_TXT_TILE - 1) / S1_TXT_TILE);
		d_codes = (int8_t *)be.alloc(size + 16);
		u64 *d_seq_start = (u64 *)be.alloc_uninit(seq_cap * 8);
		u64 *d_status = (u64 *)be.alloc((size_t)tiles * 24);
		S1_LAUNCH(B, be, k_s1_ml_text_to_codes, dim3(tiles), dim3(S1_BLOCK), d_text, size, d_status, d_status + tiles, d_status + 2 * (size_t)tiles, d_ticket, d_codes,
		          d_seq_start, seq_cap, d_small, d_err);
		if (const int rc = s1_read_errors(be, small, d_small, 3, S1_TEXT_BAD | KERR_CAPACITY, R))
			return rc;
		n = small[1];
		R.n_symbols = n;
		R.n_reads = small[0];
		S1_LAUNCH(B, be, k_s1_ml_marks, dim3((u32)((small[0] + 1 + 255) / 256)), dim3(256), d_text, n, (const u64 *)d_seq_start, small[0], P.line_cap, stride, d_codes,
		          d_has_marks);
	} else {
		/* ---- text -> codes. A line of real reads is tens of bytes; text with more line ends than size / 4 is not taken. */
		const u64 nl_cap = lpr ? size / 4 + 1024 : 1;
		const u32 tiles = (u32)((size + S1_TXT_TILE - 1) / S1_TXT_TILE);
		d_codes = (int8_t *)be.alloc(size + 16);
		u64 *d_nl = (u64 *)be.alloc(nl_cap * 8);
		u64 *d_seq_start = (u64 *)be.alloc_uninit((nl_cap / (lpr ? lpr : 1) + 2) * 8);
		u64 *d_status = (u64 *)be.alloc((size_t)tiles * 16);
		S1_LAUNCH(B, be, k_s1_text_to_codes, dim3(tiles), dim3(S1_BLOCK), d_text, size, lpr, d_status, d_status + tiles, d_ticket, d_codes, d_nl, nl_cap, d_seq_start, d_small,
		          d_err);
		if (const int rc = s1_read_errors(be, small, d_small, 3, S1_TEXT_BAD | KERR_CAPACITY, R))
			return rc;
		const u64 n_lines = small[0];
		n = small[1];
		R.n_symbols = n;
		if (lpr) {
			const u64 lines = n_lines + (text_ends_with_newline ? 0 : 1); /* titles in the part: every lpr-th line, an unterminated last line included */
			R.n_reads = (lines + lpr - 1) / lpr;
			S1_LAUNCH(B, be, k_s1_check_records, dim3((u32)((n_lines / lpr + 1 + 255) / 256)), dim3(256), d_text, size, (const u64 *)d_nl, n_lines, lpr, P.line_cap, stride,
			          (const u64 *)d_seq_start, d_codes, d_has_marks, d_err);
		} else if (n > stride) /* n_reads of a long-read part: the caller knows whether it took a title off */
			S1_LAUNCH(B, be, k_s1_mark_raw, dim3(1), dim3(256), d_codes, n, stride, d_has_marks);
	}
	R.d_raw_codes = d_codes;
	R.n_raw = n;
	/* ---- -hc: the compacted stream (pieces have become sequences of their own: no marks) replaces the code stream for everything below */
	const u64 *d_cut_marks = d_has_marks;
	if (P.homopolymer && n) {
		const u64 hc_cap = n + (n / stride + 1) * P.k; /* a mark adds its k - 1 tail codes and a separator; marks are `stride` apart */
		const u32 ht = (u32)((n + S1_TXT_TILE - 1) / S1_TXT_TILE);
		int8_t *d_hc = (int8_t *)be.alloc_uninit(hc_cap + 16);
		u64 *d_hstat = (u64 *)be.alloc((size_t)ht * 8);
		be.zero(d_ticket, 4);
		S1_LAUNCH(B, be, k_s1_hc_compact, dim3(ht), dim3(S1_BLOCK), (const int8_t *)d_codes, n, P.k, d_hstat, d_ticket, d_hc, hc_cap, d_small + 5, d_err);
		u64 hc[3]; /* ticket, error word | has_marks | compacted codes */
		if (const int rc = s1_read_errors(be, hc, d_small + 3, 0, S1_TEXT_BAD, R)) /* S1_TEXT_BAD: the record check ran beside the compaction */
			return rc;
		d_codes = d_hc;
		n = hc[2];
		d_cut_marks = nullptr;
	}
	F.d_small = d_small, F.d_has_marks = d_has_marks, F.d_ticket = d_ticket, F.d_err = d_err;
	F.d_cut_marks = d_cut_marks, F.d_codes = d_codes, F.n = n;
	if (wait_for_errors && !(P.homopolymer && n)) { /* the -hc block has just read the word */
		if (const int rc = s1_read_errors(be, small, d_small, 3, S1_TEXT_BAD, R))
			return rc;
	}
	return S1_CHAIN_OK;
}

template <class B> int s1_split_part(B &be, const uint8_t *d_text, u64 size, bool text_ends_with_newline, const S1PartParams &P, S1PartResult &R)
{
	const u32 nb = P.n_bins;
	S1Front F;
	const int front = s1_front_part(be, d_text, size, text_ends_with_newline, P, R, F, false);
	R.bin_off.assign(nb, 0);
	R.bin_bytes.assign(nb, 0);
	R.bin_sk.assign(nb, 0);
	R.bin_kmers.assign(nb, 0);
	R.bin_plus_x.assign(nb, 0);
	if (front != S1_CHAIN_OK || !size)
		return front;
	u64 *const d_small = F.d_small;
	u32 *const d_ticket = F.d_ticket, *const d_err = F.d_err;
	const u64 *const d_cut_marks = F.d_cut_marks;
	const int8_t *const d_codes = F.d_codes;
	const u64 n = F.n;
	u64 small[4];
	u32 err;
	/* ---- codes -> super-k-mers. Their number is only known afterwards: a guess, and a second cut with the exact number when it was short. */
	u64 n_sk = 0, cap = n / P.sk_guess_div + 4096;
	u64 *d_pos = nullptr;
	u32 *d_len = nullptr, *d_sig = nullptr;
	if (n) {
		const u32 ct = (u32)s1_cut_tiles(n);
		u64 *d_cstat = (u64 *)be.alloc((size_t)ct * 16);
		for (int attempt = 0; attempt < 2; ++attempt) {
			d_pos = (u64 *)be.alloc_uninit(cap * 8);
			d_len = (u32 *)be.alloc_uninit(cap * 4);
			d_sig = (u32 *)be.alloc_uninit(cap * 4);
			if (attempt) {
				be.zero(d_cstat, (size_t)ct * 16);
				be.zero(d_small + 2, 8);
			}
			be.zero(d_ticket, 4);
			S1_LAUNCH(B, be, (k_s1_cut<true>), dim3(ct), dim3(S1_BLOCK), (const u32 *)nullptr, (const int8_t *)d_codes, P.m, n, P.k, d_cstat, d_cstat + ct, d_ticket, d_pos,
			          d_len, d_sig, cap, d_small + 2, d_cut_marks, d_err);
			if (!be.d2h(small, d_small, sizeof small))
				return S1_CHAIN_BACKEND_FAILURE;
			err = (u32)(small[3] >> 32);
			n_sk = small[2];
			if (n_sk <= cap || (err & S1_TEXT_BAD))
				break;
			cap = n_sk; /* KERR_CAPACITY was raised by the short attempt: cleared with the word below */
			be.zero(d_err, 4);
			err &= ~KERR_CAPACITY;
			if (err)
				break;
		}
	} else {
		if (!be.d2h(small, d_small, sizeof small))
			return S1_CHAIN_BACKEND_FAILURE;
		err = (u32)(small[3] >> 32);
	}
	if (const int rc = s1_classify(err, S1_TEXT_BAD, R)) /* S1_TEXT_BAD: the record check ran beside the cut */
		return rc;
	R.n_superkmers = n_sk;
	/* ---- per-bin sums, layout, records */
	u64 *d_tot = (u64 *)be.alloc((size_t)4 * nb * 8); /* bytes | super-k-mers | k-mers | n_plus_x_recs */
	u64 *d_lay = (u64 *)be.alloc((size_t)(3 * nb + 2) * 8);
	const u32 sk_tiles = (u32)((n_sk + S1_SK_TILE - 1) / S1_SK_TILE);
	if (sk_tiles) {
		S1_LAUNCH(B, be, k_s1_bin_totals, dim3(sk_tiles), dim3(256), (const u32 *)d_len, (const u32 *)d_sig, n_sk, P.k, P.d_sig_to_bin, nb, d_tot, d_tot + nb, d_tot + 2 * nb,
		          d_err);
		S1_LAUNCH(B, be, k_s1_bin_plus_x, dim3(sk_tiles), dim3(256), (const int8_t *)d_codes, (const u64 *)d_pos, (const u32 *)d_len, (const u32 *)d_sig, n_sk, P.k, P.max_x,
		          P.both_strands, P.d_sig_to_bin, nb, d_tot + 3 * nb);
	}
	S1_LAUNCH(B, be, k_s1_bin_layout, dim3(1), dim3(256), (const u64 *)d_tot, nb, d_lay, d_lay + nb + 1, d_lay + 2 * nb + 2, (u64 *)nullptr);
	std::vector<u64> lay(2 * (size_t)nb + 2);
	if (!be.d2h(lay.data(), d_lay, lay.size() * 8))
		return S1_CHAIN_BACKEND_FAILURE;
	if (const int rc = s1_read_errors(be, small, d_small, 3, 0, R)) /* a signature the map does not know (KERR_CORRUPT from k_s1_bin_totals): nothing is emitted */
		return rc;
	const u64 recs_bytes = lay[nb], n_packs = lay[2 * (size_t)nb + 1];
	uint8_t *d_recs = (uint8_t *)be.alloc(recs_bytes + 16);
	u64 *d_packs = (u64 *)be.alloc((n_packs + 1) * 8);
	S1_LAUNCH(B, be, k_s1_bin_layout, dim3(1), dim3(256), (const u64 *)d_tot, nb, d_lay, d_lay + nb + 1, d_lay + 2 * nb + 2, d_packs);
	if (sk_tiles && !P.sorted_emit)
		S1_LAUNCH(B, be, k_s1_emit, dim3(sk_tiles), dim3(256), (const int8_t *)d_codes, (const u64 *)d_pos, (const u32 *)d_len, (const u32 *)d_sig, n_sk, P.k, P.d_sig_to_bin, nb,
		          (const u64 *)d_lay, (const u64 *)(d_lay + nb + 1), d_lay + 2 * nb + 2, d_recs, d_packs);
	if (sk_tiles && P.sorted_emit) {
		/* bytes of all bins before each bin, from the sums already on the device */
		std::vector<u64> cum(nb + 1, 0), bytes_now(nb);
		if (!be.d2h(bytes_now.data(), d_tot, (size_t)nb * 8))
			return S1_CHAIN_BACKEND_FAILURE;
		for (u32 b = 0; b < nb; ++b)
			cum[b + 1] = cum[b] + bytes_now[b];
		u64 *d_cum = (u64 *)be.alloc((size_t)(nb + 1) * 8);
		be.h2d(d_cum, cum.data(), (size_t)(nb + 1) * 8);
		u64 *d_keys = (u64 *)be.alloc_uninit(n_sk * 8), *d_ktmp = (u64 *)be.alloc_uninit(n_sk * 8);
		S1_LAUNCH(B, be, k_s1_sort_keys, dim3((u32)((n_sk + 255) / 256)), dim3(256), (const u32 *)d_sig, n_sk, P.d_sig_to_bin, nb, d_keys, d_err);
		const u64 *d_sorted = be.sort_by_low16(d_keys, d_ktmp, n_sk);
		const u32 et = (u32)((n_sk + S1_TILE - 1) / S1_TILE);
		u64 *d_estat = (u64 *)be.alloc((size_t)et * 8);
		be.zero(d_ticket, 4);
		S1_LAUNCH(B, be, k_s1_emit_sorted, dim3(et), dim3(S1_BLOCK), d_sorted, n_sk, (const int8_t *)d_codes, (const u64 *)d_pos, (const u32 *)d_len, P.k, nb, (const u64 *)d_lay,
		          (const u64 *)(d_lay + nb + 1), (const u64 *)d_cum, d_estat, d_ticket, d_recs, d_packs, d_err);
	}
	std::vector<u64> tot(4 * (size_t)nb);
	if (!be.d2h(tot.data(), d_tot, tot.size() * 8))
		return S1_CHAIN_BACKEND_FAILURE;
	if (const int rc = s1_read_errors(be, small, d_small, 3, 0, R))
		return rc;
	for (u32 b = 0; b < nb; ++b) {
		R.bin_off[b] = lay[b];
		R.bin_bytes[b] = tot[b];
		R.bin_sk[b] = tot[nb + b];
		R.bin_kmers[b] = tot[2 * (size_t)nb + b];
		R.bin_plus_x[b] = tot[3 * (size_t)nb + b];
	}
	R.d_recs = d_recs;
	R.recs_bytes = recs_bytes;
	return S1_CHAIN_OK;
}

/* Histogram estimation while counting (--opt-out-size): the k-mers of a part's RAW code stream (S1PartResult::d_raw_codes, n_raw) into the two counter arrays
 * of 2^r entries at d_counters (k_s1_nthash_estimate; s, r: the reference's CntHashEstimator). Not part of s1_split_part: a part whose call fails, or is
 * repeated with a larger buffer, must add nothing, so the caller launches this once nothing can fail any more, and waits for it with what it waits for last. */
template <class B> void s1_estimate_part(B &be, const int8_t *d_raw_codes, u64 n, u32 k, u32 s, u32 r, u32 *d_counters)
{
	if (n < k)
		return;
	S1_LAUNCH(B, be, k_s1_nthash_estimate, dim3((u32)((n + S1_TXT_TILE - 1) / S1_TXT_TILE)), dim3(S1_BLOCK), d_raw_codes, n, k, s, r, s1_nt_seeds(k), d_counters);
}

/* Small k (k <= 13, the reference's "small k optimization", CSplitter::ProcessReadsSmallK splitter.cpp:682-805): every window of k valid codes of the stream
 * the front half leaves (S1Front::d_codes, n: the raw stream, or the -hc stream with -hc) is one k-mer, counted in the table of 4^k 64-bit counters at
 * d_table; *d_total (zeroed by the caller) receives the number of windows. Like s1_estimate_part the caller launches this once nothing can fail any more.
 * Workgroups are persistent over tiles: max_wgs of them at most, and never more than S1_SMALLK_MAX_TILES_PER_WG tiles each (their 32-bit LDS counters).
 * lds_k: the largest k whose table is kept in LDS (S1_SMALLK_LDS_K; 0 = every k adds straight into d_table). */
template <class B> void s1_smallk_part(B &be, const int8_t *d_codes, u64 n, u32 k, u32 both_strands, u64 *d_table, u64 *d_total, u32 max_wgs = S1_SMALLK_WGS, u32 lds_k = S1_SMALLK_LDS_K)
{
	if (n < k)
		return;
	const u64 tiles = (n + S1_TXT_TILE - 1) / S1_TXT_TILE, least = (tiles + S1_SMALLK_MAX_TILES_PER_WG - 1) / S1_SMALLK_MAX_TILES_PER_WG;
	u64 grid = tiles < max_wgs ? tiles : (max_wgs ? max_wgs : 1);
	if (grid < least)
		grid = least;
	if (k <= lds_k && k <= 6)
		S1_LAUNCH(B, be, (k_s1_smallk_count<6>), dim3((u32)grid), dim3(S1_BLOCK), d_codes, n, k, both_strands, d_table, d_total);
	else if (k <= lds_k && k == 7)
		S1_LAUNCH(B, be, (k_s1_smallk_count<7>), dim3((u32)grid), dim3(S1_BLOCK), d_codes, n, k, both_strands, d_table, d_total);
	else
		S1_LAUNCH(B, be, (k_s1_smallk_count<0>), dim3((u32)grid), dim3(S1_BLOCK), d_codes, n, k, both_strands, d_table, d_total);
}

/* Stage 0 (CSplitter::CalcStats, splitter.cpp:439-533): every window of k valid codes of the stream the front half leaves (S1Front::d_codes, n) adds one to the entry
 * of its signature among the 4^m + 1 32-bit counters at d_table (k_s1_sig_stats); *d_total (zeroed by the caller) receives the number of windows. Like
 * s1_smallk_part the caller launches this once the part can no longer fail: a part that is refused or not covered leaves the table untouched. max_wgs: the
 * persistent workgroups at most; lds_m: the largest m whose table is kept in LDS (at most S1_STATS_LDS_M; 0 = every m adds straight into d_table). */
template <class B> void s1_sigstats_part(B &be, const int8_t *d_codes, u64 n, u32 k, u32 m, u32 *d_table, u64 *d_total, u32 max_wgs = S1_STATS_WGS, u32 lds_m = S1_STATS_LDS_M_DEFAULT)
{
	if (n < k)
		return;
	const u64 tiles = (n - k + 1 + S1_STATS_TILE - 1) / S1_STATS_TILE;
	const u64 grid = tiles < max_wgs ? tiles : (max_wgs ? max_wgs : 1);
	if (m <= lds_m && m <= S1_STATS_LDS_M)
		S1_LAUNCH(B, be, (k_s1_sig_stats<(int)S1_STATS_LDS_M>), dim3((u32)grid), dim3(S1_BLOCK), d_codes, n, k, m, d_table, d_total);
	else
		S1_LAUNCH(B, be, (k_s1_sig_stats<0>), dim3((u32)grid), dim3(S1_BLOCK), d_codes, n, k, m, d_table, d_total);
}

#endif
