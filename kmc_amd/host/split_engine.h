/*
 * kmc_amd/host/split_engine.h — the per-part compute engine the stage-1 worker (kb_splitter_plugin.h) drives.
 *
 * One engine instance per splitter thread. split_part() does for one part of input text what CSplitter::ProcessReads does with its n_bins
 * CKmerBinCollectors (splitter.cpp:557-672, kb_collector.cpp:34-106) up to, but not including, the bin-part buffers: it returns the bin
 * records of the part grouped by bin, with the three sums the collector keeps per buffer. The worker copies them into pmm_bins buffers
 * and pushes those to the storer exactly as the collectors would.
 *   - oracle engine: oracle/stage1_oracle.c (TEST ONLY: oracle/oracle_engine_s1.h -> oracle/_ref/kmc_oracle_s1; pins the worker's protocol
 *     and the oracle's parser and k+x-mer bookkeeping to the reference: the database must be byte-identical)
 *   - emulated engine: the stage-1 kernels under the CPU emulation (TEST ONLY: tests/hipemu/emu_split_engine.cpp -> oracle/_ref/kmc_emu_s1)
 *   - HIP engine   : kmc_hip_split_part of include/kmc_hip.h through hip_split_loader.cpp -> oracle/_ref/kmc_hip_s1 (proven on the
 *     CPU over an emulated HIP runtime; its first run on a GPU is the round-end bench / xfail-marked test of round 2)
 */
#ifndef KMC_AMD_SPLIT_ENGINE_H
#define KMC_AMD_SPLIT_ENGINE_H

#include <stdint.h>
#include <string>

struct KmcSplitParams {
	uint32_t kmer_len, signature_len, n_bins, max_x;
	int both_strands;
	int file_type;             /* 0 = FASTA (one line per sequence), 1 = FASTQ, 2 = multi-line FASTA (ReadType::na parts; only for an engine that covers_multiline_fasta()),
	                            * 4 = BAM alignment records (ReadType::na parts, GetSeq splitter.cpp:326-419; only for an engine that covers_bam()) */
	uint64_t line_cap;         /* mem_part_pmm_reads: longer lines are cut into pieces overlapping by kmer_len - 1 symbols (splitter.cpp:141-145) */
	const int32_t *sig_to_bin; /* CSignatureMapper's map, 4^signature_len + 1 entries (s_mapper.h:232) */
	int homopolymer_compressed = 0; /* -hc: every return of GetSeq is compressed on its own (splitter.cpp:424-435, :575-581); only for an engine that
	                                 * covers_homopolymer_compression() */
	uint32_t estimate_s = 0, estimate_r = 0; /* --opt-out-size: s and r of the reference's CntHashEstimator (k is kmer_len); both 0 = off. Only for an engine
	                                          * that covers_histogram_estimation(): every part's k-mers then go to the estimator of estimate_open() */
};

/* valid until the next split_part() on the same engine */
struct KmcSplitResult {
	const uint8_t *recs;       /* the records of all bins; bin b's are recs[bin_off[b] .. bin_off[b] + bin_bytes[b]) (a device engine aligns bins) */
	const uint64_t *bin_off, *bin_bytes; /* n_bins each */
	const uint64_t *bin_kmers, *bin_superkmers, *bin_plus_x; /* n_bins each: n_recs, n_super_kmers, n_plus_x_recs of the collector */
	uint64_t n_reads;          /* records whose title line the part holds (CSplitter::n_reads) */
};

/* split_part() returns 0, a negative error code, or KMC_SPLIT_UNCOVERED: the part is MALFORMED text the engine does not reproduce CSplitter::GetSeq
 * on (blank lines, quality of another length than its sequence, control characters ...): nothing was produced, and the worker stops the run (a build
 * with -DKMC_HIP_S1_REFERENCE_FALLBACK and $KMC_HIP_S1_FALLBACK=1 gives the part to the reference splitter instead).
 * long_read: the reader labelled the part ReadType::long_read (queues.h:40) — an optional title, then symbols only (GetSeqLongRead, splitter.cpp:70-86). */
enum { KMC_SPLIT_UNCOVERED = 1 };

struct KmcSplitEngine {
	virtual ~KmcSplitEngine() {}
	virtual int split_part(const uint8_t *text, uint64_t size, bool long_read, KmcSplitResult &out) = 0;
	virtual std::string last_error() = 0;
	/* parts of multi-line FASTA (file_type 2: CFastqReader::GetPartFromMultilneFasta, split as CSplitter::GetSeq's MULTILINE_FASTA branch) */
	virtual bool covers_multiline_fasta() const { return false; }
	/* parts of BAM records (file_type 4: whole records as the reference's BAM readers hand them out, fastq_reader.cpp:191-362) */
	virtual bool covers_bam() const { return false; }
	/* -hc (KmcSplitParams::homopolymer_compressed), with every file type and with long-read parts */
	virtual bool covers_homopolymer_compression() const { return false; }
	/* histogram estimation while counting (--opt-out-size; KmcSplitParams::estimate_s / _r): the engine keeps the two counter arrays of CntHashEstimator
	 * (ntHashWrapper.h: 2 x 2^r 32-bit counters, type 0 first) wherever its parts are split, and adds every part's k-mers to them.
	 * estimate_open : makes the (zeroed) counters of this engine's device; once per engine, in front of its first part. 0 or an error code.
	 * estimate_drain: when every engine of the run has split its last part: ADDS entries [first, first + count) of the counters of every device an
	 *                 estimator was opened on to dst[0 .. count) (wrapping at 2^32), count <= 2^24 (64 MB); the call that takes the last entry also closes
	 *                 the estimators. 0 or an error code. */
	virtual bool covers_histogram_estimation() const { return false; }
	virtual int estimate_open() { return -1; }
	virtual int estimate_drain(uint64_t /*first*/, uint64_t /*count*/, uint32_t * /*dst*/) { return -1; }
	/* small k (k <= 13, the reference's "small k optimization": CWSmallKSplitter, splitter.cpp:929-983, over CSplitter::ProcessReadsSmallK :682-805): the engine keeps
	 * ONE table of 4^kmer_len 64-bit counters wherever its parts are counted, instead of one per worker. An engine made for this path gets sig_to_bin = nullptr
	 * (there is no signature map in this mode) and must not need signature_len, n_bins or max_x; only kmer_len, both_strands, file_type, line_cap and
	 * homopolymer_compressed count.
	 * smallk_open : makes the (zeroed) table of this engine's device; once per engine, in front of its first part. 0 or an error code.
	 * smallk_part : counts one part: n_reads as split_part gives it, n_kmers = the k-mers counted (CSplitter::total_kmers). 0, a negative error code or
	 *               KMC_SPLIT_UNCOVERED; a call that does not return 0 has added nothing.
	 * smallk_drain: when every engine of the run has counted its last part: ADDS entries [first, first + count) of the table of every device one was opened on
	 *               to dst[0 .. count), count <= 2^22 (32 MB); the call that takes the last entry also closes the tables. 0 or an error code. */
	virtual bool covers_small_k() const { return false; }
	virtual int smallk_open() { return -1; }
	virtual int smallk_part(const uint8_t * /*text*/, uint64_t /*size*/, bool /*long_read*/, uint64_t & /*n_reads*/, uint64_t & /*n_kmers*/) { return -1; }
	virtual int smallk_drain(uint64_t /*first*/, uint64_t /*count*/, uint64_t * /*dst*/) { return -1; }
	/* stage 0, the signature statistics (CWStatsSplitter, splitter.h:118, splitter.cpp:878-925, over CSplitter::CalcStats :439-533): the engine keeps ONE array of
	 * 4^signature_len + 1 32-bit counters wherever its parts are looked at, instead of one per worker. An engine made for this path gets sig_to_bin = nullptr (the
	 * map is what the statistics are for) and must not need n_bins or max_x; kmer_len, signature_len, file_type, line_cap and homopolymer_compressed count.
	 * sigstats_open : makes the (zeroed) array of this engine's device; once per engine, in front of its first part. 0 or an error code.
	 * sigstats_part : one part: n_reads as split_part gives it, n_kmers = the windows added (the sum of 1 + len - kmer_len over the part's super-k-mers). 0, a
	 *                 negative error code or KMC_SPLIT_UNCOVERED; a call that does not return 0 has added nothing.
	 * sigstats_drain: when every engine of the run has seen its last part: ADDS entries [first, first + count) of the array of every device one was opened on to
	 *                 dst[0 .. count) (wrapping at 2^32), count <= 2^23; the call that takes the last entry also closes the arrays. 0 or an error code. */
	virtual bool covers_signature_stats() const { return false; }
	virtual int sigstats_open() { return -1; }
	virtual int sigstats_part(const uint8_t * /*text*/, uint64_t /*size*/, bool /*long_read*/, uint64_t & /*n_reads*/, uint64_t & /*n_kmers*/) { return -1; }
	virtual int sigstats_drain(uint64_t /*first*/, uint64_t /*count*/, uint32_t * /*dst*/) { return -1; }
};

/* Provided by exactly one engine implementation linked into the binary. */
KmcSplitEngine *kmc_make_split_engine(const KmcSplitParams &params, int worker_idx, int n_workers);

#endif
