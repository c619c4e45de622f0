/*
 * kmc_amd/host/kb_splitter_plugin.h — the stage-1 splitter worker of kmc_core with the splitting done by an engine
 * (docs/history/DESIGN_rounds_1_to_5.md §9): the drop-in boundary of a GPU stage 1.
 *
 * Drop-in for the reference's CWSplitter (splitter.h:100-113, splitter.cpp:814-867): the same class name, constructor, operator()(),
 * GetTotal() and destructor, so CKMC<SIZE>::ProcessStage1_impl (kmc.h:1274-1362) builds against it unchanged. Compiled in with
 * `-include kb_splitter_plugin.h` ahead of kmc_runner.cpp; the reference's own splitter.cpp is compiled with -DCWSplitter=CWSplitter_ref
 * (oracle/Makefile), which is what this header declares first: CSplitter stays the reference's for what is NOT this worker (the estimate-only
 * worker uses it directly, kmc.h:1100-1200; the small-k worker is CWSmallKSplitter_dev and stage 0's signature statistics CWStatsSplitter_dev at the end of this header); this worker itself never calls it
 * (see FAILS CLOSED below).
 *
 * Protocol kept from CWSplitter::operator() + CSplitter::ProcessReads + CKmerBinCollector:
 *   pq->pop(part, size, read_type) -> [engine: text -> sequences -> super-k-mers -> bin records] -> pmm_fastq->free(part)
 *   per bin a buffer of Params.bin_part_size bytes from pmm_bins; records are appended whole; a buffer that cannot take the next piece is
 *   pushed: bpq->push(bin, buffer, used, bin_part_size, {one expander pack: (used, n_plus_x_recs)}) + bd->update(bin, used, n_recs,
 *   n_plus_x_recs, n_super_kmers) (kb_collector.cpp:88-106; the reference never closes a pack early: its super_kmer_no is not incremented
 *   in 3.2.4, kb_collector.cpp:36-41); at the end every non-empty buffer is pushed, then bpq->mark_completed().
 * Differences a downstream stage can see: the ORDER of records inside a bin (records of one part stay together; the reference interleaves
 * reads) — stage 2 sorts, the database is byte-identical — and buffers are reserved when a bin first gets data, not all n_bins up front.
 * The reference pushes a buffer when the next RECORD does not fit; here the unit is the part's piece for that bin (its three sums come
 * from the engine in one go), walked record by record only when a piece is larger than what an empty buffer holds.
 *
 * FAILS CLOSED (round 5): this worker has no path into the reference's CSplitter. What the engine does not cover stops the run through
 * CCriticalErrorHandler with a message that names it —
 *   per job : multi-line FASTA unless the engine covers_multiline_fasta(), BAM unless it covers_bam() (a KMC database reaches the splitter as single-line FASTA,
 *             ">\n<k-mer>\n" per k-mer, binary_reader.h:238-304, and GetSeq treats it as such, splitter.cpp:100: file_type 0), homopolymer compression (-hc) unless the engine covers_homopolymer_compression(), histogram estimation while counting (--opt-out-size) unless the engine covers_histogram_estimation() (-e alone runs the reference's estimate-only worker, not this one):
 *             "use kmc_hip" (the reference's stage 1 + this library's stage 2) is the answer the message gives;
 *   per part: KMC_SPLIT_UNCOVERED — MALFORMED text that CSplitter::GetSeq happens to tolerate (blank lines, a quality string of another length than its
 *             sequence, control characters, a lone '\r'); for BAM: records that do not end with the part, a block_size that does not hold its record, a
 *             read of mem_part_pmm_reads bases or more.
 * Parts the reader labelled ReadType::long_read (queues.h:40) and lines of mem_part_pmm_reads symbols or more go through the engine like any other, and so
 * do the ReadType::na parts of multi-line FASTA (fastq_reader.cpp:399-468, :579-583) with an engine that covers them (file_type 2). With -hc the engine
 * compresses every return of GetSeq on its own, as ProcessReads does (splitter.cpp:575-581); the estimate worker stays the
 * reference's and honours the flag itself (the small-k and stage-0 workers below pass it to their engines), and n_reads does not depend on it.
 * With --opt-out-size (ESTIMATE_AND_COUNT_KMERS) the reference's splitter hashes every k-mer a second time into Queues.ntHashEstimator (splitter.cpp:576-577),
 * an object that exists before the workers are constructed (kmc.h:1277-1293). Here the engine keeps those counters where it splits: every worker opens the
 * estimator of its engine's device with the object's own s and r, the LAST worker to finish adds the counters of every device into the object's arrays
 * (in chunks of 64 MB), and kmc.h:1329-1333 then runs the reference's own EstimateHistogram on them — no floating-point line is restated here. s, r and the
 * counters are private members; they are read through pointers to members obtained by explicit instantiation (access checking does not apply to the
 * arguments of one): the class, its layout and the reference's sources stay as they are.
 * Only a build with -DKMC_HIP_S1_REFERENCE_FALLBACK (no shipped binary has it; oracle/_ref/kmc_emu_s1_fb is the test build) AND $KMC_HIP_S1_FALLBACK=1
 * in the environment hands such jobs / parts to the reference (CWSplitter_ref / a CSplitter of this thread, our buffers pushed first) and says so on stderr;
 * nothing run that way is covered by this repo's parity claims.
 */
#ifndef KMC_AMD_KB_SPLITTER_PLUGIN_H
#define KMC_AMD_KB_SPLITTER_PLUGIN_H

#define CWSplitter CWSplitter_ref
#include "splitter.h" /* the reference header, read-only: CSplitter, the *_ref worker, the stats / small-k / estimate workers (untouched) */
#undef CWSplitter

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <list>
#include <memory>
#include <sstream>
#include <vector>

#include "critical_error_handler.h"
#include "split_engine.h"
#include "kmc_order.h" /* KmcTimeline: where does the wall clock go between the stages (KMC_HIP_VERBOSE=1) */

/* n_plus_x_recs of one record (kb_collector.cpp:83-100, kb_collector.h:72-118), from the PACKED record: only needed when a bin's piece of a
 * part has to be cut (it does not fit an empty buffer), because then the engine's sum for the piece cannot be used. */
static inline uint32_t kmc_record_plus_x(const uint8_t *rec, uint32_t kmer_len, uint32_t max_x, bool both_strands)
{
	if (!max_x)
		return 0;
	const uint32_t n = kmer_len + rec[0];
	if (!both_strands)
		return 1 + (n - kmer_len) / (max_x + 1);
	auto sym = [&](uint32_t i) -> uint32_t { return (rec[1 + (i >> 2)] >> (6 - 2 * (i & 3))) & 3u; };
	uint8_t fwd = (uint8_t)((sym(0) << 6) | (sym(1) << 4) | (sym(2) << 2) | sym(3));
	uint8_t rc = (uint8_t)(((3 - sym(kmer_len - 1)) << 6) | ((3 - sym(kmer_len - 2)) << 4) | ((3 - sym(kmer_len - 3)) << 2) | (3 - sym(kmer_len - 4)));
	auto cmp = [](uint8_t a, uint8_t b) { return a < b ? 0 : (b < a ? 1 : 2); };
	int state = cmp(fwd, rc);
	uint32_t run = 0, total = 0;
	for (uint32_t i = 0; i + kmer_len < n; ++i) {
		rc = (uint8_t)((rc >> 2) | ((3 - sym(kmer_len + i)) << 6));
		fwd = (uint8_t)((fwd << 2) | sym(4 + i));
		const int s = cmp(fwd, rc);
		if (s == state) {
			if (s == 2)
				++total; /* a tie: every k-mer is its own record */
			else
				++run;
		} else {
			state = s;
			total += 1 + run / (max_x + 1);
			run = 0;
		}
	}
	return total + 1 + run / (max_x + 1);
}

/* pointers to private members of CntHashEstimator, handed out by explicit instantiations (C++14 [temp.explicit]/12); this header is part of ONE translation
 * unit per binary (-include ahead of kmc_runner.cpp) */
namespace kmc_hip_est_access {
template <class Tag> struct Stowed {
	static typename Tag::type value;
};
template <class Tag> typename Tag::type Stowed<Tag>::value;
template <class Tag, typename Tag::type P> struct Stow {
	Stow() { Stowed<Tag>::value = P; }
	static Stow instance;
};
template <class Tag, typename Tag::type P> Stow<Tag, P> Stow<Tag, P>::instance;
struct S {
	typedef uint32_t CntHashEstimator::*type;
};
struct R {
	typedef uint32_t CntHashEstimator::*type;
};
struct Counters {
	typedef uint32_t *(CntHashEstimator::*type)[2];
};
template struct Stow<S, &CntHashEstimator::s>;
template struct Stow<R, &CntHashEstimator::r>;
template struct Stow<Counters, &CntHashEstimator::counters>;
inline uint32_t s_of(CntHashEstimator &e) { return e.*Stowed<S>::value; }
inline uint32_t r_of(CntHashEstimator &e) { return e.*Stowed<R>::value; }
inline uint32_t *counters_of(CntHashEstimator &e, int type) { return (e.*Stowed<Counters>::value)[type]; }
} // namespace kmc_hip_est_access

/* KMC_SPLIT_UNCOVERED: what stops the run, by the kind of part (both workers of this header) */
static inline void kmc_hip_s1_stop_uncovered_part(InputType file_type, ReadType read_type)
{
	if (file_type == InputType::BAM)
		CCriticalErrorHandler::Inst().HandleCriticalError(
		    "Error: stage 1 on the device: a part of the BAM input is not covered: its alignment records do not end exactly at the end of the part, a "
		    "block_size is smaller than its record's header, name, cigar, bases and qualities (or negative), or a read that is counted has "
		    "mem_part_pmm_reads bases or more. Run this input with kmc_hip (the reference's stage 1, stage 2 on the device).");
	if (read_type == ReadType::na)
		CCriticalErrorHandler::Inst().HandleCriticalError(
		    "Error: stage 1 on the device: a part of the multi-line FASTA input ends inside a title line (a title longer than the reader's part). "
		    "Run this input with kmc_hip (the reference's stage 1, stage 2 on the device).");
	CCriticalErrorHandler::Inst().HandleCriticalError(
	    "Error: stage 1 on the device: a part of the input is malformed FASTA / FASTQ text (a blank line, a quality string of another length than its "
	    "sequence, a control character or a lone carriage return). The device splitter does not guess what such text means; "
	    "run this input with kmc_hip (the reference's stage 1, stage 2 on the device).");
}

class CWSplitter {
	struct BinBuf {
		uchar *buf = nullptr;
		uint32 pos = 0;
		uint64 n_recs = 0, n_plus_x = 0, n_super = 0;
	};
	CPartQueue *pq;
	CBinPartQueue *bpq;
	CBinDesc *bd;
	CMemoryPool *pmm_fastq, *pmm_bins;
	CKMCParams *params;
	CKMCQueues *queues;
#ifdef KMC_HIP_S1_REFERENCE_FALLBACK
	std::unique_ptr<CWSplitter_ref> ref;    /* non-null: the reference worker runs the whole job */
	std::unique_ptr<CSplitter> ref_splitter; /* uncovered parts of this thread */
	bool fallback_on = false;               /* $KMC_HIP_S1_FALLBACK=1 */
#endif
	std::unique_ptr<KmcSplitEngine> engine;
	std::vector<BinBuf> bins;
	uint32 kmer_len, max_x, buffer_size;
	bool both_strands;
	uint64 n_reads = 0;
	/* KMC_HIP_VERBOSE=1: one line per worker on stderr when it finishes */
	uint64 st_parts = 0, st_long_parts = 0, st_ml_parts = 0, st_bam_parts = 0, st_uncovered_parts = 0, st_pieces = 0, st_cut_pieces = 0, st_pushes = 0, st_bytes = 0;
	long long st_engine_ns = 0;

	static const char *uncovered_job(const CKMCParams &P, bool multiline_covered, bool homopolymer_covered, bool estimate_covered, bool bam_covered)
	{
		if (P.file_type != InputType::FASTA && P.file_type != InputType::FASTQ && P.file_type != InputType::KMC && !(P.file_type == InputType::MULTILINE_FASTA && multiline_covered) &&
		    !(P.file_type == InputType::BAM && bam_covered))
			return "an input format other than FASTA / FASTQ (multi-line FASTA, BAM, KMC)";
		if (P.homopolymer_compressed && !homopolymer_covered)
			return "homopolymer compression (-hc)";
		if (P.estimateHistogramCfg == KMC::EstimateHistogramCfg::ESTIMATE_AND_COUNT_KMERS && !estimate_covered)
			return "histogram estimation while counting (--opt-out-size)";
		return nullptr;
	}

	void push(uint32 bin_no) /* CKmerBinCollector::Flush, kb_collector.cpp:88-106 */
	{
		BinBuf &b = bins[bin_no];
		if (!b.buf)
			return;
		std::list<std::pair<uint64, uint64>> packs;
		if (b.pos)
			packs.push_back(std::make_pair((uint64)b.pos, b.n_plus_x));
		bpq->push(bin_no, b.buf, b.pos, buffer_size, packs);
		bd->update(bin_no, b.pos, b.n_recs, b.n_plus_x, b.n_super);
		++st_pushes;
		st_bytes += b.pos;
		b = BinBuf();
	}
	void append(uint32 bin_no, const uint8_t *recs, uint64 bytes, uint64 kmers, uint64 supers, uint64 plus_x)
	{
		BinBuf &b = bins[bin_no];
		if (b.buf && b.pos + bytes > buffer_size)
			push(bin_no);
		++st_pieces;
		if (bytes <= buffer_size) {
			if (!b.buf)
				pmm_bins->reserve(b.buf);
			memcpy(b.buf + b.pos, recs, bytes);
			b.pos += (uint32)bytes;
			b.n_recs += kmers;
			b.n_super += supers;
			b.n_plus_x += plus_x;
			return;
		}
		/* a piece larger than a buffer (one bin took most of a part): record by record, like the reference's collector */
		++st_cut_pieces;
		for (uint64 at = 0; at < bytes;) {
			const uint8_t *rec = recs + at;
			const uint32 len = 1 + (kmer_len + rec[0] + 3) / 4;
			if (b.buf && b.pos + len > buffer_size)
				push(bin_no);
			if (!b.buf)
				pmm_bins->reserve(b.buf);
			memcpy(b.buf + b.pos, rec, len);
			b.pos += len;
			b.n_recs += rec[0] + 1u;
			b.n_super += 1;
			b.n_plus_x += kmc_record_plus_x(rec, kmer_len, max_x, both_strands);
			at += len;
		}
	}
#ifdef KMC_HIP_S1_REFERENCE_FALLBACK
	/* the reference's own splitter for this part. Its collectors reserve n_bins pmm_bins buffers (one each, CKmerBinCollector's constructor), and the
	 * pool is sized for n_splitters x n_bins buffers beyond the storer's share (kmc.h:491-501): a worker must never hold two sets. So ours go to the
	 * storer first, and the reference splitter is completed (its collectors flushed and their buffers handed over) and dropped as soon as the part is
	 * through — held until the end of the run, a memory-tight run with mixed parts (nanopore FASTQ) could leave every worker waiting in
	 * pmm_bins->reserve with nothing left to free. */
	void to_reference(uchar *part, uint64 size, ReadType read_type)
	{
		push_all();
		ref_splitter = std::make_unique<CSplitter>(*params, *queues);
		ref_splitter->InitBins(*params, *queues);
		ref_splitter->ProcessReads(part, size, read_type);
		pmm_fastq->free(part);
		ref_splitter->Complete();
		uint64 n = 0;
		ref_splitter->GetTotal(n);
		n_reads += n;
		ref_splitter.reset();
	}
#endif
	void push_all()
	{
		for (uint32 i = 0; i < (uint32)bins.size(); ++i)
			push(i);
	}
	static bool estimating(CKMCParams &Params, CKMCQueues &Queues)
	{
		return Params.estimateHistogramCfg == KMC::EstimateHistogramCfg::ESTIMATE_AND_COUNT_KMERS && Queues.ntHashEstimator;
	}
	/* --opt-out-size, by the last worker to finish (every one of the n_splitters workers is constructed and run, kmc.h:1290-1294, :1323-1324): the counters
	 * of every device, added into the reference's arrays */
	static std::atomic<int> &finished_workers()
	{
		static std::atomic<int> finished{0};
		return finished;
	}
	void drain_estimate()
	{
		if (++finished_workers() != (int)params->n_splitters)
			return;
		CntHashEstimator &est = *queues->ntHashEstimator;
		const uint32_t r = kmc_hip_est_access::r_of(est);
		const uint64_t per_type = (uint64_t)1 << r, chunk = (uint64_t)1 << 24; /* 64 MB of counters at a time */
		const auto t0 = std::chrono::steady_clock::now();
		KmcTimeline::mark("splitter: histogram estimate, drain of the device counters starts");
		for (int type = 0; type < 2; ++type)
			for (uint64_t at = 0; at < per_type; at += chunk) {
				const uint64_t cnt = per_type - at < chunk ? per_type - at : chunk;
				if (int rc = engine->estimate_drain(type * per_type + at, cnt, kmc_hip_est_access::counters_of(est, type) + at)) {
					std::ostringstream ostr;
					ostr << "Error: stage-1 split engine failed to hand over the histogram estimate (code " << rc << "): " << engine->last_error();
					CCriticalErrorHandler::Inst().HandleCriticalError(ostr.str());
				}
			}
		KmcTimeline::mark("splitter: histogram estimate, device counters merged");
		if (getenv("KMC_HIP_VERBOSE"))
			fprintf(stderr, "[kmc_hip stage 1] histogram estimate on the device (--opt-out-size): s = %u, r = %u, counters of all devices merged into the reference's "
			                "estimator in %.3f s\n",
			        kmc_hip_est_access::s_of(est), r, std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count() * 1e-9);
	}
	static KmcSplitEngine *make_engine(CKMCParams &Params, CKMCQueues &Queues)
	{
		KmcSplitParams sp;
		sp.kmer_len = Params.kmer_len;
		sp.signature_len = Params.signature_len;
		sp.n_bins = Params.n_bins;
		sp.max_x = Params.max_x;
		sp.both_strands = Params.both_strands ? 1 : 0;
		sp.file_type = Params.file_type == InputType::FASTQ ? 1 : Params.file_type == InputType::MULTILINE_FASTA ? 2 : Params.file_type == InputType::BAM ? 4 : 0; /* KMC: 0 */
		sp.line_cap = (uint64_t)Params.mem_part_pmm_reads;
		sp.sig_to_bin = Queues.s_mapper->GetMap();
		sp.homopolymer_compressed = Params.homopolymer_compressed ? 1 : 0;
		if (estimating(Params, Queues)) {
			sp.estimate_s = kmc_hip_est_access::s_of(*Queues.ntHashEstimator);
			sp.estimate_r = kmc_hip_est_access::r_of(*Queues.ntHashEstimator);
		}
		static std::atomic<int> next_idx{0};
		return kmc_make_split_engine(sp, next_idx++ % (int)Params.n_splitters, (int)Params.n_splitters);
	}

public:
	CWSplitter(CKMCParams &Params, CKMCQueues &Queues)
	{
		params = &Params;
		queues = &Queues;
		pq = Queues.part_queue.get();
		bpq = Queues.bpq.get();
		bd = Queues.bd.get();
		pmm_fastq = Queues.pmm_fastq.get();
		pmm_bins = Queues.pmm_bins.get();
		kmer_len = Params.kmer_len;
		max_x = Params.max_x;
		both_strands = Params.both_strands;
		buffer_size = Params.bin_part_size;
		if (Params.file_type == InputType::MULTILINE_FASTA || Params.file_type == InputType::BAM || Params.homopolymer_compressed || estimating(Params, Queues))
			engine.reset(make_engine(Params, Queues)); /* whether the format / the compression / the estimate is covered is the engine's answer */
		if (const char *what = uncovered_job(Params, engine && engine->covers_multiline_fasta(), engine && engine->covers_homopolymer_compression(),
		                                     engine && engine->covers_histogram_estimation(), engine && engine->covers_bam())) {
#ifdef KMC_HIP_S1_REFERENCE_FALLBACK
			const char *fb = getenv("KMC_HIP_S1_FALLBACK");
			if (fb && fb[0] == '1') {
				static std::atomic<int> said{0};
				if (!said++)
					fprintf(stderr, "[kmc_hip stage 1] %s: the REFERENCE splitter runs stage 1 of this job (KMC_HIP_S1_FALLBACK=1); nothing of stage 1 is on the device\n", what);
				engine.reset();
				ref = std::make_unique<CWSplitter_ref>(Params, Queues);
				return;
			}
#endif
			std::ostringstream ostr;
			ostr << "Error: stage 1 on the device does not cover " << what << ". Run this job with kmc_hip (the reference's stage 1, stage 2 on the device).";
			CCriticalErrorHandler::Inst().HandleCriticalError(ostr.str());
		}
#ifdef KMC_HIP_S1_REFERENCE_FALLBACK
		{
			const char *fb = getenv("KMC_HIP_S1_FALLBACK");
			fallback_on = fb && fb[0] == '1';
		}
#endif
		bins.resize(Params.n_bins);
		if (!engine)
			engine.reset(make_engine(Params, Queues));
		if (!engine)
			CCriticalErrorHandler::Inst().HandleCriticalError("Error: no stage-1 split engine available");
		/* every worker of a run is constructed before the readers start (kmc.h:1290-1316), so before any worker can find the part queue completed and finish:
		 * counting from zero here serves a second run in the same process (library API), also behind a run whose workers left through the error handler */
		finished_workers() = 0;
		if (estimating(Params, Queues))
			if (int rc = engine->estimate_open()) {
				std::ostringstream ostr;
				ostr << "Error: stage-1 split engine could not open the histogram estimator (code " << rc << "): " << engine->last_error();
				CCriticalErrorHandler::Inst().HandleCriticalError(ostr.str());
			}
	}

	void operator()()
	{
		KmcTimeline::mark_first_last("splitter: first worker started", nullptr);
#ifdef KMC_HIP_S1_REFERENCE_FALLBACK
		if (ref) {
			(*ref)();
			KmcTimeline::mark_first_last(nullptr, "splitter: last worker done");
			return;
		}
#endif
		while (!pq->completed()) {
			uchar *part;
			uint64 size;
			ReadType read_type;
			if (!pq->pop(part, size, read_type))
				continue;
			/* only the multi-line FASTA reader (fastq_reader.cpp:399-468, :579-583) and the BAM readers (:191-362) make ReadType::na parts; the constructor
			 * took those formats only from an engine that covers them, and the engine was made with file_type 2 / 4 */
			if (read_type == ReadType::na && params->file_type != InputType::MULTILINE_FASTA && params->file_type != InputType::BAM)
				CCriticalErrorHandler::Inst().HandleCriticalError("Error: stage 1 on the device got a part of ReadType::na");
			const bool long_read = read_type == ReadType::long_read;
			st_long_parts += long_read ? 1 : 0;
			st_ml_parts += read_type == ReadType::na && params->file_type != InputType::BAM ? 1 : 0;
			st_bam_parts += read_type == ReadType::na && params->file_type == InputType::BAM ? 1 : 0;
			KmcSplitResult r;
			const auto t0 = std::chrono::steady_clock::now();
			const int rc = engine->split_part(part, size, long_read, r);
			st_engine_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
			if (rc == KMC_SPLIT_UNCOVERED) {
				++st_uncovered_parts;
#ifdef KMC_HIP_S1_REFERENCE_FALLBACK
				if (fallback_on) {
					to_reference(part, size, read_type);
					continue;
				}
#endif
				kmc_hip_s1_stop_uncovered_part(params->file_type, read_type);
			}
			if (rc != 0) {
				std::ostringstream ostr;
				ostr << "Error: stage-1 split engine failed (code " << rc << "): " << engine->last_error();
				CCriticalErrorHandler::Inst().HandleCriticalError(ostr.str());
			}
			++st_parts;
			pmm_fastq->free(part);
			n_reads += r.n_reads;
			for (uint32 b = 0; b < (uint32)bins.size(); ++b)
				if (r.bin_bytes[b])
					append(b, r.recs + r.bin_off[b], r.bin_bytes[b], r.bin_kmers[b], r.bin_superkmers[b], r.bin_plus_x[b]);
		}
		push_all();
		bpq->mark_completed();
		if (estimating(*params, *queues))
			drain_estimate();
		engine.reset();
		KmcTimeline::mark_first_last(nullptr, "splitter: last worker done");
		if (getenv("KMC_HIP_VERBOSE"))
			fprintf(stderr, "[kmc_hip stage 1] worker: %llu parts through the engine (%.3f s inside; %llu of them long-read parts), %llu uncovered parts, "
			                "%llu bin pieces (%llu cut record by record), %llu buffers / %.1f MB pushed, %llu multi-line FASTA parts, %llu BAM parts%s\n",
			        (unsigned long long)st_parts, st_engine_ns * 1e-9, (unsigned long long)st_long_parts, (unsigned long long)st_uncovered_parts,
			        (unsigned long long)st_pieces,
			        (unsigned long long)st_cut_pieces, (unsigned long long)st_pushes, st_bytes / 1e6, (unsigned long long)st_ml_parts, (unsigned long long)st_bam_parts,
			        params->homopolymer_compressed ? ", homopolymer-compressed (-hc) on the device" : "");
	}

	void GetTotal(uint64 &_n_reads)
	{
#ifdef KMC_HIP_S1_REFERENCE_FALLBACK
		if (ref) {
			ref->GetTotal(_n_reads);
			return;
		}
#endif
		_n_reads = n_reads;
	}
	~CWSplitter() {}
};

/* ---- the small-k worker (k <= 13, "Small k optimization on!": kmc.h:677-750, :767-862) ----
 * Drop-in for the reference's CWSmallKSplitter<uint64_t> (splitter.h:138-171, splitter.cpp:929-983): constructor (Params, Queues), operator()(), GetTotal,
 * GetResult, GetTotalKmers, Release, so that kmc.h:84, :799 and the reference's own small-k stage 2 (ProcessSmallKOptimization_Stage2 kmc.h:865-960,
 * CSmallKCompleter) build against it unchanged. The reference's class keeps its name and stays linkable (splitter.cpp instantiates it); this one has a name
 * of its own, and the #define at the end of this header points kmc.h at it.
 * With an engine that covers_small_k() the parts are counted where the engine counts them, into ONE table per device: the worker reserves and zeroes its own
 * table from pmm_small_k_buf exactly as the reference's does (stage 2 sums the tables of all n_splitters workers, kmc.h:872-885), pops parts, calls
 * smallk_part, frees each part and sums n_reads and n_kmers; the LAST worker to finish adds every device's table into its own, in chunks of 32 MB, and the
 * others hand over zeros. A part the engine answers KMC_SPLIT_UNCOVERED or an error for stops the run like a part of the bin worker does.
 * With any other engine (the oracle and emulated engines, a library without kmc_hip_smallk_*) — or one that lacks the job's format or -hc — the whole job
 * goes to the reference's CWSmallKSplitter, as it did before this worker existed. --opt-out-size and -e never get here (kmc.h:773-779). */
template <typename COUNTER_TYPE> using CWSmallKSplitter_ref = CWSmallKSplitter<COUNTER_TYPE>;

template <typename COUNTER_TYPE> class CWSmallKSplitter_dev {
	static_assert(sizeof(COUNTER_TYPE) == sizeof(uint64_t), "the engine's table has 64-bit counters (kmc.h:84 uses uint64_t)");
	CPartQueue *pq;
	CMemoryPool *pmm_fastq, *pmm_small_k;
	CKMCParams *params;
	CSmallKBuf<COUNTER_TYPE> small_k_buf;
	std::unique_ptr<CWSmallKSplitter_ref<COUNTER_TYPE>> ref; /* non-null: the reference's worker runs the whole job */
	std::unique_ptr<KmcSplitEngine> engine;
	uint64 n_reads = 0, total_kmers = 0;
	uint32 kmer_len;
	uint64 st_parts = 0;
	long long st_engine_ns = 0;

	static std::atomic<int> &finished_workers()
	{
		static std::atomic<int> finished{0};
		return finished;
	}
	void drain()
	{
		const uint64_t entries = (uint64_t)1 << (2 * kmer_len), chunk = (uint64_t)1 << 22; /* 32 MB of counters at a time */
		KmcTimeline::mark("splitter: small k, drain of the device tables starts");
		for (uint64_t at = 0; at < entries; at += chunk)
			if (int rc = engine->smallk_drain(at, entries - at < chunk ? entries - at : chunk, reinterpret_cast<uint64_t *>(small_k_buf.buf) + at)) {
				std::ostringstream ostr;
				ostr << "Error: stage-1 split engine failed to hand over the small-k table (code " << rc << "): " << engine->last_error();
				CCriticalErrorHandler::Inst().HandleCriticalError(ostr.str());
			}
		KmcTimeline::mark("splitter: small k, device tables merged");
	}

public:
	CWSmallKSplitter_dev(CKMCParams &Params, CKMCQueues &Queues)
	{
		pq = Queues.part_queue.get();
		pmm_fastq = Queues.pmm_fastq.get();
		pmm_small_k = Queues.pmm_small_k_buf.get();
		params = &Params;
		kmer_len = Params.kmer_len;
		small_k_buf.buf = nullptr;
		KmcSplitParams sp;
		sp.kmer_len = Params.kmer_len;
		sp.signature_len = Params.signature_len; /* may exceed kmer_len: not used on this path */
		sp.n_bins = Params.n_bins;
		sp.max_x = 0;
		sp.both_strands = Params.both_strands ? 1 : 0;
		sp.file_type = Params.file_type == InputType::FASTQ ? 1 : Params.file_type == InputType::MULTILINE_FASTA ? 2 : Params.file_type == InputType::BAM ? 4 : 0; /* KMC: 0 */
		sp.line_cap = (uint64_t)Params.mem_part_pmm_reads; /* (MAX_LINE_SIZE + 1) * 8 in this mode, kmc.h:689 */
		sp.sig_to_bin = nullptr;                           /* no signature mapper exists in this mode */
		sp.homopolymer_compressed = Params.homopolymer_compressed ? 1 : 0;
		static std::atomic<int> next_idx{0};
		engine.reset(kmc_make_split_engine(sp, next_idx++ % (int)Params.n_splitters, (int)Params.n_splitters));
		const bool covered = engine && engine->covers_small_k() && (Params.file_type != InputType::MULTILINE_FASTA || engine->covers_multiline_fasta()) &&
		                     (Params.file_type != InputType::BAM || engine->covers_bam()) && (!Params.homopolymer_compressed || engine->covers_homopolymer_compression());
		if (!covered) {
			engine.reset();
			ref = std::make_unique<CWSmallKSplitter_ref<COUNTER_TYPE>>(Params, Queues);
			return;
		}
		finished_workers() = 0; /* every worker is constructed before any can finish (kmc.h:797-801), as in CWSplitter above */
		if (int rc = engine->smallk_open()) {
			std::ostringstream ostr;
			ostr << "Error: stage-1 split engine could not open the small-k table (code " << rc << "): " << engine->last_error();
			CCriticalErrorHandler::Inst().HandleCriticalError(ostr.str());
		}
	}
	~CWSmallKSplitter_dev() {}

	void operator()()
	{
		if (ref) {
			(*ref)();
			return;
		}
		KmcTimeline::mark_first_last("splitter: first worker started", nullptr);
		pmm_small_k->reserve(small_k_buf.buf); /* splitter.cpp:954-955 */
		memset(small_k_buf.buf, 0, ((size_t)1 << (2 * kmer_len)) * sizeof(*small_k_buf.buf));
		while (!pq->completed()) {
			uchar *part;
			uint64 size;
			ReadType read_type;
			if (!pq->pop(part, size, read_type))
				continue;
			if (read_type == ReadType::na && params->file_type != InputType::MULTILINE_FASTA && params->file_type != InputType::BAM)
				CCriticalErrorHandler::Inst().HandleCriticalError("Error: stage 1 on the device got a part of ReadType::na");
			uint64_t part_reads = 0, part_kmers = 0;
			const auto t0 = std::chrono::steady_clock::now();
			const int rc = engine->smallk_part(part, size, read_type == ReadType::long_read, part_reads, part_kmers);
			st_engine_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
			if (rc == KMC_SPLIT_UNCOVERED)
				kmc_hip_s1_stop_uncovered_part(params->file_type, read_type);
			if (rc != 0) {
				std::ostringstream ostr;
				ostr << "Error: stage-1 split engine failed (code " << rc << "): " << engine->last_error();
				CCriticalErrorHandler::Inst().HandleCriticalError(ostr.str());
			}
			++st_parts;
			pmm_fastq->free(part);
			n_reads += part_reads;
			total_kmers += part_kmers;
		}
		if (++finished_workers() == (int)params->n_splitters)
			drain();
		engine.reset();
		KmcTimeline::mark_first_last(nullptr, "splitter: last worker done");
		if (getenv("KMC_HIP_VERBOSE"))
			fprintf(stderr, "[kmc_hip stage 1] worker: small k on the device: %llu parts, %llu k-mers (%.3f s inside the engine)%s\n", (unsigned long long)st_parts,
			        (unsigned long long)total_kmers, st_engine_ns * 1e-9, params->homopolymer_compressed ? ", homopolymer-compressed (-hc) on the device" : "");
	}

	void GetTotal(uint64 &_n_reads)
	{
		if (ref) {
			ref->GetTotal(_n_reads);
			return;
		}
		_n_reads = n_reads;
	}
	CSmallKBuf<COUNTER_TYPE> GetResult() { return ref ? ref->GetResult() : small_k_buf; }
	uint64 GetTotalKmers() { return ref ? ref->GetTotalKmers() : total_kmers; }
	void Release()
	{
		if (ref)
			ref->Release();
		else
			pmm_small_k->free(small_k_buf.buf);
	}
};
/* from here on (kmc.h is read after this header) the small-k worker of CKMC<SIZE> is the one above */
#define CWSmallKSplitter CWSmallKSplitter_dev

/* ---- the stage-0 worker (the signature statistics the signature -> bin map is built from: CKMC<SIZE>::buildSignatureMapping, kmc.h:974-1075) ----
 * Drop-in for the reference's CWStatsSplitter (splitter.h:118-131, splitter.cpp:878-925): constructor (Params, Queues), operator()(), GetStats(uint32 *), so that
 * kmc.h:1007-1054 builds against it unchanged and the reference's own CSignatureMapper::Init (s_mapper.h:141-235) runs on the result. The reference's class keeps
 * its name and stays linkable (splitter.cpp defines it); this one has a name of its own, and the #define below points kmc.h at it.
 * With an engine that covers_signature_stats() the parts of the stats queue are looked at where the engine does it, into ONE array per device (CSplitter::CalcStats
 * adds 1 + len - kmer_len per super-k-mer: the number of k-mer windows per signature): the worker reserves and zeroes its own array from pmm_stats as the
 * reference's does (kmc.h:438 sizes the pool for one per worker), pops parts, calls sigstats_part, steps the progress observer and frees each part; the LAST
 * worker to finish adds every device's array into its own and the others hand over zeros. A part the engine answers KMC_SPLIT_UNCOVERED or an error for stops
 * the run like a part of the bin worker does. With any other engine (the oracle and emulated engines, a library without kmc_hip_sigstats_*) — or one that lacks
 * the job's format or -hc — stage 0 goes to the reference's CWStatsSplitter, as it did before this worker existed. The small-k mode builds no map and never
 * constructs this worker. */
typedef CWStatsSplitter CWStatsSplitter_ref;

class CWStatsSplitter_dev {
	CStatsPartQueue *spq;
	CMemoryPool *pmm_fastq, *pmm_stats;
	CKMCParams *params;
	uint32 *stats = nullptr;
	uint32 signature_len;
	KMC::IProgressObserver *progressObserver;
	std::unique_ptr<CWStatsSplitter_ref> ref; /* non-null: the reference's worker runs stage 0 */
	std::unique_ptr<KmcSplitEngine> engine;
	uint64 st_parts = 0, st_kmers = 0;
	long long st_engine_ns = 0;

	static std::atomic<int> &finished_workers()
	{
		static std::atomic<int> finished{0};
		return finished;
	}
	void drain()
	{
		const uint64_t entries = ((uint64_t)1 << (2 * signature_len)) + 1, chunk = (uint64_t)1 << 23; /* 32 MB of counters at a time */
		KmcTimeline::mark("stage 0: drain of the device statistics starts");
		for (uint64_t at = 0; at < entries; at += chunk)
			if (int rc = engine->sigstats_drain(at, entries - at < chunk ? entries - at : chunk, stats + at)) {
				std::ostringstream ostr;
				ostr << "Error: stage-1 split engine failed to hand over the signature statistics (code " << rc << "): " << engine->last_error();
				CCriticalErrorHandler::Inst().HandleCriticalError(ostr.str());
			}
		KmcTimeline::mark("stage 0: device statistics merged");
	}

public:
	CWStatsSplitter_dev(CKMCParams &Params, CKMCQueues &Queues)
	{
		spq = Queues.stats_part_queue.get();
		pmm_fastq = Queues.pmm_fastq.get();
		pmm_stats = Queues.pmm_stats.get();
		params = &Params;
		progressObserver = Params.progressObserver;
		signature_len = Params.signature_len;
		KmcSplitParams sp;
		sp.kmer_len = Params.kmer_len;
		sp.signature_len = Params.signature_len;
		sp.n_bins = Params.n_bins;
		sp.max_x = 0;
		sp.both_strands = Params.both_strands ? 1 : 0;
		sp.file_type = Params.file_type == InputType::FASTQ ? 1 : Params.file_type == InputType::MULTILINE_FASTA ? 2 : Params.file_type == InputType::BAM ? 4 : 0;
		sp.line_cap = (uint64_t)Params.mem_part_pmm_reads;
		sp.sig_to_bin = nullptr; /* the map is what this stage is for */
		sp.homopolymer_compressed = Params.homopolymer_compressed ? 1 : 0;
		static std::atomic<int> next_idx{0};
		engine.reset(kmc_make_split_engine(sp, next_idx++ % (int)Params.n_splitters, (int)Params.n_splitters));
		const bool covered = engine && engine->covers_signature_stats() && (Params.file_type != InputType::MULTILINE_FASTA || engine->covers_multiline_fasta()) &&
		                     (Params.file_type != InputType::BAM || engine->covers_bam()) && (!Params.homopolymer_compressed || engine->covers_homopolymer_compression());
		if (!covered) {
			engine.reset();
			ref = std::make_unique<CWStatsSplitter_ref>(Params, Queues); /* reserves its own array */
			return;
		}
		pmm_stats->reserve(stats); /* splitter.cpp:887-888 */
		std::fill_n(stats, ((size_t)1 << (2 * signature_len)) + 1, 0u);
		finished_workers() = 0; /* every worker is constructed before any can finish (kmc.h:1009-1013), as in CWSplitter above */
		if (int rc = engine->sigstats_open()) {
			std::ostringstream ostr;
			ostr << "Error: stage-1 split engine could not open the signature statistics (code " << rc << "): " << engine->last_error();
			CCriticalErrorHandler::Inst().HandleCriticalError(ostr.str());
		}
	}
	~CWStatsSplitter_dev()
	{
		if (stats)
			pmm_stats->free(stats);
	}

	void operator()()
	{
		if (ref) {
			(*ref)();
			return;
		}
		KmcTimeline::mark_first_last("stage 0: first worker started", nullptr);
		while (!spq->completed()) {
			uchar *part;
			uint64 size;
			ReadType read_type;
			if (!spq->pop(part, size, read_type))
				continue;
			if (read_type == ReadType::na && params->file_type != InputType::MULTILINE_FASTA && params->file_type != InputType::BAM)
				CCriticalErrorHandler::Inst().HandleCriticalError("Error: stage 0 on the device got a part of ReadType::na");
			uint64_t part_reads = 0, part_kmers = 0;
			const auto t0 = std::chrono::steady_clock::now();
			const int rc = engine->sigstats_part(part, size, read_type == ReadType::long_read, part_reads, part_kmers);
			st_engine_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
			if (rc == KMC_SPLIT_UNCOVERED)
				kmc_hip_s1_stop_uncovered_part(params->file_type, read_type);
			if (rc != 0) {
				std::ostringstream ostr;
				ostr << "Error: stage-1 split engine failed in stage 0 (code " << rc << "): " << engine->last_error();
				CCriticalErrorHandler::Inst().HandleCriticalError(ostr.str());
			}
			++st_parts;
			st_kmers += part_kmers;
			progressObserver->Step();
			pmm_fastq->free(part);
		}
		if (++finished_workers() == (int)params->n_splitters)
			drain();
		engine.reset();
		KmcTimeline::mark_first_last(nullptr, "stage 0: last worker done");
		if (getenv("KMC_HIP_VERBOSE"))
			fprintf(stderr, "[kmc_hip stage 0] worker: signature statistics on the device: %llu parts, %llu k-mers (%.3f s inside the engine)%s\n", (unsigned long long)st_parts,
			        (unsigned long long)st_kmers, st_engine_ns * 1e-9, params->homopolymer_compressed ? ", homopolymer-compressed (-hc) on the device" : "");
	}

	void GetStats(uint32 *_stats)
	{
		if (ref) {
			ref->GetStats(_stats);
			return;
		}
		const uint32 size = (1u << (signature_len * 2)) + 1;
		for (uint32 i = 0; i < size; ++i)
			_stats[i] += stats[i];
	}
};
/* from here on the stage-0 worker of CKMC<SIZE> is the one above */
#define CWStatsSplitter CWStatsSplitter_dev

#endif
