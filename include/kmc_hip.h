/*
 * include/kmc_hip.h — C-ABI of libkmc_hip.so: KMC stage-2 "bin sort & count" on MI355X (gfx950).
 *
 * This is the drop-in boundary. Plain C: pointers + sizes, no C++/torch types.
 * Every entry point names the reference interface it replaces (paths relative to the KMC 3.2.4
 * tree, /root/reference). The C++ worker that binds these inside kmc_core is
 * kmc_amd/host/kb_sorter_plugin.h; INTEGRATION.md shows the maintainer-side change.
 *
 * Conventions
 *   - return 0 on success, a negative KMC_HIP_E* code on failure; never throws, never aborts.
 *     kmc_hip_last_error(ctx) gives the message (the worker forwards it to
 *     CCriticalErrorHandler::HandleCriticalError, critical_error_handler.h:9-90).
 *   - `dev` is an index into the device list given to kmc_hip_init (not a HIP ordinal).
 *   - host threads may call concurrently as long as each uses its own (dev, slot) pair (mirrors one
 *     CWKmerBinSorter thread per sorter, kmc.h:1576-1584); calls on one pair must be serialised by the caller.
 *   - host buffers belong to the caller; device memory, streams and events belong to the library.
 *   - records are CKmer<SIZE> PODs (kmer.h:22-67): `words` x uint64, word 0 least significant.
 */
#ifndef KMC_HIP_H
#define KMC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMC_HIP_ABI_VERSION 4 /* 3: + kmc_hip_process_bins_submit/_wait (bound by the worker's loader), kmc_hip_process_bin_multi, kmc_hip_order_database_device;
                               * 4: kmc_hip_split_params.part_kind (long-read parts); symbols added since keep it: kmc_hip_db_set_op_device, kmc_hip_db_query_reads_device,
                               * kmc_hip_db_expr_device, kmc_hip_count_* */

enum {
	KMC_HIP_OK = 0,
	KMC_HIP_EINVAL = -1,   /* bad argument / unsupported parameter combination */
	KMC_HIP_EDEVICE = -2,  /* HIP runtime error (message has the hipError string) */
	KMC_HIP_ENOMEM = -3,   /* device or pinned-host allocation failed */
	KMC_HIP_ECORRUPT = -4, /* super-k-mer stream is ragged or disagrees with n_rec / pack sizes */
	KMC_HIP_ECAPACITY = -5,/* out_capacity too small for the counted k-mers */
	KMC_HIP_EINTERNAL = -6 /* device-side watchdog tripped (look-back spin bound) */
};

typedef struct kmc_hip_ctx kmc_hip_ctx;

/* Per-run constants the reference sorter copies out of CKMCParams (kb_sorter.h:165-200). */
typedef struct kmc_hip_bin_params {
	uint32_t kmer_len;       /* Params.kmer_len, 1..256 */
	uint32_t both_strands;   /* Params.both_strands: 1 = canonical k-mers */
	uint32_t cutoff_min;     /* Params.cutoff_min */
	uint32_t without_output; /* Params.without_output: tallies only, out_bytes = 0, lut untouched */
	uint64_t cutoff_max;     /* Params.cutoff_max (compared as uint32, kb_sorter.h:186) */
	uint64_t counter_max;    /* Params.counter_max */
	uint32_t lut_prefix_len; /* Params.lut_prefix_len (kmc.h:1434-1469); 0 for KFF */
	uint32_t output_type;    /* 0 = OutputType::KMC, 1 = OutputType::KFF (kb_sorter.h:1043-1049) */
} kmc_hip_bin_params;

/* stats[] order == the four tallies of CKmerQueue::push (queues.h:826, kb_sorter.h:1273) */
enum { KMC_HIP_STAT_UNIQUE = 0, KMC_HIP_STAT_CUTOFF_MIN = 1, KMC_HIP_STAT_CUTOFF_MAX = 2, KMC_HIP_STAT_TOTAL = 3 };

/* ---- lifetime ----------------------------------------------------------------------------- */

/* Create a context on `n_dev` HIP devices (ordinals in device_ids; NULL => {0..n_dev-1}).
 * Replaces: construction of CWKmerBinSorter<SIZE> workers + pmm_radix_buf pool (kmc.h:1510,1576-1584). */
int kmc_hip_init(const int *device_ids, int n_dev, kmc_hip_ctx **out);
void kmc_hip_destroy(kmc_hip_ctx *ctx);
const char *kmc_hip_last_error(kmc_hip_ctx *ctx); /* thread-local message of the calling thread's last failure */
int kmc_hip_abi_version(void);
/* 0 = HIP on a GPU (the product). Test builds say otherwise — 1: this library's source over the CPU emulation of tests/hipemu, 2: the mock of
 * tests/hipemu/mock_hip_lib.cpp — so that whatever measures or certifies (bench.py, __graft_entry__.smoke) can refuse them. */
int kmc_hip_backend_kind(void);
int kmc_hip_num_devices(kmc_hip_ctx *ctx);
int kmc_hip_device_count(void); /* HIP devices visible to the process (0 when the runtime is unusable) */
int kmc_hip_num_slots(void); /* stream slots per device usable with _submit/_wait (independent bins in flight) */

/* Derived sizes, so callers size buffers exactly like kb_reader.h:141-165 does. */
uint32_t kmc_hip_words(uint32_t kmer_len);                                   /* SIZE = ceil(k/32) */
uint32_t kmc_hip_counter_size(uint64_t cutoff_max, uint64_t counter_max);    /* defs.h:154-159 */
uint32_t kmc_hip_out_rec_bytes(const kmc_hip_bin_params *p);                 /* suffix bytes + counter bytes */
uint64_t kmc_hip_lut_entries(const kmc_hip_bin_params *p);                   /* 4^p, 0 when p == 0 */

/* ---- narrow boundary: the sort alone ------------------------------------------------------- */

/* Ascending sort of n records of `words` uint64 by their low `key_bytes` bytes (higher bytes must be
 * zero), result left IN `recs` (host memory).
 * Replaces: SortFunction<CKmer<SIZE>> (raduls.h:19-20) = RadulsSort::RadixSortMSD_* (raduls_impl.h:769-776)
 * / RadixSort::RadixSortMSD (radix.h:845-852) as called at kb_sorter.h:775; key_bytes = rec_len there.
 * (The reference leaves the result in `tmp` when rec_len is odd; this entry always returns it in place — see _into.) */
int kmc_hip_sort_records(kmc_hip_ctx *ctx, int dev, void *recs, uint64_t n, uint32_t words, uint32_t key_bytes);

/* Same, with the sorted records delivered to `dst` (host memory; may equal recs). This is what the SortFunction adapter
 * (kmc_amd/host/hip_sort_function.h) binds: the reference wants the result in `tmp` when key_bytes is odd and in `kmers`
 * when it is even (kb_sorter.h:776-779, raduls_impl.h:552-561), so the adapter passes dst = tmp or kmers. */
int kmc_hip_sort_records_into(kmc_hip_ctx *ctx, int dev, const void *recs, void *dst, uint64_t n, uint32_t words, uint32_t key_bytes);

/* Same, on device-resident records (d_recs, d_tmp: n*words*8 bytes each, 256-B aligned). On return
 * *d_result points at whichever of the two holds the sorted records. Stream-synchronous. */
int kmc_hip_sort_records_device(kmc_hip_ctx *ctx, int dev, void *d_recs, void *d_tmp, uint64_t n, uint32_t words,
                                uint32_t key_bytes, void **d_result);

/* ---- full boundary: one bin, super-k-mer bytes in -> (suffix,count) records + LUT + tallies out --- */

/* Replaces: one iteration of CKmerBinSorter<SIZE>::ProcessBins (kb_sorter.h:210-237) = Expand (:728-752)
 * + Sort (:757-780) + Compact (:1287; CompactKmers :1128-1281 / CompactKxmers :937-1122), i.e. everything
 * between sorters_manager->GetNext (queues.h:2087) and kq->push (queues.h:826).
 *   superkmers/size : the bin image CKmerBinReader read (kb_reader.h:176-190); format kb_collector.cpp:57-71
 *   n_rec           : CBinDesc n_rec of the bin (number of k-mers)
 *   pack_bytes/n_packs : byte length of each expander pack, in order (CExpanderPackDesc::pop, queues.h:390;
 *                     first member of each pair). n_packs == 0 => the library finds pack boundaries itself.
 *   out_suffix/out_capacity : the bin's mba_suffix slot; capacity as kb_reader.h:141-150
 *   out_bytes       : bytes written = the single data pack [0, out_bytes) pushed to kq
 *   lut             : the bin's mba_lut slot, kmc_hip_lut_entries() uint64, per-bin COUNTS (the completer makes
 *                     them cumulative, kb_completer.cpp:193-199); zero-filled by the callee
 *   stats           : {n_unique, n_cutoff_min, n_cutoff_max, n_total}
 * out_suffix / lut MAY alias superkmers (they do in the reference arena when rec_len is even,
 * queues.h:1352-1369): all input is on the device before the first output byte is written.
 * Empty bins (size == 0, n_rec == 0) are valid and produce zeros. */
int kmc_hip_process_bin(kmc_hip_ctx *ctx, int dev, const kmc_hip_bin_params *params, const uint8_t *superkmers,
                        uint64_t size, uint64_t n_rec, const uint64_t *pack_bytes, uint64_t n_packs,
                        uint8_t *out_suffix, uint64_t out_capacity, uint64_t *out_bytes, uint64_t *lut,
                        uint64_t stats[4]);

/* Several bins per call through the same boundary: the host-side twin of kmc_hip_process_bins_device's grouping. The n_bins (1..16) bins are
 * uploaded together and — as far as the spare bits of the top radix digit can tag them (4 bins at k = 27, 55, 127; see kmc_hip_process_bins_device) —
 * SORTED TOGETHER: launches 4x as large and 4x fewer, which is worth ~10 % at 48 M k-mers per bin and several x on small bins. A worker that finds
 * more than one bin waiting (CBinQueue::pop_if_any, queues.h:751) hands them over in one call; every bin keeps its own buffers and gets its own
 * out_bytes / tallies, the bytes are those of n_bins separate kmc_hip_process_bin calls. _wait: out_bytes[n_bins], stats[n_bins][4], in the order of
 * the descriptors. An error in any bin fails the call (the device error word belongs to the stream). Host buffers must stay valid until _wait returns.
 * Replaces: n_bins iterations of CKmerBinSorter<SIZE>::ProcessBins (kb_sorter.h:210-237). */
typedef struct kmc_hip_host_bin {
	const uint8_t *superkmers;
	uint64_t size, n_rec;
	const uint64_t *pack_bytes;
	uint64_t n_packs;
	uint8_t *out_suffix;
	uint64_t out_capacity;
	uint64_t *lut;
} kmc_hip_host_bin;
int kmc_hip_process_bins_submit(kmc_hip_ctx *ctx, int dev, int slot, const kmc_hip_bin_params *params, const kmc_hip_host_bin *bins, uint32_t n_bins);
int kmc_hip_process_bins_wait(kmc_hip_ctx *ctx, int dev, int slot, uint64_t *out_bytes, uint64_t *stats);

/* The same bin over ALL devices of the context: the oversized-bin path.
 * Replaces: strict-memory mode's treatment of a bin that does not fit — the reference cuts it into sub-bins by the k-mers' leading symbols, sorts
 * them one after the other through the same sort_func and merges (kmc.h:1607-1692, bkb_sorter.h:187, bkb_subbin.h / bkb_merger.h). Here the cut goes
 * across GPUs: every device expands a share of the expander packs, the records are exchanged by the TOP byte of the key (one all-to-all: RCCL
 * ncclSend/ncclRecv over xGMI between distinct GPUs, peer copies when the context names one GPU more than once), every device sorts and compacts the
 * k-mers of its key range, and the ranges are emitted in order. Arguments, outputs and errors as kmc_hip_process_bin; the result is byte-identical to
 * that call's. Synchronous; takes the first stream slot of every device. */
int kmc_hip_process_bin_multi(kmc_hip_ctx *ctx, const kmc_hip_bin_params *params, const uint8_t *superkmers, uint64_t size, uint64_t n_rec,
                              const uint64_t *pack_bytes, uint64_t n_packs, uint8_t *out_suffix, uint64_t out_capacity, uint64_t *out_bytes,
                              uint64_t *lut, uint64_t stats[4]);

/* Asynchronous pair for double buffering: _submit enqueues H2D + kernels + D2H on the device's stream slot
 * `slot` (0 .. kmc_hip_num_slots()-1) and returns; _wait blocks until that slot's bin is complete and fills out_bytes/stats.
 * Host buffers must stay valid (and out must not alias in) until _wait returns. */
int kmc_hip_process_bin_submit(kmc_hip_ctx *ctx, int dev, int slot, const kmc_hip_bin_params *params,
                               const uint8_t *superkmers, uint64_t size, uint64_t n_rec, const uint64_t *pack_bytes,
                               uint64_t n_packs, uint8_t *out_suffix, uint64_t out_capacity, uint64_t *lut);
int kmc_hip_process_bin_wait(kmc_hip_ctx *ctx, int dev, int slot, uint64_t *out_bytes, uint64_t stats[4]);

/* Device-resident variant (inputs already in HBM; used by bench.py so the timed region excludes PCIe, and by
 * callers that produce bins on the GPU). All d_* pointers are device memory on `dev`:
 *   d_superkmers[size (+16 B readable slack)], d_pack_start[n_packs+1] = byte offsets of pack starts, last = size
 *   d_out[out_capacity], d_lut[kmc_hip_lut_entries()], d_stats[4] (uint64, written by the device)
 *   d_out_bytes: 1 uint64 written by the device.
 * Returns after enqueueing unless `sync` != 0. Asynchronous calls are spread round-robin over several internal streams
 * (bins are independent), so consecutive small bins overlap (a bin with more than 2 GiB of record arrays always takes
 * the first stream: it fills the GPU alone); kmc_hip_synchronize(dev) waits for all of them and reports any deferred
 * device error (errors are kept in a per-stream sticky word that only a synchronising call clears). Output buffers of calls in flight must be distinct. */
int kmc_hip_process_bin_device(kmc_hip_ctx *ctx, int dev, const kmc_hip_bin_params *params,
                               const uint8_t *d_superkmers, uint64_t size, uint64_t n_rec,
                               const uint64_t *d_pack_start, uint64_t n_packs, uint8_t *d_out, uint64_t out_capacity,
                               uint64_t *d_out_bytes, uint64_t *d_lut, uint64_t *d_stats, int sync);

/* Many device-resident bins in one call (per-GPU bin queue): bin i is enqueued on internal stream
 * (i mod n_streams), in index order per stream, by one host thread per stream — a group of bins is 13-14 launches, so hundreds of
 * small bins are bound by the host's launch rate unless several threads submit (KMC's default is 512 bins per run,
 * kmc.h n_bins). n_streams <= 0 picks the default (8), capped at kmc_hip_num_slots(). Returns after enqueueing;
 * kmc_hip_synchronize(dev) waits and reports deferred device errors. Output buffers of all bins must be distinct.
 * Consecutive bins of a stream are SORTED TOGETHER when the top radix digit has spare bits (8 ceil(k/4) - 2k of them: groups of 4 at
 * k = 27, 55, 127): the bin's number inside the group is kept in those bits while the records are on the device, so one set of passes
 * orders the group bin-major; front end and compaction stay per bin. $KMC_HIP_GROUP caps the group size (1 = every bin on its own).
 * Replaces: the hand-out of bins to n_sorters CWKmerBinSorter threads (kmc.h:1576-1584, queues.h:2087-2128). */
typedef struct kmc_hip_bin_desc {
	const uint8_t *d_superkmers;
	uint64_t size, n_rec;
	const uint64_t *d_pack_start;
	uint64_t n_packs;
	uint8_t *d_out;
	uint64_t out_capacity;
	uint64_t *d_out_bytes, *d_lut, *d_stats;
} kmc_hip_bin_desc;
int kmc_hip_process_bins_device(kmc_hip_ctx *ctx, int dev, const kmc_hip_bin_params *params, const kmc_hip_bin_desc *bins,
                                uint64_t n_bins, int n_streams);

/* ---- a globally ordered database ---------------------------------------------
 * The bins of a run — as kmc_hip_process_bin[s]_device left them: per bin `d_out` (suffix records, ascending inside the bin), `d_out_bytes`, `d_lut`
 * (records per lut_prefix_len-symbol prefix) — merged into ONE ascending sequence of all counted k-mers: records of (kmer_len - out_lut_prefix_len) / 4
 * suffix bytes (most significant first) + counter bytes (least significant first) into d_out, and into d_lut_out[4^out_lut_prefix_len] the number of
 * records with a prefix BELOW each entry — the body of the database `kmc_tools transform <db> sort <out>` writes (kmc_tools/kmc1_db_writer.h:368-395;
 * the header and the 'KMCP'/'KMCS' markers around it are the caller's, :309-370). Every k-mer is in exactly one bin (bins partition by signature), so
 * this is a sort, not a merge of counts: records unpacked to (k-mer, count), ordered by the library's LSD passes, packed again. Synchronous; *n_kmers =
 * records written. params: the parameters the bins were made with (KMC output, lut_prefix_len > 0); kmer_len <= 224.
 * Replaces: kmc_tools' sort operation on the CPU (CKMC1DbWriter fed by a priority queue over the bins). */
int kmc_hip_order_database_device(kmc_hip_ctx *ctx, int dev, const kmc_hip_bin_params *params, const kmc_hip_bin_desc *bins, uint64_t n_bins,
                                  uint32_t out_lut_prefix_len, uint8_t *d_out, uint64_t out_capacity, uint64_t *d_lut_out, uint64_t *n_kmers);

/* ---- set operations between two ordered databases --------------------------------------------------
 * `kmc_tools simple <db1> <db2> <operation> <out>` on the device. Each input is a database BODY as kmc_hip_order_database_device leaves it and kmc_tools writes
 * it (KMC1): n_recs ascending records of (kmer_len - lut_prefix_len) / 4 suffix bytes (most significant first) + counter_size counter bytes (least significant
 * first), and a LUT of 4^lut_prefix_len uint64 where entry i is the number of records with a prefix below i. The inputs share kmer_len (<= 224) and may differ in
 * lut_prefix_len and counter_size. A record whose count lies outside its input's [cutoff_min, cutoff_max] is treated as absent, as the reference's readers do
 * (kmc_tools/kmc1_db_reader.h:574-576,618). The two sequences are merged; every k-mer is only in A, only in B, or in both, and
 *   INTERSECT keeps the pairs, UNION everything, KMERS_SUBTRACT what is only in A, COUNTERS_SUBTRACT what is only in A and the pairs, and the REVERSE_ operations
 *   the same with the inputs' roles swapped (operations.h:317-322);
 *   a pair's count is counter_op(count in A, count in B) in 32-bit unsigned arithmetic — SUM wraps, DIFF is 0 when the left count is not larger — with the counts
 *   swapped for REVERSE_COUNTERS_SUBTRACT (operations.h:337-340, bundle.h:257-278); the two KMERS_SUBTRACT operations ignore counter_op;
 *   then the writer's rule (kmc1_db_writer.h:382-385): a count below the output's cutoff_min (>= 1) or above its cutoff_max is dropped, what is left is clamped to
 *   counter_max (>= 1).
 * d_out receives the kept records in ascending order, packed for out_lut_prefix_len and a counter of MIN(BYTE_LOG(counter_max), BYTE_LOG(cutoff_max)) bytes
 * (kmc1_db_writer.h:154; that is kmc_hip_counter_size(cutoff_max, counter_max), except that counter_max == 1 still stores one byte here), d_lut_out the LUT of
 * 4^out_lut_prefix_len entries. out_capacity (bytes) must hold the operation's upper bound: the records of both inputs for UNION, of the smaller input for
 * INTERSECT, of A for the two SUBTRACT operations, of B for the two REVERSE_ ones — KMC_HIP_ECAPACITY otherwise. KMC_HIP_EINVAL: a NULL argument, a counter_size
 * outside 1..4, a lut_prefix_len with (kmer_len - lut_prefix_len) % 4 != 0; KMC_HIP_ECORRUPT: a LUT whose last entry exceeds n_recs. Either input may be empty
 * (d_recs may then be NULL). Synchronous. *n_kmers = records written = stats[KMC_HIP_DB_STAT_WRITTEN]; the header and the markers around the body are the caller's
 * (kmc_amd/dbio.py writes them).
 * Replaces: CSimpleOperation<SIZE>::process_impl (kmc_tools/operations.h:298-491), a single-threaded two-pointer merge, feeding CKMC1DbWriter<SIZE>::add_kmer
 * (kmc1_db_writer.h:375-404). */
enum { KMC_HIP_DB_INTERSECT = 0, KMC_HIP_DB_UNION = 1, KMC_HIP_DB_KMERS_SUBTRACT = 2, KMC_HIP_DB_COUNTERS_SUBTRACT = 3, KMC_HIP_DB_REVERSE_KMERS_SUBTRACT = 4,
       KMC_HIP_DB_REVERSE_COUNTERS_SUBTRACT = 5 };
enum { KMC_HIP_DB_CNT_MIN = 0, KMC_HIP_DB_CNT_MAX = 1, KMC_HIP_DB_CNT_SUM = 2, KMC_HIP_DB_CNT_DIFF = 3, KMC_HIP_DB_CNT_LEFT = 4, KMC_HIP_DB_CNT_RIGHT = 5 };
/* stats[]: k-mers in both inputs / only in A / only in B (after the inputs' cutoffs), candidates the output's cutoff_min / cutoff_max dropped, records written */
enum { KMC_HIP_DB_STAT_PAIRS = 0, KMC_HIP_DB_STAT_ONLY_A = 1, KMC_HIP_DB_STAT_ONLY_B = 2, KMC_HIP_DB_STAT_BELOW_MIN = 3, KMC_HIP_DB_STAT_ABOVE_MAX = 4, KMC_HIP_DB_STAT_WRITTEN = 5 };
typedef struct kmc_hip_db_view { /* one input: a KMC1 body on the device */
	const uint8_t *d_recs;
	uint64_t n_recs;
	const uint64_t *d_lut;
	uint32_t lut_prefix_len, counter_size; /* counter_size 1..4; 0 is KMC_HIP_EINVAL */
	uint32_t cutoff_min;
	uint64_t cutoff_max; /* the input's -ci / -cx */
} kmc_hip_db_view;
typedef struct kmc_hip_db_op {
	uint32_t op;         /* KMC_HIP_DB_INTERSECT .. KMC_HIP_DB_REVERSE_COUNTERS_SUBTRACT */
	uint32_t counter_op; /* KMC_HIP_DB_CNT_MIN .. _RIGHT (ignored by the two kmers_subtract operations) */
	uint32_t cutoff_min, counter_max;
	uint64_t cutoff_max; /* of the output */
	uint32_t out_lut_prefix_len;
} kmc_hip_db_op;
int kmc_hip_db_set_op_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *a, const kmc_hip_db_view *b, const kmc_hip_db_op *op, uint8_t *d_out,
                             uint64_t out_capacity, uint64_t *d_lut_out, uint64_t *n_kmers, uint64_t stats[6]);

/* ---- reads against an ordered database -----------------------------------------------------------
 * `kmc_tools filter <db> <reads> <out>` on the device: for every window of kmer_len symbols of every read, the counter the database holds for it. `db` is a database
 * body as above (its [cutoff_min, cutoff_max]: the database's -ci / -cx; counter_size 1..4), kmer_len <= 224. d_seq[n_bytes] holds the reads' sequence lines as they
 * are in the file, every read followed by ONE terminator byte ('\n'): read r is d_seq[d_read_off[r] .. d_read_off[r + 1] - 1), d_read_off has n_reads + 1 ascending
 * entries and the last one is at most n_bytes. Symbols are classified as CKmerAPI::num_codes does (kmc_api/kmer_api.h:268-275): ACGTacgt are 0..3, every other byte —
 * the terminator too — is invalid, so no window reaches from one read into the next.
 *   d_counters[i], i < n_bytes (required): the counter of the k-mer that starts at byte i — with both_strands the smaller of it and its reverse complement
 *     (kmc_file.cpp:998-1001), found by a binary search of the suffix records under the bounds of its LUT prefix (kmc_file.cpp:905-925,1321-1399) — if that counter lies
 *     in [cutoff_min, cutoff_max]; 0 if the k-mer is absent, cut, the window holds an invalid symbol, or i > n_bytes - kmer_len. Every entry is written.
 *   d_n_valid[r] (or NULL): the non-zero counters among the read's max(len - kmer_len + 1, 0) windows (fastq_filter.cpp:111-115).
 *   d_trim_len[r] (or NULL): 0 if len < kmer_len or the first window's counter is below `threshold`; otherwise kmer_len - 1 + j, j the first window >= 1 whose counter
 *     is below `threshold`, or the number of windows (fastq_filter.cpp:134-152; there a read shorter than kmer_len reads an empty vector).
 *   d_masked[n_bytes] (or NULL): d_seq with every base of a read replaced by 'N' that lies in a window of that read whose counter is below `threshold`
 *     (fastq_filter.cpp:153-176); reads shorter than kmer_len, terminators and bytes outside every read are copied.
 *   stats[0..3]: windows without an invalid symbol; of those, found with a counter inside the cutoffs; found but cut by the cutoffs; windows with an invalid symbol —
 *     the last counted over the n_bytes - kmer_len + 1 window starts of d_seq, terminators included.
 * A read must be shorter than 2^32 symbols. Synchronous. An empty database, n_bytes < kmer_len and n_reads == 0 are legal (every counter 0; without reads d_masked is a copy).
 * KMC_HIP_EINVAL: a NULL argument (d_read_off may be NULL only when n_reads is 0 and none of d_n_valid, d_trim_len, d_masked is given), a counter_size outside 1..4,
 * a lut_prefix_len with (kmer_len - lut_prefix_len) % 4 != 0, kmer_len > 224; KMC_HIP_ECORRUPT: a LUT whose last entry exceeds n_recs, read offsets that do not ascend
 * or end behind n_bytes, a read whose terminator is a valid symbol (the outputs are then undefined, nothing outside them is touched).
 * Replaces: CKMCFile::GetCountersForRead (kmc_api/kmc_file.cpp:873-1027) per read and the three rules of CFastqFilter (kmc_tools/fastq_filter.cpp:106-176), one
 * thread per input part there. */
enum { KMC_HIP_DBQ_STAT_VALID = 0, KMC_HIP_DBQ_STAT_FOUND = 1, KMC_HIP_DBQ_STAT_CUT = 2, KMC_HIP_DBQ_STAT_INVALID = 3 };
int kmc_hip_db_query_reads_device(kmc_hip_ctx *ctx, int dev, const kmc_hip_db_view *db, uint32_t kmer_len, uint32_t both_strands, const uint8_t *d_seq, uint64_t n_bytes,
                                  const uint64_t *d_read_off, uint64_t n_reads, uint32_t threshold, uint32_t *d_counters /* [n_bytes], required */,
                                  uint32_t *d_n_valid /* [n_reads] or NULL */, uint32_t *d_trim_len /* [n_reads] or NULL */, uint8_t *d_masked /* [n_bytes] or NULL */,
                                  uint64_t stats[4]);

/* ---- one database transformed -----------------------------------------------------------------------
 * `kmc_tools transform <db> reduce | compact | set_counts | sort | histogram | dump` on the device (kmc_tools/kmc_tools.cpp:41-137,415-484; the command line and its
 * defaults: parameters_parser.cpp:272-453,842-892). `db` is a database body as above, kmer_len - lut_prefix_len a positive multiple of 4, counter_size 1..4. A record whose
 * counter lies outside the view's [cutoff_min, cutoff_max] — the input's -ci / -cx — is absent for every output (kmc1_db_reader.h:574-576,618, kmc2_db_reader.h:1812,1897)
 * and counted in stats[KMC_HIP_DBT_STAT_CUT_IN]. All three are synchronous; an empty database is legal (d_recs may then be NULL). KMC_HIP_EINVAL: a NULL argument, a
 * counter_size outside 1..4, a lut_prefix_len that is not as above, an output's cutoff_min or counter_max below 1; KMC_HIP_ECORRUPT: a LUT whose last entry exceeds n_recs.
 *
 * _reduce: the database outputs. db is ORDERED (a KMC1 body; kmer_len <= 224). The writer's rule (kmc1_db_writer.h:375-404): with counter_value != 0 (set_counts) every
 *   present record is written with that count; otherwise a count below cutoff_min or above cutoff_max is dropped and what is left is clamped to counter_max. reduce, compact
 *   (counter_max 1) and sort of a body that is already ordered are this rule with the command line's numbers. d_out receives the kept records in their order, packed for
 *   out_lut_prefix_len and a counter of MIN(BYTE_LOG(counter_max), BYTE_LOG(cutoff_max)) bytes — BYTE_LOG(counter_value) for set_counts — (kmc1_db_writer.h:154-156),
 *   d_lut_out the LUT of 4^out_lut_prefix_len entries, as kmc_hip_db_set_op_device leaves them. out_capacity (bytes) must hold n_recs records: KMC_HIP_ECAPACITY otherwise.
 *   *n_kmers = records written = stats[KMC_HIP_DBT_STAT_WRITTEN]; stats[1], [2]: present records the output's cutoff_min / cutoff_max dropped.
 *   Replaces: CKMC1DbWriter<SIZE>::add_kmer fed record by record from the loop of CTools::ProcessTransformOper (kmc_tools.cpp:93-115).
 * _histogram: d_hist[cutoff_max - cutoff_min + 1] (uint64, every entry written): entry i = present records whose counter is cutoff_min + i, no clamp
 *   (histogram_writer.h:32-36; the text `i\tcount\n` is the caller's, :45-48). The records need not be ordered: the counters are read straight from the packed records.
 *   n_lut_segments (>= 1) says how long the LUT is, as for _dump; counting does not read it beyond the check of its end. KMC_HIP_EINVAL also for cutoff_max < cutoff_min or
 *   >= 2^32. stats[3]: cut by the input, present but outside [cutoff_min, cutoff_max], counted.
 *   Replaces: CHistogramWriterForTransform::PutCounter per record (kmc_tools.cpp:75-92).
 * _dump: records [first, first + count) of the body as text into d_text, per record kept `<kmer_len symbols ACGT>\t<decimal counter>\n` (dump_writer.h:111-160): kept
 *   if cutoff_min <= counter <= cutoff_max, then clamped to counter_max; in record order. n_lut_segments: 1 for an ordered body (a LUT of 4^lut_prefix_len entries); for a
 *   body as `kmc` wrote it (KMC2: records ordered inside every bin, the bins one after the other) the number of bins — the LUT is then the file's: n_lut_segments x
 *   4^lut_prefix_len global record offsets and ONE closing entry (= n_recs) behind them, and a record's prefix is the index of the last entry <= its number, modulo
 *   4^lut_prefix_len (kmc2_db_reader.h:1776-1791) — so a KMC2 database is dumped in file order without ordering it. A record takes at most kmer_len + 12 bytes:
 *   text_capacity < count x (kmer_len + 12) is KMC_HIP_ECAPACITY. *n_bytes = bytes written; no byte of d_text outside [0, *n_bytes) is touched. count == 0 is legal;
 *   first + count > n_recs is KMC_HIP_EINVAL. stats[4]: cut by the input, below cutoff_min, above cutoff_max, records written — of the range.
 *   $KMC_HIP_DUMP_TILE: records per workgroup (default: 32 KiB of text).
 *   Replaces: CDumpWriterForTransform<SIZE>::PutKmer per record (kmc_tools.cpp:83-103), one thread. */
enum { KMC_HIP_DBT_STAT_CUT_IN = 0, KMC_HIP_DBT_STAT_BELOW_MIN = 1, KMC_HIP_DBT_STAT_ABOVE_MAX = 2, KMC_HIP_DBT_STAT_WRITTEN = 3 };
enum { KMC_HIP_DBH_STAT_CUT_IN = 0, KMC_HIP_DBH_STAT_OUTSIDE = 1, KMC_HIP_DBH_STAT_COUNTED = 2 };
int kmc_hip_db_reduce_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *db, uint32_t cutoff_min, uint64_t cutoff_max, uint32_t counter_max,
                             uint32_t counter_value, uint32_t out_lut_prefix_len, uint8_t *d_out, uint64_t out_capacity, uint64_t *d_lut_out, uint64_t *n_kmers, uint64_t stats[4]);
int kmc_hip_db_histogram_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *db, uint32_t n_lut_segments, uint32_t cutoff_min, uint64_t cutoff_max,
                                uint64_t *d_hist, uint64_t stats[3]);
int kmc_hip_db_dump_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *db, uint32_t n_lut_segments, uint64_t first, uint64_t count, uint32_t cutoff_min,
                           uint64_t cutoff_max, uint32_t counter_max, uint8_t *d_text, uint64_t text_capacity, uint64_t *n_bytes, uint64_t stats[4]);

/* ---- a set expression over several ordered databases ---------------------------------------------------
 * `kmc_tools complex <operations_definition_file>` on the device: n_views database bodies as above (kmer_len <= 224, each view with its own input cutoffs) and ONE
 * expression over them, given as a postfix program of n_steps steps:
 *   kind KMC_HIP_DB_EXPR_INPUT: push the input views[arg];
 *   kind KMC_HIP_DB_INTERSECT | _UNION | _KMERS_SUBTRACT | _COUNTERS_SUBTRACT: pop the right side, pop the left side, push the node; arg is the node's counter mode
 *     KMC_HIP_DB_CNT_* (ignored by KMERS_SUBTRACT).
 * An input may be named by several steps; every such occurrence is a LEAF, and a program has at most KMC_HIP_DB_EXPR_MAX_LEAVES of them.
 * Semantics, node by node as the reference evaluates its tree (kmc_tools/expression_node.h, operations.h):
 *   leaf: the records of the input whose counter lies in the view's [cutoff_min, cutoff_max] (kmc1_db_reader.h:574-576,618);
 *   inner node: counters are uint32. A k-mer in both sides: INTERSECT, UNION and COUNTERS_SUBTRACT give it the counter min / max / sum (wraps) / left / right of the
 *     two; mode DIFF gives left - right if left > right and NO record otherwise (C2ArgOper::EqualsToOuputBundle, operations.h:40-68); KMERS_SUBTRACT drops it
 *     (:174-205). A k-mer in one side only: UNION keeps it from either side (:91-127), the two subtractions keep the left side's (:174-205, :221-255), INTERSECT
 *     drops it (:139-161). No cutoff and no clamp inside the tree;
 *   root: the writer's rule and nothing else (kmc1_db_writer.h:382-385): a counter below out->cutoff_min (>= 1) or above out->cutoff_max is dropped and tallied, what
 *     is left is clamped to out->counter_max (>= 1).
 * `out` is a kmc_hip_db_op whose op and counter_op are ignored: cutoff_min, cutoff_max, counter_max and out_lut_prefix_len of the output. d_out, d_lut_out, the counter
 * bytes and *n_kmers are as kmc_hip_db_set_op_device leaves them. A program of one INPUT step is legal (`out = a`: transform reduce).
 * out_capacity (bytes) must hold the tree's own upper bound, computed from the inputs' n_recs: UNION left + right, INTERSECT the smaller side, the subtractions the left
 * side — KMC_HIP_ECAPACITY otherwise. KMC_HIP_EINVAL: a NULL argument; a malformed program (no steps, an input index >= n_views, an unknown kind or counter mode, a
 * stack underflow, not exactly one value left); more leaves than KMC_HIP_DB_EXPR_MAX_LEAVES; a view that kmc_hip_db_set_op_device would refuse; out->cutoff_min or
 * out->counter_max below 1. KMC_HIP_ECORRUPT: a LUT whose last entry exceeds n_recs; inputs that are not ordered sets, found when a tile of the key space holds more
 * records than the partition's bound allows (nothing of that tile is written). Synchronous.
 * stats[5]: distinct k-mers present in at least one leaf; k-mers the root holds before the writer's rule; of those, dropped below cutoff_min / above cutoff_max; written.
 * $KMC_HIP_EXPR_TILE: records of a tile of the key space (downwards only; default: 32 KiB of LDS per workgroup).
 * Replaces: the tree of CUnion / CIntersection / CKmersSubtract / CCountersSubtract bundles (operations.h:85-256), one thread per node passing bundles through queues,
 * feeding CKMC1DbWriter<SIZE>::add_kmer. A chain of kmc_hip_db_set_op_device calls is NOT equivalent: every call there applies the writer's rule. */
#define KMC_HIP_DB_EXPR_INPUT 16u     /* kmc_hip_db_expr_step.kind of a leaf */
#define KMC_HIP_DB_EXPR_MAX_LEAVES 16 /* the value stack of a right-deep tree is then 16 registers of the tile kernel, and the leaves' pointers and lengths fit its arguments */
enum { KMC_HIP_DBX_STAT_KEYS = 0, KMC_HIP_DBX_STAT_RESULT = 1, KMC_HIP_DBX_STAT_BELOW_MIN = 2, KMC_HIP_DBX_STAT_ABOVE_MAX = 3, KMC_HIP_DBX_STAT_WRITTEN = 4 };
typedef struct kmc_hip_db_expr_step {
	uint32_t kind; /* KMC_HIP_DB_EXPR_INPUT, or KMC_HIP_DB_INTERSECT .. KMC_HIP_DB_COUNTERS_SUBTRACT */
	uint32_t arg;  /* INPUT: index into views; otherwise KMC_HIP_DB_CNT_MIN .. _RIGHT */
} kmc_hip_db_expr_step;
int kmc_hip_db_expr_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *views, uint32_t n_views, const kmc_hip_db_expr_step *steps, uint32_t n_steps,
                           const kmc_hip_db_op *out, uint8_t *d_out, uint64_t out_capacity, uint64_t *d_lut_out, uint64_t *n_kmers, uint64_t stats[5]);

/* ---- a KFF file's records as a database body -----------------------------------------------------------
 * What kmc_tools' KFF readers hand to `simple`, `transform`, `complex` and `filter` (kmc_tools/kff_db_reader.h; the container: kmc_core/kff_writer.cpp,
 * kmc_tools/kff_info_reader.cpp), on the device: d_kff holds the records of all raw sections of one file back to back, section i the next section_n_recs[i] of them
 * (a host array; sections may be empty). A record is ceil(kmer_len / 4) bytes of k-mer, most significant first and right-aligned (kmer_len % 4 != 0: the top bits of the
 * first byte are padding and zero), then data_size counter bytes, MOST significant first (kff_db_reader.h:374-401; `max` = 1, so no per-block count). Every section is
 * strictly ascending (the file's `ordered` = 1, which kmc_tools requires, kmer_file_header.cpp:143-147). kmer_len 1..224, data_size 1..4, (kmer_len -
 * out_lut_prefix_len) a positive multiple of 4 and out_lut_prefix_len 1..15. d_out receives n = sum of section_n_recs database records of (kmer_len -
 * out_lut_prefix_len) / 4 suffix bytes and data_size counter bytes, least significant first, as kmc_hip_db_set_op_device leaves them: the view (d_out, n, d_lut_out,
 * out_lut_prefix_len, data_size) is what every kmc_hip_db_* entry takes. *n_kmers = n.
 *   ordered = 1: ONE ascending body, d_lut_out the KMC1 LUT of 4^out_lut_prefix_len entries. At most one section that is not empty: the records are re-framed where they
 *     lie (k_kff_repack). Several: they are unpacked, sorted by the stable LSD passes kmc_hip_order_database_device uses and packed again; a k-mer that two sections
 *     hold is KMC_HIP_ECORRUPT (the reference's merge, kff_db_reader.h:929-1112, would emit it twice, and every kmc_hip_db_* entry takes unique k-mers).
 *   ordered = 0: the body as it lies in the file, d_lut_out the segmented LUT kmc_hip_db_dump_device and kmc_hip_db_histogram_device take with n_lut_segments =
 *     n_sections: n_sections x 4^out_lut_prefix_len global record offsets and ONE closing entry (= n) behind them (kmc2_db_reader.h:1776-1791) — what `transform`
 *     histogram and dump without -s read, in file order as the reference's sequential reader (kff_db_reader.h:1320-1492). No sort. With n_sections = 0 the LUT is
 *     the closing entry alone. n_sections x 4^out_lut_prefix_len + 1 must be below 2^31.
 * The same pass verifies the records: padding bits zero, the prefix below 4^out_lut_prefix_len (one check: the padding bits are the top bits of the prefix bytes), every
 * record strictly greater than its predecessor in its section on the big-endian bytes. KMC_HIP_ECORRUPT names the smallest offending record and its section; the
 * outputs are then undefined and nothing outside them is touched.
 * KMC_HIP_EINVAL: a NULL argument (d_kff may be NULL when there is no record, section_n_recs when n_sections is 0), data_size outside 1..4, kmer_len 0 or > 224, an
 * out_lut_prefix_len that is not as above, ordered > 1; KMC_HIP_ECAPACITY: out_capacity (bytes) below n records. Empty input — no section, or only empty ones — is
 * legal. Synchronous; temporaries are the stream slot's grow-only buffers. $KMC_HIP_KFF_IPT: records per thread of a k_kff_repack tile of 256 threads (default: 32 KiB
 * of LDS per workgroup, at most 8).
 * Replaces: CKFFDbReader<SIZE> (kff_db_reader.h), for sorted access a priority-queue merge over all sections on one thread. */
int kmc_hip_kff_import_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, uint32_t data_size, const uint8_t *d_kff /* the records of all sections, back to back */,
                              const uint64_t *section_n_recs /* host, [n_sections] */, uint32_t n_sections, uint32_t ordered, uint32_t out_lut_prefix_len, uint8_t *d_out,
                              uint64_t out_capacity, uint64_t *d_lut_out, uint64_t *n_kmers);

/* ---- a database body framed as the records of a KFF file ------------------------------------------------
 * The inverse of kmc_hip_kff_import_device, for KFF output: records [first, first + count) of the body db — packed records of (kmer_len - lut_prefix_len) / 4 suffix
 * bytes and counter_size counter bytes, least significant first, under a LUT of record offsets — become count KFF records of ceil(kmer_len / 4) + data_size bytes in
 * d_kff: the k-mer most significant byte first and right-aligned (the prefix bytes come back from the LUT: the prefix of record j is the index of the last LUT entry
 * <= j), then data_size - counter_size zero bytes and the counter bytes most significant first. A large body goes through in parts, as the dump does.
 *   n_lut_segments as for kmc_hip_db_dump_device: 1, an ordered body under a LUT of 4^lut_prefix_len entries; above 1, a KMC2 body (or an unordered KFF import) in file
 *     order under n_lut_segments x 4^lut_prefix_len global record offsets and the closing entry; the prefix is the entry's index modulo 4^lut_prefix_len.
 *   data_size: counter_size..4. The two writers of the reference size a set_counts output differently (kff_db_writer.h:74 takes MIN(BYTE_LOG(counter_max),
 *     BYTE_LOG(cutoff_max)), kmc1_db_writer.h BYTE_LOG(counter_value)): a body made for the one can be framed for the other.
 * db->cutoff_min and db->cutoff_max are NOT read: the body is an output — the entry that made it (kmc_hip_db_reduce_device, kmc_hip_db_set_op_device,
 * kmc_hip_count_order ...) has already applied the writer's rule (kff_db_writer.h:101-109), and every record of the range is framed.
 * Synchronous. count = 0 and an empty body are legal (d_recs and d_kff may then be NULL). No byte of d_kff outside [0, count x (ceil(kmer_len / 4) + data_size)) is
 * touched. KMC_HIP_EINVAL: a NULL argument, counter_size outside 1..4, data_size outside counter_size..4, a lut_prefix_len the other kmc_hip_db_* entries refuse,
 * kmer_len 0 or > 224, first + count > n_recs, n_lut_segments 0 or a LUT of 2^31 entries or more; KMC_HIP_ECAPACITY: kff_capacity (bytes) below what the range needs;
 * KMC_HIP_ECORRUPT: a LUT that ends behind the records. Nothing is allocated.
 * k_kff_frame works flat over tiles of 256 x ipt records, both images of a tile in LDS and moved as whole aligned 16-byte pieces; the tile's slice of the LUT is found
 * by loads that are the same in every lane (a bisection for its first record, doubling steps to its last one); a thread bisects that slice for its first record, walks a
 * few entries for each following one and bisects again where the next prefix lies further away, so a record costs O(log LUT entries) however sparse the LUT is. $KMC_HIP_KFF_IPT: records per thread, as for the import (default: 32 KiB of LDS per workgroup, at most 8, and lowered
 * while that many records of either kind are a multiple of 64 bytes: neighbouring lanes would meet on one LDS bank).
 * Replaces: CKFFDbWriter<SIZE>::add_kmer (kmc_tools/kff_db_writer.h:98-118), one k-mer at a time on one thread; the container around the records (CKFFWriter,
 * kmc_core/kff_writer.cpp) stays on the host. */
int kmc_hip_db_kff_export_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *db, uint32_t n_lut_segments, uint64_t first, uint64_t count,
                                 uint32_t data_size, uint8_t *d_kff, uint64_t kff_capacity);

/* ---- two ordered databases compared --------------------------------------------------------------------
 * `kmc_tools compare <db1> <db2>` on the device: a and b are ordered bodies as every kmc_hip_db_* entry takes them, of one kmer_len (<= 224); lut_prefix_len,
 * counter_size and cutoffs may differ. Semantics, the reference's: a record whose counter lies outside its view's [cutoff_min, cutoff_max] is absent
 * (kmc1_db_reader.h:574-576,618); the two sequences of present (k-mer, counter) pairs are walked in step; at the first ordinal i where they disagree the databases
 * differ — the COUNTER is compared before the k-mer (CComparer::Equals, operations.h:266-285) — and they differ as well where one sequence ends first (:286-292:
 * `one of input is not finished`). result[8]:
 *   [KIND]     KMC_HIP_DBC_EQUAL, _COUNTER (the counters at i differ, whatever the k-mers do), _KMER (equal counters, other k-mers), _A_ENDED, _B_ENDED
 *   [ORDINAL]  i among the present records; min(present A, present B) where one input ended; 0 for EQUAL
 *   [N_A], [N_B]            present records of a and of b
 *   [COUNTER_A], [COUNTER_B] the counters at i; 0 for an input that has no record i, and for EQUAL
 *   [RECORD_A], [RECORD_B]   the numbers in the bodies (cut records included) of the two records at i, for kmc_hip_db_dump_device; n_recs for an input that has no record
 *                            i; 0 for EQUAL
 * Both bodies are unpacked to (k-mer words, count word); an input whose cutoffs removed a record is made dense by the stable compaction of kmc_hip_db_reduce_device,
 * an input that lost nothing is not; k_db_compare walks min(present A, present B) x (words + 1) 64-bit words flat, one word per thread and step, and publishes the
 * smallest differing record of a wave with one atomic minimum; the waves of a tile that starts behind the published minimum's tile leave at once (a relaxed load: no spin, no ticket).
 * Which of the two kinds the record at the minimum is, is read from the two records afterwards. The result does not depend on the order in which tiles run.
 * Synchronous. Either input may be empty (d_recs may then be NULL). KMC_HIP_EINVAL and KMC_HIP_ECORRUPT exactly where kmc_hip_db_set_op_device returns them for its
 * inputs. Nothing but temporaries of the call is allocated.
 * $KMC_HIP_COMPARE_STEPS: words per thread of a tile of 256 threads (a power of two, default 8); $KMC_HIP_COMPARE_REVERSED=1: the workgroups take the tiles last to
 * first (tests: the smaller of two differences must win in either order).
 * Replaces: CComparer<SIZE>::Equals over two CBundle readers (kmc_tools.cpp:503-528, operations.h:258-295), one thread and two priority-queue readers. */
enum { KMC_HIP_DBC_EQUAL = 0, KMC_HIP_DBC_COUNTER = 1, KMC_HIP_DBC_KMER = 2, KMC_HIP_DBC_A_ENDED = 3, KMC_HIP_DBC_B_ENDED = 4 };
enum { KMC_HIP_DBC_RES_KIND = 0, KMC_HIP_DBC_RES_ORDINAL = 1, KMC_HIP_DBC_RES_N_A = 2, KMC_HIP_DBC_RES_N_B = 3, KMC_HIP_DBC_RES_COUNTER_A = 4, KMC_HIP_DBC_RES_COUNTER_B = 5,
       KMC_HIP_DBC_RES_RECORD_A = 6, KMC_HIP_DBC_RES_RECORD_B = 7 };
int kmc_hip_db_compare_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *a, const kmc_hip_db_view *b, uint64_t result[8]);

/* ---- end-of-run tallies ---------------------------------------------------------------------- */

/* Sum stats[4] over the context's devices with one RCCL all-reduce (ncclUint64 x 4, ncclSum) over xGMI.
 * in/out: per_dev_stats[n_dev][4] host array -> every row holds the sum. With one device this is a device
 * round-trip through the same code path. Replaces: the completer's running sums n_unique.. (kb_completer.cpp:206-209)
 * when bins are sharded over GPUs. */
int kmc_hip_allreduce_stats(kmc_hip_ctx *ctx, uint64_t *per_dev_stats);

/* ---- instrumentation --------------------------------------------------------------------------- */

/* Per-phase device time of the last completed bin on (dev): ms[0]=index (pack scan), [1]=expand, [2]=histogram,
 * [3]=radix scatter passes, [4]=compact, [5]=total enqueue->done; measured with hipEvents on the bin's stream.
 * Replaces: USE_TIMERS / MEASURE_TIMES compile-time probes (raduls_impl.h:30,567-657). */
int kmc_hip_last_timings(kmc_hip_ctx *ctx, int dev, float ms[6]);
/* Radix scatter (k_onesweep) launches of every bin completed on `dev` since the last reset: how many, their summed
 * duration (HIP events around each launch, on the launch's own stream) and the records they moved — the roofline
 * input of bench.py. Waits for the device's streams. */
int kmc_hip_scatter_totals(kmc_hip_ctx *ctx, int dev, int reset, uint64_t *n_launches, double *total_ms, uint64_t *total_records);
/* The LDS half of the hybrid sort (k_bucket_bounds + k_bucket_rank, kmc_amd/csrc/bucket_sort.hip.h; replaces the small-bucket recursion and
 * CSmallSort of raduls_impl.h:133-141,497-510 / small_sort.h:29-179): launches, summed duration (HIP events on the launch's stream) and records
 * since the last reset; plus, process-wide, how many groups of bins took the hybrid sort and how many of them had to be sorted again with LSD
 * passes over every byte because a bucket did not fit a tile. Any pointer may be NULL. Waits for the device's streams. */
int kmc_hip_local_sort_totals(kmc_hip_ctx *ctx, int dev, int reset, uint64_t *n_launches, double *total_ms, uint64_t *total_records,
                              uint64_t *n_hybrid_groups, uint64_t *n_redo_groups);
/* Which sort stage 2 runs (process-wide; overrides $KMC_HIP_HYBRID; tests and tuning): 0 = 8-bit LSD passes over every key byte + k_compact (rounds 1-2);
 * 1 = default: LSD passes over the top key bytes only, then every bucket-aligned tile ranked and counted inside LDS by k_bucket_rank (round 4: every record
 * width; $KMC_HIP_RANK_FUSE=0: rank-in-place + k_compact for k <= 32, LSD passes for wider records); -h = `h` top bytes forced. (2 — round 3's k_bucket_count /
 * k_bucket_sort, which left the library in round 6 — is taken as 1.) Also clears the group counters of kmc_hip_local_sort_totals and
 * kmc_hip_path_counters. Returns the mode that was in force. */
int kmc_hip_set_hybrid(int mode);
/* Groups of bins (a bin on its own is a group of one) by the path their sort + compaction took, process-wide since the last kmc_hip_set_hybrid: [0] top bytes
 * through HBM, tiles ranked AND counted inside LDS (k_bucket_rank fused: the default since round 4, every record width); [1] ranked in place, then k_compact
 * (one-word records whose output may outgrow a tile's span); [2] unused since round 6 (0; was k_bucket_count); [3] 8-bit
 * LSD passes over every key byte + k_compact (rounds 1-2; redo runs; tiny groups). With a context (ctx != NULL; waits for the device's streams): [4] tiles whose
 * largest bucket did not fit LDS and that k_giant_tiles sorted on their own (k-mers repeated thousands of times) and [5] the records in them, since the context
 * was made. [6] the groups of [0] (records of three words and more) whose HBM passes moved one word per record — the key's top four bytes above the record's
 * number — with the records gathered by number inside k_bucket_rank (process-wide, like [0..3]). [7] reserved (0). What replaces raduls_impl.h:216-520,
 * :680-737 / small_sort.h for a group. */
int kmc_hip_path_counters(kmc_hip_ctx *ctx, int dev, uint64_t counters[8]);
/* Diagnostics (process-wide, since the library was loaded): where the host-boundary calls (kmc_hip_process_bin_submit/_wait, kmc_hip_process_bins_submit/_wait) spent
 * their wall time, in seconds summed over all slots: [0] pack starts + device buffers, [1] staging copy in (callers whose images are in ordinary memory), [2] enqueueing
 * copies and launches, [3] waiting for the kernels (includes the H2D copy in front of them and whatever other slots queued before), [4] D2H of the exact-size results,
 * [5] staging copy out (callers whose output buffers are ordinary memory); [6] calls, [7] redo rounds (counts). What the drop-in's worker report prints under
 * $KMC_HIP_VERBOSE; no reference counterpart (the CPU worker has no host link). */
int kmc_hip_host_boundary_times(double seconds[8]);
/* Optional, once per (device, slot), before the slot's first bin: ONE device allocation of `bytes` from which the host-boundary entries (kmc_hip_process_bin_submit/_wait,
 * kmc_hip_process_bins_submit/_wait) carve the slot's grow-only buffers; a buffer that does not fit what is left is allocated on its own, as without a slab. Lets a caller
 * whose process is busy mapping and unmapping memory while bins arrive (the reference's RAM-only stage 2: mem_disk_file.cpp:84-100) pay for device allocations ahead of time —
 * the drop-in's loader reserves while KMC's stage 1 runs. What the CPU worker gets from CMemoryBins, reserved by the reader before the worker sees the bin
 * (queues.h:1288-1340). Refused (KMC_HIP_ECAPACITY, nothing allocated) when it would leave the device with less than half of its memory free. Freed with the context. */
int kmc_hip_reserve_slot(kmc_hip_ctx *ctx, int dev, int slot, uint64_t bytes);
/* Device memory helpers so non-HIP callers (ctypes tests, the C++ worker) need not link HIP themselves. */
int kmc_hip_malloc(kmc_hip_ctx *ctx, int dev, uint64_t bytes, void **d_ptr);
int kmc_hip_free(kmc_hip_ctx *ctx, int dev, void *d_ptr);
int kmc_hip_memcpy_h2d(kmc_hip_ctx *ctx, int dev, void *d_dst, const void *src, uint64_t bytes);
int kmc_hip_memcpy_d2h(kmc_hip_ctx *ctx, int dev, void *dst, const void *d_src, uint64_t bytes);
int kmc_hip_host_register(kmc_hip_ctx *ctx, void *ptr, uint64_t bytes);   /* pin the caller's arena (CMemoryBins buffer) */
int kmc_hip_host_unregister(kmc_hip_ctx *ctx, void *ptr);
int kmc_hip_host_alloc(kmc_hip_ctx *ctx, uint64_t bytes, void **ptr);      /* pinned host memory (hipHostMalloc) for _submit/_wait callers */
int kmc_hip_host_free(kmc_hip_ctx *ctx, void *ptr);
int kmc_hip_synchronize(kmc_hip_ctx *ctx, int dev);

/* ---- stage-isolating test hooks (not used by the worker): run only index+expand, or only compaction ---- */
int kmc_hip_debug_expand(kmc_hip_ctx *ctx, int dev, const kmc_hip_bin_params *params, const uint8_t *superkmers, uint64_t size,
                         uint64_t n_rec, const uint64_t *pack_bytes, uint64_t n_packs, uint64_t *out_recs /* n_rec*words */);
int kmc_hip_debug_compact(kmc_hip_ctx *ctx, int dev, const kmc_hip_bin_params *params, const uint64_t *sorted_recs, uint64_t n,
                          uint8_t *out_suffix, uint64_t out_capacity, uint64_t *out_bytes, uint64_t *lut, uint64_t stats[4]);

/* ---- stage 1, first kernels (groundwork, NOT part of the drop-in) ----
 * codes: one symbol per byte, 0..3 = A C G T, anything negative = N or a read boundary (join reads with one such byte). Computes on the
 * device what CSplitter::ProcessReads (splitter.cpp:557-672) computes read by read: the minimizer signature (CMmer, kmc_api/mmer.h:25-110,
 * signature_len 5..11) of the k-mer starting at every position -> sig[n] (0xFFFFFFFF where no valid k-mer starts), and the super-k-mers in
 * position order -> sk_pos / sk_len (symbols: kmer_len + extra, extra <= 255) / sk_sig, *n_sk of them (KMC_HIP_ECAPACITY beyond sk_cap).
 * The bin of a super-k-mer is s_mapper->get_bin_id(signature) (s_mapper.h, stays with the reference), its record kb_collector.cpp:57-71. */
int kmc_hip_debug_split_reads(kmc_hip_ctx *ctx, int dev, const int8_t *codes, uint64_t n, uint32_t kmer_len, uint32_t signature_len, uint32_t *sig,
                              uint64_t *sk_pos, uint32_t *sk_len, uint32_t *sk_sig, uint64_t sk_cap, uint64_t *n_sk);

/* ---- stage 1 on the device (groundwork, NOT yet wired into the reference's stage 1) ----
 * Reads already in HBM as codes (as above) -> the signature bins of CSplitter::ProcessReads + CKmerBinCollector (splitter.cpp:557-672,
 * kb_collector.cpp:57-106), left IN HBM in the layout kmc_hip_process_bins_device takes: no trip through the host, no temporary files
 * (CKmerBinStorer, kb_storer.cpp) between the stages.
 *   _plan : signatures, super-k-mers, per-bin totals. d_sig_to_bin[4^signature_len + 1] (device, int32) is the reference's signature map
 *           (CSignatureMapper::get_bin_id, s_mapper.h:232; the map itself is built from stage-0 statistics and stays with the reference).
 *           Fills the caller's HOST arrays: bin_base[n_bins + 1] (byte offset of each bin image in the buffer to allocate, 256-byte aligned;
 *           the last entry is the buffer size incl. the readable slack stage 2 wants), bin_bytes / bin_superkmers / bin_kmers[n_bins],
 *           pack_base[n_bins + 1] (first entry of each bin in the pack-start array; the last entry is the array length).
 *   _emit : writes the bin images into d_bins[bin_base[n_bins]] and the pack boundaries into d_pack_start[pack_base[n_bins]]; d_codes and
 *           d_sig_to_bin of the plan must still be valid. Afterwards bin b is
 *           kmc_hip_bin_desc{d_bins + bin_base[b], bin_bytes[b], bin_kmers[b], d_pack_start + pack_base[b], pack_base[b+1] - pack_base[b] - 1, ...}.
 *           Super-k-mers of a bin are NOT in read order (neither are the reference's with several splitter threads); stage 2 is order-blind.
 *   _free : releases the plan (always call it, also after a failed _emit).
 * One call handles up to 2^41 symbols; the plan keeps 16 bytes per super-k-mer (one per 10-40 symbols of real reads at k = 27) until _free. */
typedef struct kmc_hip_s1_plan kmc_hip_s1_plan;
int kmc_hip_split_reads_plan(kmc_hip_ctx *ctx, int dev, const int8_t *d_codes, uint64_t n, uint32_t kmer_len, uint32_t signature_len, const int32_t *d_sig_to_bin,
                             uint32_t n_bins, kmc_hip_s1_plan **plan, uint64_t *bin_base, uint64_t *bin_bytes, uint64_t *bin_superkmers, uint64_t *bin_kmers,
                             uint64_t *pack_base);
int kmc_hip_split_reads_emit(kmc_hip_ctx *ctx, kmc_hip_s1_plan *plan, uint8_t *d_bins, uint64_t *d_pack_start);
void kmc_hip_split_reads_free(kmc_hip_ctx *ctx, kmc_hip_s1_plan *plan);

/* ---- stage 1, one part of input text (the engine behind kmc_amd/host/kb_splitter_plugin.h; emulation-validated) ----
 * Replaces, for one part the reference's readers cut (fastq_reader.cpp), CSplitter::ProcessReads and the n_bins CKmerBinCollectors up to the
 * bin-part buffers (splitter.cpp:557-672, kb_collector.cpp:34-106): text (host) -> the part's bin records (host, bin b at recs + bin_off[b],
 * bin_bytes[b] bytes; bins are 256-byte aligned. *recs_bytes = bytes of `recs` the part needs: about 0.3 bytes per symbol + 256 per bin for
 * real reads, but up to 1 + k/4 bytes per k-mer when every k-mer is its own super-k-mer — KMC_HIP_ECAPACITY asks for a second call with a
 * larger buffer) and per bin the three sums a
 * collector keeps: bin_kmers (n_recs), bin_superkmers (n_super_kmers), bin_plus_x (n_plus_x_recs, kb_collector.h:72-118); *n_reads = titles
 * in the part. kmc_hip_split_set_map uploads CSignatureMapper's map (s_mapper.h:232; 4^signature_len + 1 entries) once per device.
 * part_kind 1 = a part the reader labelled ReadType::long_read (queues.h:40: a record longer than the reader's buffer, handed out in parts that
 * overlap by k - 1 symbols): an optional title, then symbols only (CSplitter::GetSeqLongRead, splitter.cpp:70-86). Lines of mem_part_pmm_reads
 * symbols or more inside an ordinary part, and long-read parts, reach the reference's super-k-mer loop in pieces that overlap by k - 1 symbols
 * (splitter.cpp:141-145, :226-231, :80-84); the kernels cut super-k-mers at the same piece starts, so the three sums agree with the reference's.
 * file_type 2 = a multi-line FASTA part as CFastqReader::GetPartFromMultilneFasta cuts it (ReadType::na, fastq_reader.cpp:399-468: a title keeps its
 * run of end-of-line bytes, the sequence text has none, a part may start inside a sequence); it is split as CSplitter::GetSeq's MULTILINE_FASTA branch
 * does (splitter.cpp:304-323), *n_reads = titles in the part, and part_kind must be 0.
 * file_type 4 = a part of BAM alignment records as the reference's BAM readers hand them out (ReadType::na, fastq_reader.cpp:191-362: BGZF inflated and the
 * file header taken off on the host; whole records, the first one at byte 0), smaller than 2 GiB, part_kind 0. It is split as CSplitter::GetSeq's BAM branch
 * does (splitter.cpp:326-419): records with flag 0x100 or 0x800 are skipped, every other record is one read (*n_reads; one without bases too), its 4-bit
 * bases decoded (A C G T, all else invalid) and, with both_strands 0 and flag 0x10, reversed and complemented. KMC_HIP_UNCOVERED: the records do not end
 * exactly at the part's end, a block_size below what its header, name, cigar, bases and qualities take (a negative one included), a negative l_seq, a header
 * that runs past the part, or an included record of line_cap bases or more (the reference writes those past its buffer). Works with every flag. The value is 4,
 * not 3: callers of libraries from before BAM use 3 as the file type that is KMC_HIP_EINVAL and that kmc_hip_split_covers answers 0 for, and it stays so (as
 * 0x101 does among the capabilities).
 * Returns 0, a negative KMC_HIP_E* code, or KMC_HIP_UNCOVERED: the text is MALFORMED in a way CSplitter::GetSeq tolerates and the kernels do not
 * reproduce (blank lines, quality of another length than its sequence, a lone '\r', control characters; multi-line FASTA: a part that ends inside a
 * title line) — nothing was produced; the stage-1 worker
 * stops the run with an error (it has no path into the reference splitter unless built with -DKMC_HIP_S1_REFERENCE_FALLBACK). Calls on one
 * (dev, slot) are serialised. */
#define KMC_HIP_UNCOVERED 1
typedef struct kmc_hip_split_params {
	uint32_t kmer_len, signature_len, n_bins, max_x; /* max_x: CKMCParams::max_x (0..3) */
	uint32_t both_strands;
	uint32_t file_type;                              /* 0 = FASTA (one line per sequence), 1 = FASTQ, 2 = multi-line FASTA (-fm), 4 = BAM records (-fbam); 3 stays unknown */
	uint64_t line_cap;                               /* CKMCParams::mem_part_pmm_reads */
	uint32_t part_kind;                              /* 0 = whole records (ReadType::normal_read), 1 = ReadType::long_read */
	uint32_t flags;                                  /* KMC_HIP_SPLIT_*; any other bit is KMC_HIP_EINVAL. (Named `reserved`, to be 0, before the first flag.) */
} kmc_hip_split_params;
/* flags bit 0: homopolymer compression (-hc). Every buffer CSplitter::GetSeq returns — a whole line, or ONE PIECE of a line of mem_part_pmm_reads symbols
 * or more, of a long-read part or of a multi-line sequence — is compressed on its own before the super-k-mers are cut (HomopolymerCompressSeq,
 * splitter.cpp:424-435, :575-581: the first symbol and every symbol whose code differs from the one before it), with every file_type and part_kind;
 * *n_reads does not change. A library from before the flag ignores the field silently: ask kmc_hip_split_covers(KMC_HIP_SPLIT_COVERS_HOMOPOLYMER) first. */
#define KMC_HIP_SPLIT_HOMOPOLYMER 1u
/* flags bit 2 (value 4; value 2 stays an unknown bit): histogram estimation while counting (--opt-out-size). The k-mers of the part — of every buffer
 * CSplitter::GetSeq returns, BEFORE the homopolymer compression, as CntHashEstimator::Process sees them (splitter.cpp:576-577) — are added to the estimator
 * that kmc_hip_estimate_open opened on `dev`; KMC_HIP_EINVAL when none is open or its kmer_len differs. Works with every file_type, part_kind and with
 * KMC_HIP_SPLIT_HOMOPOLYMER. A call that does not return 0 (KMC_HIP_UNCOVERED and KMC_HIP_ECAPACITY included) leaves the counters as they were. Ask
 * kmc_hip_split_covers(KMC_HIP_SPLIT_COVERS_ESTIMATE) first. */
#define KMC_HIP_SPLIT_ESTIMATE 4u
int kmc_hip_split_set_map(kmc_hip_ctx *ctx, int dev, const int32_t *sig_to_bin, uint32_t signature_len);
/* 1 if kmc_hip_split_part takes parts of this file_type, else 0. Added without a new ABI version: a loader that finds no such symbol takes file_type 0
 * and 1 only. Values above the file types ask for a capability: KMC_HIP_SPLIT_COVERS_HOMOPOLYMER = the flag KMC_HIP_SPLIT_HOMOPOLYMER is honoured (a library
 * from before the flag answers 0, like for every value it does not know). */
#define KMC_HIP_SPLIT_COVERS_HOMOPOLYMER 0x100u
#define KMC_HIP_SPLIT_COVERS_ESTIMATE 0x102u /* KMC_HIP_SPLIT_ESTIMATE and kmc_hip_estimate_open / _read / _close (0x101 stays unknown) */
#define KMC_HIP_SPLIT_COVERS_SMALLK 0x103u   /* kmc_hip_smallk_open / _part / _read / _close: small k (k <= 13) counted on the device */
int kmc_hip_split_covers(uint32_t what);
int kmc_hip_split_part(kmc_hip_ctx *ctx, int dev, int slot, const kmc_hip_split_params *p, const uint8_t *text, uint64_t size, uint8_t *recs,
                       uint64_t recs_capacity, uint64_t *recs_bytes, uint64_t *bin_off, uint64_t *bin_bytes, uint64_t *bin_kmers, uint64_t *bin_superkmers, uint64_t *bin_plus_x,
                       uint64_t *n_reads);

/* ---- stage 1, histogram estimation while counting (--opt-out-size; added within ABI version 4, like kmc_hip_split_covers) ----
 * The device's share of the reference's CntHashEstimator (kmc_core/libs/ntHash/ntHashWrapper.h): two arrays of 2^r 32-bit counters on `dev`, to which every
 * kmc_hip_split_part call with KMC_HIP_SPLIT_ESTIMATE adds the sampled ntHash values of its part's k-mers (k_s1_nthash_estimate; counters wrap at 2^32 like
 * the reference's). The caller adds the counters of all devices into the reference's own object, whose EstimateHistogram then runs unchanged.
 * _open : allocates and zeroes 2 x 2^r counters (1 GB at the reference's r = 27); s in 1..16, r in 8..27 (the reference: s = 7 or 11). Opening again with the
 *         same (kmer_len, s, r) is a no-op, with another triple KMC_HIP_EINVAL.
 * _read : waits for everything the device's slots have launched, then copies entries [first, first + count) of the 2^(r+1)-entry array (type 0 first, then
 *         type 1) to dst: a caller can drain in chunks, without a second gigabyte on the host. The counters are not cleared.
 * _close: frees the counters (kmc_hip_destroy does it too); no estimator open is not an error. It waits for the kmc_hip_split_part calls with
 * KMC_HIP_SPLIT_ESTIMATE that are inside the library on `dev`; a call that starts after it finds no estimator (KMC_HIP_EINVAL). kmc_hip_destroy does not
 * wait: like every other call, none may be running when it is called. */
int kmc_hip_estimate_open(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, uint32_t s, uint32_t r);
int kmc_hip_estimate_read(kmc_hip_ctx *ctx, int dev, uint64_t first, uint64_t count, uint32_t *dst);
int kmc_hip_estimate_close(kmc_hip_ctx *ctx, int dev);

/* ---- stage 1, small k (k <= 13; added within ABI version 4, like kmc_hip_estimate_*) ----
 * With k <= 13 the reference counts without signatures and bins whenever the tables fit in memory, and always when k < signature_len ("small k optimization",
 * CKMC::AdjustMemoryLimitsSmallK kmc.h:677-750): every CWSmallKSplitter worker (splitter.h:138, splitter.cpp:929-983) keeps one table of 4^k counters that
 * CSplitter::ProcessReadsSmallK (splitter.cpp:682-805) increments once per k-mer, and stage 2 (ProcessSmallKOptimization_Stage2 kmc.h:865-960, CSmallKCompleter)
 * sums the workers' tables and writes the database. These entries keep ONE such table on `dev` (k_s1_smallk_count); the caller hands it to the reference's
 * stage 2 as one worker's table (kmc_hip_smallk_read), or turns it into the database where it lies (kmc_hip_smallk_tally / kmc_hip_smallk_view_device below). Ask
 * kmc_hip_split_covers(KMC_HIP_SPLIT_COVERS_SMALLK) first.
 * _open : replaces the reserve + memset of CWSmallKSplitter::operator() (splitter.cpp:954-955): allocates and zeroes 4^kmer_len uint64 counters (8 bytes at
 *         k = 1, 512 MB at k = 13); kmer_len 1..13. Opening again with the same (kmer_len, both_strands) is a no-op, with another pair KMC_HIP_EINVAL.
 * _part : replaces CSplitter::ProcessReadsSmallK for one part (splitter.cpp:682-805, with GetSeq :88-421 and HomopolymerCompressSeq :424-435 in front): every
 *         window of k valid symbols of every buffer GetSeq returns (compressed first with KMC_HIP_SPLIT_HOMOPOLYMER) adds one to its k-mer's counter — the
 *         canonical k-mer, min(forward, reverse complement) as 2k-bit integers, with both_strands, the forward one without. Uses kmer_len, both_strands,
 *         file_type (0, 1, 2, 4), line_cap (mem_part_pmm_reads; (MAX_LINE_SIZE + 1) * 8 in this mode, kmc.h:689), part_kind and flags (only
 *         KMC_HIP_SPLIT_HOMOPOLYMER; any other bit is KMC_HIP_EINVAL) of `p`; signature_len, n_bins and max_x are ignored and no signature map is needed.
 *         *n_reads = titles in the part (as kmc_hip_split_part), *n_kmers = the windows counted (CSplitter::total_kmers :751, :799). Returns 0, a negative
 *         code, or KMC_HIP_UNCOVERED for the malformed inputs kmc_hip_split_part answers it for. A call that does not return 0 leaves the table as it was: the
 *         counting kernel is launched only once the call can no longer fail. Calls on different slots of one device may run at once and add into the one table.
 * _read : replaces CWSmallKSplitter::GetResult (splitter.h:155-158): waits for everything the device's slots have launched, then copies entries
 *         [first, first + count) to dst, so that a caller can drain in chunks. The table is not cleared.
 * _close: replaces CWSmallKSplitter::Release (splitter.h:167-170): frees the table (kmc_hip_destroy does it too); none open is not an error. It waits for the
 *         kmc_hip_smallk_part calls that are inside the library on `dev`; a call that starts after it finds no table (KMC_HIP_EINVAL). */
int kmc_hip_smallk_open(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, uint32_t both_strands);
int kmc_hip_smallk_part(kmc_hip_ctx *ctx, int dev, int slot, const kmc_hip_split_params *p, const uint8_t *text, uint64_t size, uint64_t *n_reads, uint64_t *n_kmers);
int kmc_hip_smallk_read(kmc_hip_ctx *ctx, int dev, uint64_t first, uint64_t count, uint64_t *dst);
int kmc_hip_smallk_close(kmc_hip_ctx *ctx, int dev);

/* ---- small k, stage 2 on the device: the table as a database (added within ABI version 4, like the entries above) ----
 * Replaces CSmallKCompleter::CompleteKMCFormat / CompleteKFFFormat (kb_completer.h:149-378) for a caller that goes on on the device or writes the files itself: the
 * table of 4^kmer_len uint64 counters — d_table, or with d_table == NULL the one kmc_hip_smallk_open made on `dev`; then kmer_len must be the open table's, and the
 * kmc_hip_smallk_part calls in flight on `dev` are waited for, as _read does — is its own database order (the index is the k-mer), so k_sk_tally / k_db_cumsum /
 * k_sk_emit compact and frame it without a sort. The table is not modified (the reference clamps in place). An entry c != 0 is unique; c < cutoff_min is below,
 * c > cutoff_max above, everything else kept, in 64-bit arithmetic (counts above 2^32 are ordinary: poly-A, k = 1). Both entries are synchronous.
 * Ask kmc_hip_split_covers(KMC_HIP_SPLIT_COVERS_SMALLK_DB) first.
 * _tally      : stats[4] = unique, below, above, kept — what kmc prints, what a caller sizes d_out by and chooses out_lut_prefix_len from (kmc.h:906-936).
 * _view_device: the kept entries in index order as records in d_out, *n_kmers of them, and the same stats[4]. counter_size = kmc_hip_counter_size(cutoff_max,
 *               counter_max). framing 0, KMC1: (kmer_len - out_lut_prefix_len) / 4 suffix bytes, most significant first (0..3; none is what k <= 4 gets), then
 *               counter_size bytes of min(count, counter_max), least significant first; d_lut_out receives all 4^out_lut_prefix_len entries (the kept entries in front
 *               of the prefix's first k-mer); *view is filled as kmc_hip_count_order fills it, and for kmer_len - out_lut_prefix_len >= 4 every kmc_hip_db_* entry takes
 *               it. A body without suffix bytes is for files only: the other entries refuse it. framing 1, KFF: ceil(kmer_len / 4) k-mer bytes, most significant first,
 *               then data_size (counter_size..4) bytes of the clamped count, MOST significant first; no LUT, d_lut_out and view may be NULL. both_strands describes the
 *               table for the caller's header and changes nothing in the body.
 * KMC_HIP_EINVAL: a NULL output, kmer_len outside 1..13, no open table (or one of another kmer_len) with d_table == NULL, cutoff_min < 1, cutoff_max < cutoff_min,
 * counter_size outside 1..4 (counter_max == 1 gives 0), KMC1 with out_lut_prefix_len outside 1..kmer_len or (kmer_len - out_lut_prefix_len) % 4 != 0, KFF with
 * data_size outside counter_size..4, framing above 1. KMC_HIP_ECAPACITY: out_capacity (bytes) below kept x record bytes — found after the tally, before anything is
 * written. $KMC_HIP_SMALLK_IPT (1..8, default 8): entries per thread; $KMC_HIP_SMALLK_TALLY_WGS (default 2048): the most workgroups k_sk_tally is launched
 * with; the result depends on neither. */
#define KMC_HIP_SPLIT_COVERS_SMALLK_DB 0x109u /* kmc_hip_smallk_tally / _view_device (0x108 stays unknown, as 0x106, 0x104 and 0x101 do) */
int kmc_hip_smallk_tally(kmc_hip_ctx *ctx, int dev, const uint64_t *d_table, uint32_t kmer_len, uint64_t cutoff_min, uint64_t cutoff_max, uint64_t stats[4]);
int kmc_hip_smallk_view_device(kmc_hip_ctx *ctx, int dev, const uint64_t *d_table, uint32_t kmer_len, uint32_t both_strands, uint64_t cutoff_min, uint64_t cutoff_max,
                               uint64_t counter_max, uint32_t framing, uint32_t out_lut_prefix_len, uint32_t data_size, uint8_t *d_out, uint64_t out_capacity,
                               uint64_t *d_lut_out, kmc_hip_db_view *view, uint64_t *n_kmers, uint64_t stats[4]);

/* ---- stage 0, signature statistics (added within ABI version 4, like kmc_hip_smallk_*) ----
 * The reference decides which signature goes to which bin from a sample of the input: every CWStatsSplitter worker (splitter.h:118, splitter.cpp:878-925) runs
 * CSplitter::CalcStats (splitter.cpp:439-533) over the parts of the stage-0 queue, which adds 1 + len - kmer_len per super-k-mer to stats[signature] (4^m + 1
 * uint32 counters, entry 4^m the special signature); the workers' arrays are summed and CSignatureMapper::Init (s_mapper.h:141-235) builds the map from them. A
 * super-k-mer is a maximal run of k-mers with one signature, so stats[s] is the number of k-mer windows whose signature is s. These entries keep ONE such array
 * on `dev` (k_s1_sig_stats); the caller hands it to the reference's Init as one worker's array. Ask kmc_hip_split_covers(KMC_HIP_SPLIT_COVERS_SIGSTATS) first.
 * _open : replaces the allocation and fill of CWStatsSplitter's constructor (splitter.cpp:878-893): allocates and zeroes 4^signature_len + 1 uint32 counters;
 *         signature_len 5..11, signature_len <= kmer_len <= 256. Opening again with the same (kmer_len, signature_len) is a no-op, with another pair KMC_HIP_EINVAL.
 * _part : replaces CSplitter::CalcStats for one part (with GetSeq splitter.cpp:88-421 and HomopolymerCompressSeq :424-435 in front): every window of kmer_len
 *         valid symbols of every buffer GetSeq returns (compressed first with KMC_HIP_SPLIT_HOMOPOLYMER) adds one to the counter of its signature, the minimum
 *         of norm[m-mer] over the window's m-mers (kmc_api/mmer.h:39-95). Uses kmer_len, signature_len, file_type (0, 1, 2, 4), line_cap, part_kind and flags
 *         (only KMC_HIP_SPLIT_HOMOPOLYMER; any other bit is KMC_HIP_EINVAL) of `p`; n_bins, max_x and both_strands decide nothing, and no signature map is read.
 *         *n_reads = titles in the part (as kmc_hip_split_part), *n_kmers = the windows added: the sum of the part's adds. Counters wrap at 2^32 like the
 *         reference's. Returns 0, a negative code, or KMC_HIP_UNCOVERED for the malformed inputs kmc_hip_split_part answers it for. A call that does not return 0
 *         leaves the array as it was: the kernel is launched only once the call can no longer fail. Calls on different slots of one device may run at once.
 * _read : replaces CWStatsSplitter::GetStats (splitter.cpp:919-925): waits for everything the device's slots have launched, then copies entries
 *         [first, first + count) to dst. The array is not cleared.
 * _close: frees the array (kmc_hip_destroy does it too); none open is not an error. It waits for the kmc_hip_sigstats_part calls that are inside the library on
 *         `dev`; a call that starts after it finds no array (KMC_HIP_EINVAL). */
#define KMC_HIP_SPLIT_COVERS_SIGSTATS 0x107u /* kmc_hip_sigstats_open / _part / _read / _close (0x106 stays unknown, as 0x104 and 0x101 do) */
int kmc_hip_sigstats_open(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, uint32_t signature_len);
int kmc_hip_sigstats_part(kmc_hip_ctx *ctx, int dev, int slot, const kmc_hip_split_params *p, const uint8_t *text, uint64_t size, uint64_t *n_reads, uint64_t *n_kmers);
int kmc_hip_sigstats_read(kmc_hip_ctx *ctx, int dev, uint64_t first, uint64_t count, uint32_t *dst);
int kmc_hip_sigstats_close(kmc_hip_ctx *ctx, int dev);
/* Which entries of the array can be a signature at all: dst[s] = 1 for the m-mers CMmer::is_allowed accepts (kmc_api/mmer.h:39-64, the kernels' own s1_allowed),
 * 0 for the others and for entry 4^signature_len; 4^signature_len + 1 bytes. CSignatureMapper::Init gives a bin to every allowed m-mer, also to those that never
 * occur as a signature because their reverse complement is the smaller one — which a table of norm values cannot tell from a forbidden one. Needs no context. */
int kmc_hip_sigstats_allowed(uint32_t signature_len, uint8_t *dst);

/* ---- a counting session: reads in, one ordered database body out, no bin record leaves the device (added within ABI version 4, like kmc_hip_smallk_*) ----
 * The reference carries every part's bin records from stage 1 to stage 2 through the host: CKmerBinStorer appends each collector's buffer to its bin's file
 * (kb_storer.cpp), CKmerBinReader reads every file back as one bin image (kb_reader.h:141-190), the completer hands the sorted bins on (kb_completer.cpp:160-320). A
 * session keeps them in HBM instead: kmc_hip_count_part is kmc_hip_split_part up to the records and leaves them in the session's store; kmc_hip_count_finish gathers
 * the (part, bin) segments into whole bins (k_cnt_gather), runs stage 2 on them where they lie and keeps the bins' outputs; kmc_hip_count_order merges those into the
 * body `kmc <in> <db> <tmp>` followed by `kmc_tools transform <db> sort <out>` writes, as a kmc_hip_db_view. All occurrences of a canonical k-mer share one signature and
 * so one bin: the result depends neither on the signature map, nor on n_bins, nor on where the parts are cut. One device per session; k <= 13 has kmc_hip_smallk_*.
 * Ask kmc_hip_split_covers(KMC_HIP_SPLIT_COVERS_COUNT) first.
 * _open  : replaces the opening of the bin files (CKmerBinStorer::OpenFiles, kb_storer.cpp). Fixes kmer_len, signature_len, n_bins and both_strands of `p` for the
 *          session; max_x is taken as 0; the signature map is the one kmc_hip_split_set_map uploaded for `dev`. KMC_HIP_EINVAL for the parameters kmc_hip_split_part
 *          refuses and for kmer_len > 224 (kmc_hip_order_database_device's limit).
 * _part  : replaces CSplitter::ProcessReads + the collectors for one part, as kmc_hip_split_part does, and CKmerBinStorer::PutBinToTmpFile for its buffers
 *          (kb_storer.cpp): every file_type (0, 1, 2, 4), part_kind and KMC_HIP_SPLIT_HOMOPOLYMER; KMC_HIP_SPLIT_ESTIMATE, and a part whose kmer_len, signature_len,
 *          n_bins or both_strands differ from the session's, are KMC_HIP_EINVAL. The part's records are copied device to device into the store: HBM chunks
 *          ($KMC_HIP_COUNT_CHUNK_MB each, default 256; 0: a chunk per part), a part larger than a chunk gets one of its own, a part's records lie in one chunk. A call
 *          that does not return 0 (KMC_HIP_UNCOVERED, KMC_HIP_ENOMEM when the store cannot grow, a device error) leaves the session exactly as it was. Calls on
 *          different slots may run at once; calls on one slot are serialised.
 * _finish: replaces CKmerBinReader (kb_reader.h:141-190: one image per bin, its expander packs) and the sorters' hand-over to the completer (kb_completer.cpp:160-320).
 *          Once per session, synchronous, no _part may be running. Lays the bins out (256-byte aligned images, one expander pack per non-empty (part, bin) segment: any
 *          run of whole records is a legal pack, queues.h:376-396), gathers, frees the store, then runs kmc_hip_process_bins_device over the bins in index order, in
 *          batches whose worst-case outputs (n_rec x kmc_hip_out_rec_bytes) fit an arena — a quarter of the free device memory, or $KMC_HIP_COUNT_ARENA_MB (0: a bin
 *          per batch); a bin beyond the arena is a batch of its own, KMC_HIP_ENOMEM before anything of it is launched if that does not fit either — and keeps each bin's
 *          output in a tight store. bp: kmer_len and both_strands of the session, output_type 0, without_output 0; lut_prefix_len (> 0) is the bins' own and
 *          invisible in the result. stats[4]: the sum of the bins' tallies in KMC_HIP_STAT_* order; totals[4]: reads, super-k-mers, k-mers entering stage 2, bytes of
 *          bin records; *n_records: the records stage 2 kept (what a caller chooses out_lut_prefix_len by). A session without a single k-mer finishes with zeros.
 *          KMC_HIP_EINVAL while a _part call is running. After an error behind the gather the session can only be closed; one in front of it leaves the session as it was.
 * _order : replaces kmc_tools' sort of the completer's database (CKMC1DbWriter fed by a priority queue over the bins). After _finish, any number of times: allocates
 *          body and LUT for out_lut_prefix_len (owned by the session, replaced by the next _order), runs kmc_hip_order_database_device over the bins' outputs and
 *          fills *view: d_recs, n_recs, d_lut, lut_prefix_len, counter_size = kmc_hip_counter_size(cutoff_max, counter_max), and the cutoffs of bp — every record
 *          lies inside them, so the view goes to every kmc_hip_db_* entry as it is. (With a cutoff_min above counter_max the clamped counters lie below cutoff_min and
 *          the view, like the header the reference writes for such a run, hides every record from a reader that applies the cutoffs.) KMC_HIP_EINVAL before _finish and for (kmer_len - out_lut_prefix_len) % 4 != 0.
 * _info  : info[6] = parts in the store, chunks of the store, table entries the gather copied, stage-2 batches, k-mers of the largest bin, bins that are not empty
 *          (the last four after _finish; diagnostics, the front end's balance figure, tests).
 * _timings: seconds[4] of the session's last _finish and _order: layout, allocations and uploads of _finish (wall clock); k_cnt_gather (HIP events around the launch);
 *          stage 2 with the copies into the tight store (wall clock); the last _order (wall clock). What tools/count_bench.py reports.
 * _close : replaces CKmerBinStorer::Release and the removal of the bin files (kb_storer.cpp): frees everything, in any state; kmc_hip_destroy closes open sessions.
 *          _part after _finish and a second _finish are KMC_HIP_EINVAL. */
#define KMC_HIP_SPLIT_COVERS_COUNT 0x105u /* kmc_hip_count_open / _part / _finish / _order / _info / _timings / _close (0x104 stays unknown, as 0x101 does: callers of libraries
                                           * from before the session use it as the capability that answers 0) */
typedef struct kmc_hip_count kmc_hip_count; /* one counting session on one device */
int kmc_hip_count_open(kmc_hip_ctx *ctx, int dev, const kmc_hip_split_params *p, kmc_hip_count **out);
int kmc_hip_count_part(kmc_hip_ctx *ctx, kmc_hip_count *session, int slot, const kmc_hip_split_params *p, const uint8_t *text, uint64_t size, uint64_t *n_reads);
int kmc_hip_count_finish(kmc_hip_ctx *ctx, kmc_hip_count *session, const kmc_hip_bin_params *bp, uint64_t stats[4], uint64_t totals[4], uint64_t *n_records);
int kmc_hip_count_order(kmc_hip_ctx *ctx, kmc_hip_count *session, uint32_t out_lut_prefix_len, kmc_hip_db_view *view);
int kmc_hip_count_info(kmc_hip_ctx *ctx, kmc_hip_count *session, uint64_t info[6]);
int kmc_hip_count_timings(kmc_hip_ctx *ctx, kmc_hip_count *session, double seconds[4]);
void kmc_hip_count_close(kmc_hip_ctx *ctx, kmc_hip_count *session);
/* Test hook in the style of kmc_hip_debug_expand: k_cnt_gather, the segmented copy of _finish, on a table of n_segments x {source offset, destination offset, bytes}
 * (host memory; offsets into d_src / d_dst, device memory), and the wait for it. No byte outside a destination segment is written, none outside
 * [source, source + bytes + 16) of a segment is read. $KMC_HIP_COUNT_GATHER_WGS: workgroups of the persistent grid (default 2048). */
int kmc_hip_debug_gather_segments(kmc_hip_ctx *ctx, int dev, const uint8_t *d_src, uint8_t *d_dst, const uint64_t *table, uint64_t n_segments);

/* ---- BGZF input: BAM files and bgzipped FASTA / FASTQ inflated on the device (added within ABI version 4) ----
 * A BGZF file is a sequence of independent gzip members of at most 64 KiB of output each; every member names its own compressed size (BSIZE in the BC extra
 * subfield) and ends with CRC32 and ISIZE. The host walks the headers, the device inflates one member per wave and checks its CRC (k_bgzf_inflate, bgzf.hip.h).
 * Ask kmc_hip_split_covers(KMC_HIP_SPLIT_COVERS_BGZF) first. */
#define KMC_HIP_SPLIT_COVERS_BGZF 0x10Bu /* kmc_hip_bgzf_scan / _inflate_device / _inflate, kmc_hip_bam_whole_records (0x10A stays unknown, as the even values before it do) */
#define KMC_HIP_BGZF_NONE 0xFFFFFFFFu     /* *first_bad when no member failed */
typedef struct kmc_hip_bgzf_member {
	uint64_t src_off;  /* of the member's raw deflate data, in the bytes the table was made from */
	uint64_t dst_off;  /* of its output: the running sum of the isize fields in front of it */
	uint32_t comp_len; /* bytes of deflate data: between the gzip header and the 8 bytes of CRC32 and ISIZE */
	uint32_t isize, crc;
	uint32_t reserved; /* 0 */
} kmc_hip_bgzf_member;
/* Host only, no context. Walks the gzip member headers of src[0 .. size) from byte 0: magic 1f 8b, CM 8, FLG.FEXTRA; the BC subfield of length 2 wherever it lies in
 * the extra field; FNAME, FCOMMENT and FHCRC skipped where the flags are set. Fills members[0 .. *n_members) and stops in front of the first member that is not wholly
 * inside `size` (the caller carries src[*src_used ..) to its next piece), that would take the output beyond max_out_bytes, or at `cap` members. *out_bytes = the
 * members' isize summed. An empty member (the 28-byte EOF block, also in the middle of a file) is an ordinary member of isize 0. KMC_HIP_ECORRUPT, with the byte
 * offset in the message: a header that is not BGZF, isize above 65536, a BSIZE too small for the member's own header and trailer.
 * Replaces: the header walk of CFastqReader's BGZF branch (kmc_core/fastq_reader.cpp:72-140). */
int kmc_hip_bgzf_scan(const uint8_t *src, uint64_t size, uint64_t max_out_bytes, kmc_hip_bgzf_member *members, uint64_t cap, uint64_t *n_members, uint64_t *src_used,
                      uint64_t *out_bytes);
/* d_src[0 .. src_size) (device) holds the compressed bytes the table (host memory; uploaded here) was made from; member i's output goes to
 * d_dst[dst_off, dst_off + isize). Stored, fixed and dynamic blocks, several blocks per member, matches up to length 258 at distance up to 32768. Synchronous; calls on
 * one (dev, slot) are serialised. Returns 0 with *first_bad = KMC_HIP_BGZF_NONE, or KMC_HIP_ECORRUPT with *first_bad = the smallest failing member, its source offset
 * and the reason in the message: everything zlib's inflate refuses, output that is not isize bytes, compressed bytes left over or missing, a CRC32 mismatch. A failing
 * member ends alone: every other member's output is written, a failing member's range is left as it was. member_errors (host, [n_members], may be NULL): 0 or the
 * reason's number per member. KMC_HIP_ECAPACITY: dst_capacity below the end of the last member's output; KMC_HIP_EINVAL: a NULL argument, a bad slot, a member with
 * isize or comp_len above 65536, one that ends behind src_size, dst_off values that do not ascend past the output before them. No byte outside a member's compressed
 * bytes is read and none outside its output range is written, whatever the bytes say.
 * Replaces: inflate() and crc32() per member on one host thread (kmc_core/fastq_reader.cpp:141-189). */
int kmc_hip_bgzf_inflate_device(kmc_hip_ctx *ctx, int dev, int slot, const uint8_t *d_src, uint64_t src_size, const kmc_hip_bgzf_member *members, uint64_t n_members,
                                uint8_t *d_dst, uint64_t dst_capacity, uint32_t *first_bad, uint32_t *member_errors);
/* the same from host memory to host memory: upload, the device entry's kernel, download (buffers of the slot, grow-only). What `count` uses today; a session entry that
 * takes device text would spare the two copies (kmc_hip_bgzf_inflate_device exists for it). With KMC_HIP_ECORRUPT the good members' output is in dst all the same.
 * Replaces: the same lines as kmc_hip_bgzf_inflate_device; CFastqReader::ProcessBamBinaryPart's caller could hand its compressed buffer to this entry. */
int kmc_hip_bgzf_inflate(kmc_hip_ctx *ctx, int dev, int slot, const uint8_t *src, uint64_t src_size, const kmc_hip_bgzf_member *members, uint64_t n_members, uint8_t *dst,
                         uint64_t dst_capacity, uint32_t *first_bad, uint32_t *member_errors);
/* milliseconds between HIP events around the last k_bgzf_inflate of (dev, slot): what tools/bgzf_bench.py reports */
int kmc_hip_bgzf_last_ms(kmc_hip_ctx *ctx, int dev, int slot, float *ms);
/* Host only. Walks the block_size chain of inflated BAM alignment records from byte 0 of buf: *n_bytes = the bytes that are whole records (what a part may hold; the
 * rest is carried in front of the next piece), *n_records = how many. KMC_HIP_ECORRUPT: a block_size below 32 (negative ones included).
 * Replaces: the record walk of CFastqReader::GetPartFromBam (kmc_core/fastq_reader.cpp:285-361). */
int kmc_hip_bam_whole_records(const uint8_t *buf, uint64_t size, uint64_t *n_bytes, uint64_t *n_records);

#ifdef __cplusplus
}
#endif
#endif /* KMC_HIP_H */
