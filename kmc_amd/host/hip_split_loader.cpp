/*
 * kmc_amd/host/hip_split_loader.cpp — the HIP split engine of the stage-1 worker (kb_splitter_plugin.h): kmc_hip_split_part of
 * include/kmc_hip.h through the library hip_loader.cpp already loaded. Had not met a real GPU when round 2 ended; proven on the
 * CPU twice: bound to a mock of the library and to the library's own source over an emulated HIP runtime (tests/test_stage1_plugin.py,
 * tests/test_hostlib_emulated.py).
 * No CPU fallback: without the library or a GPU the engine reports the error and the worker raises it.
 */
#include <dlfcn.h>

#include <mutex>
#include <string>
#include <vector>

#include "kmc_hip.h"
#include "split_engine.h"

bool kmc_hip_loader_handles(void *&so, kmc_hip_ctx *&ctx, int &n_dev, int &n_slots, std::string &err); /* hip_loader.cpp */

namespace {
struct SplitApi {
	int (*set_map)(kmc_hip_ctx *, int, const int32_t *, uint32_t) = nullptr;
	int (*split_part)(kmc_hip_ctx *, int, int, const kmc_hip_split_params *, const uint8_t *, uint64_t, uint8_t *, uint64_t, uint64_t *, uint64_t *, uint64_t *,
	                  uint64_t *, uint64_t *, uint64_t *, uint64_t *) = nullptr;
	const char *(*last_error)(kmc_hip_ctx *) = nullptr;
	int (*covers)(uint32_t) = nullptr; /* optional: a library without kmc_hip_split_covers takes FASTA and FASTQ only, and no flags */
	/* optional, added with KMC_HIP_SPLIT_ESTIMATE: a library without them (or whose kmc_hip_split_covers does not know the capability) does not estimate */
	int (*est_open)(kmc_hip_ctx *, int, uint32_t, uint32_t, uint32_t) = nullptr;
	int (*est_read)(kmc_hip_ctx *, int, uint64_t, uint64_t, uint32_t *) = nullptr;
	int (*est_close)(kmc_hip_ctx *, int) = nullptr;
	std::mutex est_mtx;
	std::vector<char> est_on; /* per device: an estimator was opened and not drained yet */
	/* optional, added with KMC_HIP_SPLIT_COVERS_SMALLK: a library without them (or whose kmc_hip_split_covers does not know the capability) counts no small k */
	int (*sk_open)(kmc_hip_ctx *, int, uint32_t, uint32_t) = nullptr;
	int (*sk_part)(kmc_hip_ctx *, int, int, const kmc_hip_split_params *, const uint8_t *, uint64_t, uint64_t *, uint64_t *) = nullptr;
	int (*sk_read)(kmc_hip_ctx *, int, uint64_t, uint64_t, uint64_t *) = nullptr;
	int (*sk_close)(kmc_hip_ctx *, int) = nullptr;
	std::mutex sk_mtx;
	std::vector<char> sk_on; /* per device: a small-k table was opened and not drained yet */
	/* optional, added with KMC_HIP_SPLIT_COVERS_SIGSTATS: a library without them (or whose kmc_hip_split_covers does not know the capability) leaves stage 0 to the reference */
	int (*ss_open)(kmc_hip_ctx *, int, uint32_t, uint32_t) = nullptr;
	int (*ss_part)(kmc_hip_ctx *, int, int, const kmc_hip_split_params *, const uint8_t *, uint64_t, uint64_t *, uint64_t *) = nullptr;
	int (*ss_read)(kmc_hip_ctx *, int, uint64_t, uint64_t, uint32_t *) = nullptr;
	int (*ss_close)(kmc_hip_ctx *, int) = nullptr;
	std::mutex ss_mtx;
	std::vector<char> ss_on; /* per device: an array of signature statistics was opened and not drained yet */
	kmc_hip_ctx *ctx = nullptr;
	int n_dev = 1, n_slots = 1;
	std::string err;
	std::mutex map_mtx;
	std::vector<uint64_t> map_hash; /* per device: hash of the signature -> bin map that was uploaded last (0 = none) */
} g_split;
std::once_flag g_split_once;

void bind()
{
	void *so = nullptr;
	if (!kmc_hip_loader_handles(so, g_split.ctx, g_split.n_dev, g_split.n_slots, g_split.err))
		return;
	g_split.set_map = reinterpret_cast<decltype(g_split.set_map)>(dlsym(so, "kmc_hip_split_set_map"));
	g_split.split_part = reinterpret_cast<decltype(g_split.split_part)>(dlsym(so, "kmc_hip_split_part"));
	g_split.last_error = reinterpret_cast<decltype(g_split.last_error)>(dlsym(so, "kmc_hip_last_error"));
	g_split.covers = reinterpret_cast<decltype(g_split.covers)>(dlsym(so, "kmc_hip_split_covers"));
	g_split.est_open = reinterpret_cast<decltype(g_split.est_open)>(dlsym(so, "kmc_hip_estimate_open"));
	g_split.est_read = reinterpret_cast<decltype(g_split.est_read)>(dlsym(so, "kmc_hip_estimate_read"));
	g_split.est_close = reinterpret_cast<decltype(g_split.est_close)>(dlsym(so, "kmc_hip_estimate_close"));
	g_split.sk_open = reinterpret_cast<decltype(g_split.sk_open)>(dlsym(so, "kmc_hip_smallk_open"));
	g_split.sk_part = reinterpret_cast<decltype(g_split.sk_part)>(dlsym(so, "kmc_hip_smallk_part"));
	g_split.sk_read = reinterpret_cast<decltype(g_split.sk_read)>(dlsym(so, "kmc_hip_smallk_read"));
	g_split.sk_close = reinterpret_cast<decltype(g_split.sk_close)>(dlsym(so, "kmc_hip_smallk_close"));
	g_split.ss_open = reinterpret_cast<decltype(g_split.ss_open)>(dlsym(so, "kmc_hip_sigstats_open"));
	g_split.ss_part = reinterpret_cast<decltype(g_split.ss_part)>(dlsym(so, "kmc_hip_sigstats_part"));
	g_split.ss_read = reinterpret_cast<decltype(g_split.ss_read)>(dlsym(so, "kmc_hip_sigstats_read"));
	g_split.ss_close = reinterpret_cast<decltype(g_split.ss_close)>(dlsym(so, "kmc_hip_sigstats_close"));
	if (!g_split.set_map || !g_split.split_part || !g_split.last_error) {
		g_split.err = "libkmc_hip.so lacks kmc_hip_split_set_map / kmc_hip_split_part";
		g_split.ctx = nullptr;
	}
	g_split.map_hash.assign((size_t)g_split.n_dev, 0);
	g_split.est_on.assign((size_t)g_split.n_dev, 0);
	g_split.sk_on.assign((size_t)g_split.n_dev, 0);
	g_split.ss_on.assign((size_t)g_split.n_dev, 0);
}

struct HipSplitEngine : KmcSplitEngine {
	KmcSplitParams P;
	int dev, slot;
	std::string err;
	std::vector<uint8_t> recs;
	std::vector<uint64_t> arrays; /* bin_off | bin_bytes | bin_kmers | bin_superkmers | bin_plus_x */
	std::vector<uint32_t> drain_buf; /* estimate_drain, sigstats_drain: one chunk of one device's counters */
	std::vector<uint64_t> sk_drain_buf; /* smallk_drain: one chunk of one device's table */

	uint64_t map_hash = 0; /* of this run's map: a second KMC run in the same process (library API) with another map must not split with the first one's */
	HipSplitEngine(const KmcSplitParams &p, int dev, int slot) : P(p), dev(dev), slot(slot)
	{
		arrays.assign((size_t)5 * p.n_bins, 0);
		uint64_t h = 1469598103934665603ull ^ p.signature_len; /* FNV-1a over the map's entries, once per engine */
		const size_t n = p.sig_to_bin ? ((size_t)1 << (2 * p.signature_len)) + 1 : 0; /* no map: an engine of the small-k worker, which splits nothing */
		for (size_t i = 0; i < n; ++i)
			h = (h ^ (uint32_t)p.sig_to_bin[i]) * 1099511628211ull;
		map_hash = h ? h : 1;
	}
	std::string last_error() override { return err; }
	bool covers_multiline_fasta() const override { return g_split.ctx && g_split.covers && g_split.covers(2) == 1; }
	bool covers_bam() const override { return g_split.ctx && g_split.covers && g_split.covers(4) == 1; }
	/* a library from before the flag ignores it silently: the query is the only way to know */
	bool covers_homopolymer_compression() const override { return g_split.ctx && g_split.covers && g_split.covers(KMC_HIP_SPLIT_COVERS_HOMOPOLYMER) == 1; }
	bool covers_histogram_estimation() const override
	{
		return g_split.ctx && g_split.covers && g_split.est_open && g_split.est_read && g_split.est_close && g_split.covers(KMC_HIP_SPLIT_COVERS_ESTIMATE) == 1;
	}
	int estimate_open() override
	{
		if (!covers_histogram_estimation() || !P.estimate_r) {
			err = "HIP split engine: no histogram estimation (the library does not cover it, or the engine was made without estimate_s / estimate_r)";
			return KMC_HIP_EINVAL;
		}
		std::lock_guard<std::mutex> lck(g_split.est_mtx);
		if (int rc = g_split.est_open(g_split.ctx, dev, P.kmer_len, P.estimate_s, P.estimate_r)) { /* a second engine on the device: the same triple, a no-op */
			err = g_split.last_error(g_split.ctx);
			return rc;
		}
		g_split.est_on[dev] = 1;
		return 0;
	}
	int estimate_drain(uint64_t first, uint64_t count, uint32_t *dst) override
	{
		const uint64_t entries = (uint64_t)2 << P.estimate_r;
		if (!P.estimate_r || !g_split.ctx || count > ((uint64_t)1 << 24) || first > entries || count > entries - first) {
			err = "HIP split engine: estimate_drain outside the counters, or more than 2^24 entries at once";
			return KMC_HIP_EINVAL;
		}
		std::lock_guard<std::mutex> lck(g_split.est_mtx);
		drain_buf.resize(count);
		for (int d = 0; d < g_split.n_dev; ++d) {
			if (!g_split.est_on[d])
				continue;
			if (int rc = g_split.est_read(g_split.ctx, d, first, count, drain_buf.data())) {
				err = g_split.last_error(g_split.ctx);
				return rc;
			}
			for (uint64_t i = 0; i < count; ++i)
				dst[i] += drain_buf[i];
			if (first + count == entries) {
				g_split.est_on[d] = 0;
				if (int rc = g_split.est_close(g_split.ctx, d)) {
					err = g_split.last_error(g_split.ctx);
					return rc;
				}
			}
		}
		if (first + count == entries)
			std::vector<uint32_t>().swap(drain_buf);
		return 0;
	}
	bool covers_small_k() const override
	{
		return g_split.ctx && g_split.covers && g_split.sk_open && g_split.sk_part && g_split.sk_read && g_split.sk_close && g_split.covers(KMC_HIP_SPLIT_COVERS_SMALLK) == 1;
	}
	int smallk_open() override
	{
		if (!covers_small_k()) {
			err = "HIP split engine: the library does not count small k on the device";
			return KMC_HIP_EINVAL;
		}
		std::lock_guard<std::mutex> lck(g_split.sk_mtx);
		if (int rc = g_split.sk_open(g_split.ctx, dev, P.kmer_len, P.both_strands ? 1u : 0u)) { /* a second engine on the device: the same pair, a no-op */
			err = g_split.last_error(g_split.ctx);
			return rc;
		}
		g_split.sk_on[dev] = 1;
		return 0;
	}
	int smallk_part(const uint8_t *text, uint64_t size, bool long_read, uint64_t &n_reads, uint64_t &n_kmers) override
	{
		if (!covers_small_k()) {
			err = "HIP split engine: the library does not count small k on the device";
			return KMC_HIP_EINVAL;
		}
		kmc_hip_split_params hp;
		hp.kmer_len = P.kmer_len;
		hp.signature_len = hp.n_bins = hp.max_x = 0; /* not read */
		hp.both_strands = P.both_strands ? 1u : 0u;
		hp.file_type = (uint32_t)P.file_type;
		hp.line_cap = P.line_cap;
		hp.part_kind = long_read ? 1u : 0u;
		hp.flags = P.homopolymer_compressed ? KMC_HIP_SPLIT_HOMOPOLYMER : 0u;
		const int rc = g_split.sk_part(g_split.ctx, dev, slot, &hp, text, size, &n_reads, &n_kmers);
		if (rc == KMC_HIP_UNCOVERED)
			return KMC_SPLIT_UNCOVERED;
		if (rc)
			err = g_split.last_error(g_split.ctx);
		return rc;
	}
	int smallk_drain(uint64_t first, uint64_t count, uint64_t *dst) override
	{
		const uint64_t entries = (uint64_t)1 << (2 * P.kmer_len);
		if (!g_split.ctx || P.kmer_len > 13 || count > ((uint64_t)1 << 22) || first > entries || count > entries - first) {
			err = "HIP split engine: smallk_drain outside the table, or more than 2^22 entries at once";
			return KMC_HIP_EINVAL;
		}
		std::lock_guard<std::mutex> lck(g_split.sk_mtx);
		sk_drain_buf.resize(count);
		for (int d = 0; d < g_split.n_dev; ++d) {
			if (!g_split.sk_on[d])
				continue;
			if (int rc = g_split.sk_read(g_split.ctx, d, first, count, sk_drain_buf.data())) {
				err = g_split.last_error(g_split.ctx);
				return rc;
			}
			for (uint64_t i = 0; i < count; ++i)
				dst[i] += sk_drain_buf[i];
			if (first + count == entries) {
				g_split.sk_on[d] = 0;
				if (int rc = g_split.sk_close(g_split.ctx, d)) {
					err = g_split.last_error(g_split.ctx);
					return rc;
				}
			}
		}
		if (first + count == entries)
			std::vector<uint64_t>().swap(sk_drain_buf);
		return 0;
	}
	bool covers_signature_stats() const override
	{
		return g_split.ctx && g_split.covers && g_split.ss_open && g_split.ss_part && g_split.ss_read && g_split.ss_close && g_split.covers(KMC_HIP_SPLIT_COVERS_SIGSTATS) == 1;
	}
	int sigstats_open() override
	{
		if (!covers_signature_stats()) {
			err = "HIP split engine: the library does not compute the signature statistics on the device";
			return KMC_HIP_EINVAL;
		}
		std::lock_guard<std::mutex> lck(g_split.ss_mtx);
		if (int rc = g_split.ss_open(g_split.ctx, dev, P.kmer_len, P.signature_len)) { /* a second engine on the device: the same pair, a no-op */
			err = g_split.last_error(g_split.ctx);
			return rc;
		}
		g_split.ss_on[dev] = 1;
		return 0;
	}
	int sigstats_part(const uint8_t *text, uint64_t size, bool long_read, uint64_t &n_reads, uint64_t &n_kmers) override
	{
		if (!covers_signature_stats()) {
			err = "HIP split engine: the library does not compute the signature statistics on the device";
			return KMC_HIP_EINVAL;
		}
		kmc_hip_split_params hp;
		hp.kmer_len = P.kmer_len;
		hp.signature_len = P.signature_len;
		hp.n_bins = hp.max_x = 0; /* not read */
		hp.both_strands = P.both_strands ? 1u : 0u;
		hp.file_type = (uint32_t)P.file_type;
		hp.line_cap = P.line_cap;
		hp.part_kind = long_read ? 1u : 0u;
		hp.flags = P.homopolymer_compressed ? KMC_HIP_SPLIT_HOMOPOLYMER : 0u;
		const int rc = g_split.ss_part(g_split.ctx, dev, slot, &hp, text, size, &n_reads, &n_kmers);
		if (rc == KMC_HIP_UNCOVERED)
			return KMC_SPLIT_UNCOVERED;
		if (rc)
			err = g_split.last_error(g_split.ctx);
		return rc;
	}
	int sigstats_drain(uint64_t first, uint64_t count, uint32_t *dst) override
	{
		const uint64_t entries = ((uint64_t)1 << (2 * P.signature_len)) + 1;
		if (!g_split.ctx || P.signature_len > 11 || count > ((uint64_t)1 << 23) || first > entries || count > entries - first) {
			err = "HIP split engine: sigstats_drain outside the array, or more than 2^23 entries at once";
			return KMC_HIP_EINVAL;
		}
		std::lock_guard<std::mutex> lck(g_split.ss_mtx);
		drain_buf.resize(count);
		for (int d = 0; d < g_split.n_dev; ++d) {
			if (!g_split.ss_on[d])
				continue;
			if (int rc = g_split.ss_read(g_split.ctx, d, first, count, drain_buf.data())) {
				err = g_split.last_error(g_split.ctx);
				return rc;
			}
			for (uint64_t i = 0; i < count; ++i)
				dst[i] += drain_buf[i];
			if (first + count == entries) {
				g_split.ss_on[d] = 0;
				if (int rc = g_split.ss_close(g_split.ctx, d)) {
					err = g_split.last_error(g_split.ctx);
					return rc;
				}
			}
		}
		if (first + count == entries)
			std::vector<uint32_t>().swap(drain_buf);
		return 0;
	}
	int split_part(const uint8_t *text, uint64_t size, bool long_read, KmcSplitResult &out) override
	{
		if (!g_split.ctx) {
			err = g_split.err.empty() ? "HIP split engine not initialised" : g_split.err;
			return KMC_HIP_EDEVICE;
		}
		{
			std::lock_guard<std::mutex> lck(g_split.map_mtx);
			if (g_split.map_hash[dev] != map_hash) {
				if (int rc = g_split.set_map(g_split.ctx, dev, P.sig_to_bin, P.signature_len)) {
					err = g_split.last_error(g_split.ctx);
					return rc;
				}
				g_split.map_hash[dev] = map_hash;
			}
		}
		kmc_hip_split_params hp;
		hp.kmer_len = P.kmer_len;
		hp.signature_len = P.signature_len;
		hp.n_bins = P.n_bins;
		hp.max_x = P.max_x;
		hp.both_strands = P.both_strands ? 1u : 0u;
		hp.file_type = (uint32_t)P.file_type;
		hp.line_cap = P.line_cap;
		hp.part_kind = long_read ? 1u : 0u;
		hp.flags = (P.homopolymer_compressed ? KMC_HIP_SPLIT_HOMOPOLYMER : 0u) | (P.estimate_r ? KMC_HIP_SPLIT_ESTIMATE : 0u);
		/* records of real reads take ~0.3 bytes per symbol; text whose k-mers are nearly all their own super-k-mer needs more: second call */
		if (recs.size() < size + 256ull * (P.n_bins + 1))
			recs.resize(size + 256ull * (P.n_bins + 1));
		const size_t nb = P.n_bins;
		uint64_t n_reads = 0, need = 0;
		int rc = g_split.split_part(g_split.ctx, dev, slot, &hp, text, size, recs.data(), recs.size(), &need, &arrays[0], &arrays[nb], &arrays[2 * nb], &arrays[3 * nb],
		                            &arrays[4 * nb], &n_reads);
		if (rc == KMC_HIP_ECAPACITY && need > recs.size()) {
			recs.resize(need);
			rc = g_split.split_part(g_split.ctx, dev, slot, &hp, text, size, recs.data(), recs.size(), &need, &arrays[0], &arrays[nb], &arrays[2 * nb], &arrays[3 * nb],
			                        &arrays[4 * nb], &n_reads);
		}
		if (rc == KMC_HIP_UNCOVERED)
			return KMC_SPLIT_UNCOVERED;
		if (rc) {
			err = g_split.last_error(g_split.ctx);
			return rc;
		}
		out.recs = recs.data();
		out.bin_off = &arrays[0];
		out.bin_bytes = &arrays[nb];
		out.bin_kmers = &arrays[2 * nb];
		out.bin_superkmers = &arrays[3 * nb];
		out.bin_plus_x = &arrays[4 * nb];
		out.n_reads = n_reads;
		return 0;
	}
};
} // namespace

KmcSplitEngine *kmc_make_split_engine(const KmcSplitParams &params, int worker_idx, int /*n_workers*/)
{
	std::call_once(g_split_once, bind);
	const int n = g_split.n_dev > 0 ? g_split.n_dev : 1;
	return new HipSplitEngine(params, worker_idx % n, (worker_idx / n) % (g_split.n_slots > 0 ? g_split.n_slots : 1));
}
