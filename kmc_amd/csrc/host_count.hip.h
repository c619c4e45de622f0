/* kmc_amd/csrc/host_count.hip.h — part of kmc_hip.hip (included there, not compiled on its own): the counting session. A reads file goes in part by part, every part's
 * bin records stay in HBM; at the end they are gathered into whole bins (k_cnt_gather, count_gather.hip.h), stage 2 runs on the bins where they lie and the result is
 * ordered into one database body. What the reference does between its stages with CKmerBinStorer and the bin files (kb_storer.cpp), CKmerBinReader (kb_reader.h) and the
 * completer's hand-over (kb_completer.cpp) — without a byte of bin records leaving the device. */

struct kmc_hip_count {
	int dev = 0;
	u32 k = 0, m = 0, n_bins = 0, both = 0;
	std::mutex mtx; /* the part list and the store: _part calls on different slots run at once */
	/* the store: HBM chunks, grown chunk by chunk; a part's records lie in one chunk */
	struct Chunk {
		uint8_t *p = nullptr;
		u64 cap = 0, used = 0;
	};
	struct Part {
		const uint8_t *d_recs = nullptr; /* inside a chunk, 256-byte aligned */
		std::vector<u64> bin_off, bin_bytes, bin_kmers, bin_sk;
		u64 n_reads = 0;
	};
	u64 chunk_bytes = 0; /* 0: every part gets a chunk of its own */
	std::vector<Chunk> chunks;
	std::vector<Part> parts;
	bool finished = false; /* _finish ran: no more parts */
	bool has_result = false; /* ... and got through: _order may run */
	u32 parts_running = 0;   /* _part calls between their first look at the session and their return (under mtx): _finish refuses while there are any */
	/* after _finish */
	kmc_hip_bin_params bp = {};
	std::vector<kmc_hip_bin_desc> descs; /* d_out: inside `results`; d_lut, d_stats, d_out_bytes: resident */
	std::vector<void *> results;         /* the tight result store, one block per stage-2 batch */
	void *d_luts = nullptr, *d_small = nullptr;
	u64 n_records = 0, n_segments = 0, n_batches = 0, gathered_bytes = 0, largest_bin = 0, bins_in_use = 0;
	/* after _order: owned by the session, replaced by the next _order */
	void *d_body = nullptr, *d_lut_out = nullptr;
	double seconds[4] = {0, 0, 0, 0}; /* kmc_hip_count_timings */
};

namespace {
constexpr u64 CNT_CHUNK_MB_DEFAULT = 256;

/* $name as a number of MiB; 0 is a value of its own (a chunk per part, a bin per batch); `dflt_bytes` when unset or not a number */
u64 count_env_mb(const char *name, u64 dflt_bytes)
{
	const char *e = getenv(name);
	if (!e || *e < '0' || *e > '9')
		return dflt_bytes;
	return (u64)strtoull(e, nullptr, 10) << 20;
}

int count_check_fixed(const char *who, const kmc_hip_split_params *p)
{
	if (p->kmer_len < 1 || p->kmer_len > (uint32_t)S1_MAX_K || p->signature_len < 5 || p->signature_len > 11 || p->signature_len > p->kmer_len || p->n_bins < 1 ||
	    p->n_bins > (uint32_t)S1_MAX_BINS)
		return fail(KMC_HIP_EINVAL, std::string(who) + ": unsupported parameters");
	if (p->kmer_len > 224)
		return fail(KMC_HIP_EINVAL, std::string(who) + ": kmer_len <= 224 (the limit of kmc_hip_order_database_device)");
	return 0;
}

void count_free_store(kmc_hip_count *c)
{
	for (auto &ch : c->chunks)
		if (ch.p)
			(void)hipFree(ch.p);
	c->chunks.clear();
}

void count_release(kmc_hip_count *c)
{
	count_free_store(c);
	for (void *p : c->results)
		(void)hipFree(p);
	for (void *p : {c->d_luts, c->d_small, c->d_body, c->d_lut_out})
		if (p)
			(void)hipFree(p);
	delete c;
}

/* the table on the device, the launch, the wait: what the session and the test hook share. table: n x {source, destination, bytes} on the host */
int count_gather_run(Slot &s, const uint8_t *src_base, uint8_t *dst_base, const u64 *table, u64 n, float *kernel_ms = nullptr)
{
	if (kernel_ms)
		*kernel_ms = 0;
	if (!n)
		return 0;
	DevTemps tmp;
	void *d_table = nullptr;
	if (int rc = tmp.alloc(&d_table, (size_t)n * 24))
		return rc;
	HIPCHK(hipMemcpyAsync(d_table, table, (size_t)n * 24, hipMemcpyHostToDevice, s.stream));
	const u32 wgs = env_positive("KMC_HIP_COUNT_GATHER_WGS", CG_MAX_WGS); /* a test switch: a grid smaller than the table */
	HIPCHK(hipEventRecord(s.ev[0], s.stream));
	k_cnt_gather<<<dim3((u32)(n < wgs ? n : wgs)), dim3(CG_THREADS), 0, s.stream>>>(src_base, dst_base, (const u64 *)d_table, n);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(s.ev[1], s.stream));
	HIPCHK(hipStreamSynchronize(s.stream));
	if (kernel_ms)
		HIPCHK(hipEventElapsedTime(kernel_ms, s.ev[0], s.ev[1]));
	return 0;
}

void count_close_all(kmc_hip_ctx *ctx)
{
	for (kmc_hip_count *c : ctx->counts)
		count_release(c);
	ctx->counts.clear();
}
} // namespace

/* ---- test hook: k_cnt_gather on a planted table ---- */
int kmc_hip_debug_gather_segments(kmc_hip_ctx *ctx, int dev, const uint8_t *d_src, uint8_t *d_dst, const uint64_t *table, uint64_t n_segments)
{
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (n_segments && (!table || !d_src || !d_dst))
		return fail(KMC_HIP_EINVAL, "kmc_hip_debug_gather_segments: NULL argument");
	Slot &s = ctx->devs[dev]->slot[0];
	std::lock_guard<std::mutex> lck(s.mtx);
	return count_gather_run(s, d_src, d_dst, (const u64 *)table, n_segments);
}

int kmc_hip_count_open(kmc_hip_ctx *ctx, int dev, const kmc_hip_split_params *p, kmc_hip_count **out)
{
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (!p || !out)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_open: NULL argument");
	if (int rc = count_check_fixed("kmc_hip_count_open", p))
		return rc;
	kmc_hip_count *c = new kmc_hip_count;
	c->dev = dev, c->k = p->kmer_len, c->m = p->signature_len, c->n_bins = p->n_bins, c->both = p->both_strands ? 1u : 0u;
	c->chunk_bytes = count_env_mb("KMC_HIP_COUNT_CHUNK_MB", CNT_CHUNK_MB_DEFAULT << 20);
	std::lock_guard<std::mutex> lck(ctx->mtx);
	ctx->counts.push_back(c);
	*out = c;
	return 0;
}

int kmc_hip_count_part(kmc_hip_ctx *ctx, kmc_hip_count *c, int slot, const kmc_hip_split_params *p, const uint8_t *text, uint64_t size, uint64_t *n_reads)
{
	const char *who = "kmc_hip_count_part";
	if (!c)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_part: no session");
	if (int rc = set_dev(ctx, c->dev))
		return rc;
	if (!p || (size && !text) || !n_reads || slot < 0 || slot >= N_SLOTS)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_part: bad argument");
	if (int rc = count_check_fixed(who, p))
		return rc;
	if (p->kmer_len != c->k || p->signature_len != c->m || p->n_bins != c->n_bins || (p->both_strands ? 1u : 0u) != c->both)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_part: kmer_len, signature_len, n_bins and both_strands are the session's");
	if (p->flags & KMC_HIP_SPLIT_ESTIMATE)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_part: KMC_HIP_SPLIT_ESTIMATE belongs to kmc_hip_split_part");
	if (p->flags & ~KMC_HIP_SPLIT_HOMOPOLYMER)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_part: unknown bit in flags");
	if (int rc = s1_part_check(who, p, size))
		return rc;
	Dev &d = *ctx->devs[c->dev];
	if (!d.d_sig_map || d.sig_map_entries != (1u << (2 * p->signature_len)) + 1)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_part: kmc_hip_split_set_map was not called for this signature length");
	/* Lock order: a _part call takes the session's mutex alone, lets go, then the slot's mutex and the session's inside it; _finish takes the session's mutex and slot
	 * mutexes inside it. The two orders never meet: _finish refuses while parts_running is not 0, and a _part call that arrives while _finish holds the session waits here,
	 * before it holds a slot, and finds the session finished. */
	struct Running {
		kmc_hip_count *c;
		~Running()
		{
			std::lock_guard<std::mutex> lck(c->mtx);
			--c->parts_running;
		}
	};
	{
		std::lock_guard<std::mutex> lck(c->mtx);
		if (c->finished)
			return fail(KMC_HIP_EINVAL, "kmc_hip_count_part: the session is finished");
		++c->parts_running;
	}
	Running running{c};
	Slot &s = d.slot[slot];
	std::lock_guard<std::mutex> lck(s.mtx);
	/* the work area of kmc_hip_split_part (see there) */
	const bool hc = (p->flags & KMC_HIP_SPLIT_HOMOPOLYMER) != 0;
	const size_t per_byte = p->file_type == 4 ? 14 + (hc ? 4 : 0) : (p->file_type == 2 ? 10 : 8) + (hc ? 2 : 0);
	S1Part part;
	if (int rc = part.begin(d, slot, p, text, size, per_byte))
		return rc;
	S1PartParams &sp = part.sp;
	sp.m = p->signature_len;
	sp.n_bins = p->n_bins;
	sp.max_x = 0;
	sp.d_sig_to_bin = d.d_sig_map;
	sp.sorted_emit = getenv("KMC_HIP_S1_SORTED_EMIT") != nullptr;
	S1PartResult R;
	try {
		uint8_t *d_text = part.upload();
		if (int rc = part.code(who, s1_split_part(part.be, d_text, part.size, part.ends_with_newline(), sp, R), R))
			return rc;
	} catch (const S1BackendFailure &f) {
		return fail_hip(f.what, f.e);
	}
	/* the records are made; from here to the part's entry in the list the session's mutex is held, so that whatever fails takes back exactly what it took. The store may
	 * grow (hipMalloc) and the copy is waited for under it: the store copies of calls on different slots go one after the other, their chains do not */
	std::lock_guard<std::mutex> clck(c->mtx);
	if (c->finished)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_part: the session is finished");
	const u64 need = up256(R.recs_bytes);
	bool new_chunk = false;
	u64 at = 0;
	if (R.recs_bytes) {
		if (c->chunks.empty() || c->chunks.back().used + need > c->chunks.back().cap) {
			kmc_hip_count::Chunk ch;
			ch.cap = need > c->chunk_bytes ? need : c->chunk_bytes; /* a part larger than a chunk gets a chunk of its own */
			hipError_t e = hipMalloc((void **)&ch.p, ch.cap + 256);
			if (e != hipSuccess)
				return fail_hip("kmc_hip_count_part: the store cannot grow", e);
			c->chunks.push_back(ch);
			new_chunk = true;
		}
		kmc_hip_count::Chunk &ch = c->chunks.back();
		at = ch.used;
		/* device to device, ordered on the slot's stream behind the chain; the wait tells whether it arrived */
		hipError_t e = hipMemcpyAsync(ch.p + at, R.d_recs, R.recs_bytes, hipMemcpyDeviceToDevice, s.stream);
		if (e == hipSuccess)
			e = hipStreamSynchronize(s.stream);
		u32 err = 0;
		int rc = e == hipSuccess ? read_and_clear_sticky(s, err) : fail_hip("kmc_hip_count_part: copy into the store", e);
		if (!rc && err)
			rc = err_to_code(err);
		if (rc) {
			if (new_chunk) {
				(void)hipFree(ch.p);
				c->chunks.pop_back();
			}
			return rc;
		}
		ch.used = at + need;
	}
	kmc_hip_count::Part pt;
	pt.d_recs = R.recs_bytes ? c->chunks.back().p + at : nullptr;
	pt.bin_off = R.bin_off, pt.bin_bytes = R.bin_bytes, pt.bin_kmers = R.bin_kmers, pt.bin_sk = R.bin_sk;
	pt.bin_off.resize(c->n_bins), pt.bin_bytes.resize(c->n_bins), pt.bin_kmers.resize(c->n_bins), pt.bin_sk.resize(c->n_bins);
	pt.n_reads = R.n_reads;
	c->parts.push_back(std::move(pt));
	*n_reads = R.n_reads;
	return 0;
}

int kmc_hip_count_finish(kmc_hip_ctx *ctx, kmc_hip_count *c, const kmc_hip_bin_params *bp, uint64_t stats[4], uint64_t totals[4], uint64_t *n_records)
{
	if (!c)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_finish: no session");
	if (int rc = set_dev(ctx, c->dev))
		return rc;
	if (!bp || !stats || !totals || !n_records)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_finish: NULL argument");
	DevParams P;
	if (int rc = check_params(bp, P))
		return rc;
	if (bp->output_type != 0 || bp->without_output != 0 || !bp->lut_prefix_len)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_finish: output_type 0, without_output 0 and a lut_prefix_len above 0 (the bins are ordered by kmc_hip_order_database_device)");
	if (bp->kmer_len != c->k || (bp->both_strands ? 1u : 0u) != c->both)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_finish: kmer_len and both_strands are the session's");
	std::lock_guard<std::mutex> clck(c->mtx);
	if (c->finished)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_finish: the session is finished");
	if (c->parts_running)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_finish: a kmc_hip_count_part call is running");
	const u32 nb = c->n_bins;
	/* 1. the layout: per bin the image (its segments in part order) at a 256-byte aligned base, one pack per non-empty segment — a segment begins at a record start and
	 * any run of whole records is a legal pack (queues.h:376-396) */
	std::vector<u64> bin_base(nb + 1, 0), bin_bytes(nb, 0), bin_kmers(nb, 0), pack_first(nb + 1, 0);
	u64 tot_reads = 0, tot_sk = 0, tot_kmers = 0, tot_bytes = 0, largest_bin = 0, bins_in_use = 0; /* into the session only once nothing can leave it unfinished */
	for (const auto &pt : c->parts) {
		tot_reads += pt.n_reads;
		for (u32 b = 0; b < nb; ++b) {
			bin_bytes[b] += pt.bin_bytes[b];
			bin_kmers[b] += pt.bin_kmers[b];
			tot_sk += pt.bin_sk[b];
			if (pt.bin_bytes[b])
				++pack_first[b + 1];
		}
	}
	for (u32 b = 0; b < nb; ++b) {
		bin_base[b + 1] = bin_base[b] + up256(bin_bytes[b]);
		pack_first[b + 1] += pack_first[b] + 1; /* + the closing entry of the bin's pack-start array */
		tot_kmers += bin_kmers[b];
		largest_bin = bin_kmers[b] > largest_bin ? bin_kmers[b] : largest_bin;
		bins_in_use += bin_kmers[b] ? 1 : 0;
		tot_bytes += bin_bytes[b];
	}
	for (int i = 0; i < 4; ++i)
		stats[i] = 0;
	totals[0] = tot_reads, totals[1] = tot_sk, totals[2] = tot_kmers, totals[3] = tot_bytes;
	*n_records = 0;
	c->bp = *bp;
	if (!tot_kmers) { /* no parts, or not a single k-mer: zeros */
		count_free_store(c);
		c->parts.clear();
		c->finished = c->has_result = true;
		return 0;
	}
	if (int rc = kmc_hip_synchronize(ctx, c->dev)) /* whatever the slots still run */
		return rc;
	const auto t0 = std::chrono::steady_clock::now();
	auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
	DevTemps tmp; /* the bin images and their pack starts: freed when stage 2 is through */
	void *d_img = nullptr, *d_packs = nullptr;
	int rc = 0;
	if ((rc = tmp.alloc(&d_img, (size_t)bin_base[nb] + 256)) || (rc = tmp.alloc(&d_packs, (size_t)pack_first[nb] * 8)))
		return rc;
	{
		std::vector<u64> packs((size_t)pack_first[nb], 0), table, cursor(nb, 0), n_pack(nb, 0);
		for (const auto &pt : c->parts)
			for (u32 b = 0; b < nb; ++b) {
				const u64 len = pt.bin_bytes[b];
				if (!len)
					continue;
				packs[pack_first[b] + n_pack[b]++] = cursor[b];
				const u64 src = (u64)(uintptr_t)(pt.d_recs + pt.bin_off[b]), dst = (u64)(uintptr_t)d_img + bin_base[b] + cursor[b];
				for (u64 o = 0; o < len; o += CG_PIECE_BYTES) { /* long segments (few bins) as several entries: they spread over the grid */
					table.push_back(src + o);
					table.push_back(dst + o);
					table.push_back(len - o < CG_PIECE_BYTES ? len - o : CG_PIECE_BYTES);
				}
				cursor[b] += len;
			}
		for (u32 b = 0; b < nb; ++b)
			packs[pack_first[b] + n_pack[b]] = bin_bytes[b];
		c->n_segments = table.size() / 3;
		c->gathered_bytes = tot_bytes;
		Slot &s = ctx->devs[c->dev]->slot[0];
		std::lock_guard<std::mutex> lck(s.mtx);
		HIPCHK(hipMemcpyAsync(d_packs, packs.data(), packs.size() * 8, hipMemcpyHostToDevice, s.stream));
		HIPCHK(hipMemsetAsync((char *)d_img + bin_base[nb], 0, 256, s.stream)); /* the readable slack behind the last image */
		/* 2. the gather; the store has done its work */
		float ms = 0;
		if ((rc = count_gather_run(s, nullptr, nullptr, table.data(), c->n_segments, &ms)))
			return rc;
		c->seconds[1] = ms / 1e3;
	}
	c->seconds[0] = since(t0) - c->seconds[1];
	const auto t1 = std::chrono::steady_clock::now();
	count_free_store(c);
	c->parts.clear();
	c->largest_bin = largest_bin, c->bins_in_use = bins_in_use;
	c->finished = true; /* the records are gone: whatever fails below, the session can only be closed */
	/* 3. stage 2 in batches of bins whose worst-case outputs fit the arena */
	const u64 rb = kmc_hip_out_rec_bytes(bp), lut_entries = kmc_hip_lut_entries(bp);
	size_t free_b = 0, total_b = 0;
	HIPCHK(hipMemGetInfo(&free_b, &total_b));
	const u64 arena_budget = count_env_mb("KMC_HIP_COUNT_ARENA_MB", (u64)free_b / 4);
	std::vector<std::pair<u32, u32>> batches; /* (first bin, bins) */
	u64 arena_need = 0;
	for (u32 b = 0; b < nb;) {
		u64 sum = 0;
		u32 e = b;
		while (e < nb && (e == b || sum + up256(bin_kmers[e] * rb + 256) <= arena_budget))
			sum += up256(bin_kmers[e++] * rb + 256);
		batches.push_back({b, e - b});
		arena_need = sum > arena_need ? sum : arena_need;
		b = e;
	}
	void *d_arena = nullptr;
	if ((rc = tmp.alloc(&d_arena, (size_t)arena_need)))
		return rc; /* KMC_HIP_ENOMEM: a bin beyond the arena that does not fit on its own either; nothing of it was launched */
	HIPCHK(hipMalloc(&c->d_luts, (size_t)nb * lut_entries * 8 + 256));
	HIPCHK(hipMalloc(&c->d_small, (size_t)nb * 64));
	HIPCHK(hipMemset(c->d_luts, 0, (size_t)nb * lut_entries * 8));
	HIPCHK(hipMemset(c->d_small, 0, (size_t)nb * 64));
	c->descs.assign(nb, kmc_hip_bin_desc{});
	std::vector<u64> small((size_t)nb * 8, 0);
	for (const auto &bt : batches) {
		u64 at = 0;
		for (u32 b = bt.first; b < bt.first + bt.second; ++b) {
			kmc_hip_bin_desc &ds = c->descs[b];
			ds.d_superkmers = (const uint8_t *)d_img + bin_base[b];
			ds.size = bin_bytes[b], ds.n_rec = bin_kmers[b];
			ds.d_pack_start = (const uint64_t *)d_packs + pack_first[b];
			ds.n_packs = pack_first[b + 1] - pack_first[b] - 1;
			ds.d_out = (uint8_t *)d_arena + at;
			ds.out_capacity = bin_kmers[b] * rb;
			ds.d_stats = (uint64_t *)c->d_small + (size_t)b * 8;
			ds.d_out_bytes = ds.d_stats + 4;
			ds.d_lut = (uint64_t *)c->d_luts + (size_t)b * lut_entries;
			at += up256(bin_kmers[b] * rb + 256);
		}
		if ((rc = kmc_hip_process_bins_device(ctx, c->dev, bp, c->descs.data() + bt.first, bt.second, 0)) || (rc = kmc_hip_synchronize(ctx, c->dev)))
			return rc;
		/* each bin's first out_bytes bytes into a tight block; the arena is then free for the next batch */
		HIPCHK(hipMemcpy(small.data() + (size_t)bt.first * 8, (u64 *)c->d_small + (size_t)bt.first * 8, (size_t)bt.second * 64, hipMemcpyDeviceToHost));
		u64 kept = 0;
		for (u32 b = bt.first; b < bt.first + bt.second; ++b)
			kept += small[(size_t)b * 8 + 4];
		void *blk = nullptr;
		HIPCHK(hipMalloc(&blk, (size_t)kept + 256));
		c->results.push_back(blk);
		Slot &s = ctx->devs[c->dev]->slot[0];
		std::lock_guard<std::mutex> lck(s.mtx);
		u64 o = 0;
		for (u32 b = bt.first; b < bt.first + bt.second; ++b) {
			const u64 ob = small[(size_t)b * 8 + 4];
			if (ob)
				HIPCHK(hipMemcpyAsync((uint8_t *)blk + o, c->descs[b].d_out, ob, hipMemcpyDeviceToDevice, s.stream));
			c->descs[b].d_out = (uint8_t *)blk + o;
			c->descs[b].out_capacity = ob;
			o += ob;
		}
		HIPCHK(hipStreamSynchronize(s.stream));
		++c->n_batches;
	}
	/* 4. the results; the bin images go with `tmp` */
	for (u32 b = 0; b < nb; ++b) {
		for (int i = 0; i < 4; ++i)
			stats[i] += small[(size_t)b * 8 + i];
		c->n_records += small[(size_t)b * 8 + 4] / rb;
		c->descs[b].d_superkmers = nullptr, c->descs[b].d_pack_start = nullptr;
	}
	*n_records = c->n_records;
	c->seconds[2] = since(t1);
	c->has_result = true;
	return 0;
}

int kmc_hip_count_order(kmc_hip_ctx *ctx, kmc_hip_count *c, uint32_t out_lut_prefix_len, kmc_hip_db_view *view)
{
	const char *who = "kmc_hip_count_order";
	if (!c)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_order: no session");
	if (int rc = set_dev(ctx, c->dev))
		return rc;
	if (!view)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_order: NULL argument");
	std::lock_guard<std::mutex> clck(c->mtx);
	if (!c->finished)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_order: kmc_hip_count_finish comes first");
	if (int rc = check_prefix_len(who, "out_lut_prefix_len", out_lut_prefix_len, c->k))
		return rc;
	if (!c->has_result)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_order: kmc_hip_count_finish failed, the session holds no result");
	for (void **p : {&c->d_body, &c->d_lut_out})
		if (*p) {
			(void)hipFree(*p);
			*p = nullptr;
		}
	const u32 cs = kmc_hip_counter_size(c->bp.cutoff_max, c->bp.counter_max);
	const u64 cap = c->n_records * ((c->k - out_lut_prefix_len) / 4 + cs), lut_bytes = (u64)8 << (2 * out_lut_prefix_len);
	HIPCHK(hipMalloc(&c->d_body, (size_t)cap + 256));
	HIPCHK(hipMalloc(&c->d_lut_out, (size_t)lut_bytes));
	const auto t0 = std::chrono::steady_clock::now();
	uint64_t n = 0;
	if (c->n_records) {
		if (int rc = kmc_hip_order_database_device(ctx, c->dev, &c->bp, c->descs.data(), c->descs.size(), out_lut_prefix_len, (uint8_t *)c->d_body, cap, (uint64_t *)c->d_lut_out, &n))
			return rc;
	} else
		HIPCHK(hipMemset(c->d_lut_out, 0, (size_t)lut_bytes));
	c->seconds[3] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	view->d_recs = (const uint8_t *)c->d_body;
	view->n_recs = n;
	view->d_lut = (const uint64_t *)c->d_lut_out;
	view->lut_prefix_len = out_lut_prefix_len;
	view->counter_size = cs;
	/* the cutoffs the records were kept under: every record lies inside them, so every kmc_hip_db_* entry takes the view as it is */
	view->cutoff_min = c->bp.cutoff_min;
	view->cutoff_max = c->bp.cutoff_max;
	return 0;
}

int kmc_hip_count_info(kmc_hip_ctx *ctx, kmc_hip_count *c, uint64_t info[6])
{
	(void)ctx;
	if (!c || !info)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_info: NULL argument");
	std::lock_guard<std::mutex> clck(c->mtx);
	info[0] = c->finished ? 0 : c->parts.size(), info[1] = c->chunks.size(), info[2] = c->n_segments, info[3] = c->n_batches;
	info[4] = c->largest_bin, info[5] = c->bins_in_use;
	return 0;
}

int kmc_hip_count_timings(kmc_hip_ctx *ctx, kmc_hip_count *c, double seconds[4])
{
	(void)ctx;
	if (!c || !seconds)
		return fail(KMC_HIP_EINVAL, "kmc_hip_count_timings: NULL argument");
	std::lock_guard<std::mutex> clck(c->mtx);
	for (int i = 0; i < 4; ++i)
		seconds[i] = c->seconds[i];
	return 0;
}

void kmc_hip_count_close(kmc_hip_ctx *ctx, kmc_hip_count *c)
{
	if (!ctx || !c)
		return;
	(void)set_dev(ctx, c->dev);
	{
		std::lock_guard<std::mutex> lck(ctx->mtx);
		auto it = std::find(ctx->counts.begin(), ctx->counts.end(), c);
		if (it == ctx->counts.end())
			return;
		ctx->counts.erase(it);
	}
	(void)hipDeviceSynchronize();
	count_release(c);
}
