/* kmc_amd/csrc/host_smallk_db.hip.h — part of kmc_hip.hip (included there, not compiled on its own): the small-k table (k <= 13) tallied and framed as a database body
 * on the device (CSmallKCompleter::CompleteKMCFormat / CompleteKFFFormat, kmc_core/kb_completer.h:149-378; the kernels are in smallk_db.hip.h). */
namespace {
/* the table an entry works on: the caller's, or the one kmc_hip_smallk_open made on the device — held (AccumHold) until the entry returns, so that a concurrent
 * close cannot free it in front of the kernels; in both cases everything the device's slots have launched is waited for */
int sk_table(kmc_hip_ctx *ctx, int dev, const char *who, const u64 *d_table, u32 kmer_len, AccumHold &hold, const u64 *&table)
{
	const std::string w(who);
	if (kmer_len < 1 || kmer_len > 13)
		return fail(KMC_HIP_EINVAL, w + ": kmer_len 1..13");
	Dev &d = *ctx->devs[dev];
	table = d_table;
	if (!d_table) {
		std::lock_guard<std::mutex> lck(d.smallk.mtx);
		if (!d.smallk.p)
			return fail(KMC_HIP_EINVAL, w + ": d_table is NULL and no small-k table is open on this device (kmc_hip_smallk_open)");
		if (d.smallk.par[0] != kmer_len)
			return fail(KMC_HIP_EINVAL, w + ": the open table has another kmer_len");
		table = (const u64 *)d.smallk.p;
		hold.take(d.smallk);
	}
	return kmc_hip_synchronize(ctx, dev); /* the kmc_hip_smallk_part calls in flight, as _read waits for them */
}
int sk_check_cutoffs(const char *who, u64 cutoff_min, u64 cutoff_max)
{
	if (cutoff_min < 1 || cutoff_max < cutoff_min)
		return fail(KMC_HIP_EINVAL, std::string(who) + ": cutoff_min must be at least 1 and cutoff_max at least cutoff_min");
	return 0;
}

struct SkGeo {
	u32 ipt;
	bool pair; /* 16-byte loads: an even ipt and a table aligned to 16 bytes */
	u64 n, n_tiles;
	u64 *tile_count, *tile_base, *stats; /* [n_tiles] | [n_tiles + 1] (the last one: kept entries) | [4] */
};
int sk_plan(const u64 *table, u32 kmer_len, DevTemps &tmp, SkGeo &g)
{
	g.ipt = std::min(env_positive("KMC_HIP_SMALLK_IPT", SK_IPT_DEFAULT), SK_IPT_MAX); /* tests: 1 and 3, so that small tables cross tile seams */
	g.pair = g.ipt % 2 == 0 && ((size_t)table & 15) == 0;
	g.n = (u64)1 << (2 * kmer_len);
	const u64 tile = (u64)SK_THREADS * g.ipt;
	g.n_tiles = (g.n + tile - 1) / tile; /* at most 4^13 / 256 */
	void *p = nullptr;
	if (int rc = tmp.alloc(&p, (size_t)(2 * g.n_tiles + 1 + 4) * 8))
		return rc;
	g.tile_count = (u64 *)p;
	g.tile_base = g.tile_count + g.n_tiles;
	g.stats = g.tile_base + g.n_tiles + 1;
	return 0;
}
/* k_sk_tally and the scan of its counts; h_stats: unique, below, above, kept */
int sk_tally(Slot &s, const u64 *table, const SkGeo &g, const SkCut &cut, u64 *h_stats)
{
	HIPCHK(hipMemsetAsync(g.stats, 0, 4 * 8, s.stream));
	const u32 wgs = (u32)std::min<u64>(g.n_tiles, env_positive("KMC_HIP_SMALLK_TALLY_WGS", SK_TALLY_WGS)); /* tests: 1 and 3, so that a workgroup walks many tiles */
	if (g.pair)
		k_sk_tally<true><<<dim3(wgs), dim3(SK_THREADS), 0, s.stream>>>(table, g.n, g.ipt, (u32)g.n_tiles, cut, g.tile_count, g.stats);
	else
		k_sk_tally<false><<<dim3(wgs), dim3(SK_THREADS), 0, s.stream>>>(table, g.n, g.ipt, (u32)g.n_tiles, cut, g.tile_count, g.stats);
	k_db_cumsum<<<dim3(1), dim3(256), 0, s.stream>>>(g.tile_count, g.n_tiles, g.tile_base);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(s.stream));
	HIPCHK(hipMemcpy(h_stats, g.stats, 3 * 8, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(h_stats + SK_ST_KEPT, g.tile_base + g.n_tiles, 8, hipMemcpyDeviceToHost));
	return 0;
}
int sk_emit(Slot &s, const u64 *table, const SkGeo &g, const SkCut &cut, const SkFrame &f, uint8_t *d_out, u64 *d_lut)
{
	const size_t lds = sk_emit_lds_bytes(SK_THREADS * g.ipt, f.key_bytes + f.cnt_bytes);
	if (g.pair)
		k_sk_emit<true><<<dim3((u32)g.n_tiles), dim3(SK_THREADS), lds, s.stream>>>(table, g.n, g.ipt, cut, f, g.tile_base, d_out, d_lut);
	else
		k_sk_emit<false><<<dim3((u32)g.n_tiles), dim3(SK_THREADS), lds, s.stream>>>(table, g.n, g.ipt, cut, f, g.tile_base, d_out, d_lut);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(s.stream));
	return 0;
}
} // namespace

int kmc_hip_smallk_tally(kmc_hip_ctx *ctx, int dev, const uint64_t *d_table, uint32_t kmer_len, uint64_t cutoff_min, uint64_t cutoff_max, uint64_t stats[4])
{
	const char *who = "kmc_hip_smallk_tally";
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (!stats)
		return fail(KMC_HIP_EINVAL, "kmc_hip_smallk_tally: NULL argument");
	if (int rc = sk_check_cutoffs(who, cutoff_min, cutoff_max))
		return rc;
	AccumHold hold;
	const u64 *table = nullptr;
	if (int rc = sk_table(ctx, dev, who, (const u64 *)d_table, kmer_len, hold, table))
		return rc;
	Slot &s = ctx->devs[dev]->slot[0];
	std::lock_guard<std::mutex> lck(s.mtx);
	DevTemps tmp;
	SkGeo g;
	if (int rc = sk_plan(table, kmer_len, tmp, g))
		return rc;
	s.timed = false;
	if (int rc = sk_tally(s, table, g, SkCut{cutoff_min, cutoff_max, ~0ull}, (u64 *)stats))
		return rc;
	return finish(s);
}

int kmc_hip_smallk_view_device(kmc_hip_ctx *ctx, int dev, const uint64_t *d_table, uint32_t kmer_len, uint32_t both_strands, uint64_t cutoff_min, uint64_t cutoff_max,
                               uint64_t counter_max, uint32_t framing, uint32_t out_lut_prefix_len, uint32_t data_size, uint8_t *d_out, uint64_t out_capacity,
                               uint64_t *d_lut_out, kmc_hip_db_view *view, uint64_t *n_kmers, uint64_t stats[4])
{
	const char *who = "kmc_hip_smallk_view_device";
	const std::string w(who);
	(void)both_strands; /* a table holds canonical k-mers or forward ones: the body is the same function of it; the caller's header says which */
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (framing > SK_FRAME_KFF)
		return fail(KMC_HIP_EINVAL, w + ": framing 0 (KMC1) or 1 (KFF)");
	if (!d_out || !n_kmers || !stats || (framing == SK_FRAME_KMC1 && (!d_lut_out || !view)))
		return fail(KMC_HIP_EINVAL, w + ": NULL argument (d_out, n_kmers, stats; KMC1: d_lut_out and view)");
	if (kmer_len < 1 || kmer_len > 13)
		return fail(KMC_HIP_EINVAL, w + ": kmer_len 1..13");
	if (int rc = sk_check_cutoffs(who, cutoff_min, cutoff_max))
		return rc;
	const u32 cs = counter_bytes(cutoff_max, counter_max);
	if (cs < 1 || cs > 4 || std::min(cutoff_max, counter_max) > 0xFFFFFFFFull) /* a kept count is at most the smaller of the two: it must fit the four bytes */
		return fail(KMC_HIP_EINVAL, w + ": kmc_hip_counter_size(cutoff_max, counter_max) must be 1..4 (counter_max 1 stores no counter; a database has at most four counter bytes)");
	const u32 p = out_lut_prefix_len;
	SkFrame f = {};
	if (framing == SK_FRAME_KMC1) {
		if (p < 1 || p > kmer_len || (kmer_len - p) % 4)
			return fail(KMC_HIP_EINVAL, w + ": out_lut_prefix_len must be 1..kmer_len with (kmer_len - out_lut_prefix_len) a multiple of 4");
		f = SkFrame{(kmer_len - p) / 4, cs, 0u, 2 * (kmer_len - p)};
	} else {
		if (data_size < cs || data_size > 4)
			return fail(KMC_HIP_EINVAL, w + ": data_size must be the counter size..4");
		f = SkFrame{(kmer_len + 3) / 4, data_size, 1u, 0u};
	}
	AccumHold hold;
	const u64 *table = nullptr;
	if (int rc = sk_table(ctx, dev, who, (const u64 *)d_table, kmer_len, hold, table))
		return rc;
	Slot &s = ctx->devs[dev]->slot[0];
	std::lock_guard<std::mutex> lck(s.mtx);
	DevTemps tmp;
	SkGeo g;
	if (int rc = sk_plan(table, kmer_len, tmp, g))
		return rc;
	const SkCut cut = {cutoff_min, cutoff_max, counter_max};
	s.timed = false;
	u64 h[4] = {0, 0, 0, 0};
	if (int rc = sk_tally(s, table, g, cut, h))
		return rc;
	const u32 rb = f.key_bytes + f.cnt_bytes;
	if (h[SK_ST_KEPT] > out_capacity / rb) /* nothing has been written yet */
		return fail(KMC_HIP_ECAPACITY, w + ": out_capacity below kept x record bytes (kmc_hip_smallk_tally gives kept)");
	if (int rc = sk_emit(s, table, g, cut, f, d_out, framing == SK_FRAME_KMC1 ? (u64 *)d_lut_out : nullptr))
		return rc;
	for (int q = 0; q < 4; ++q)
		stats[q] = h[q];
	*n_kmers = h[SK_ST_KEPT];
	if (view && framing == SK_FRAME_KMC1) {
		view->d_recs = d_out;
		view->n_recs = h[SK_ST_KEPT];
		view->d_lut = d_lut_out;
		view->lut_prefix_len = p;
		view->counter_size = cs;
		view->cutoff_min = (uint32_t)std::min<u64>(cutoff_min, 0xFFFFFFFFull);
		view->cutoff_max = cutoff_max;
	}
	return finish(s);
}
