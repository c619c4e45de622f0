/* kmc_amd/csrc/host_transform.hip.h — part of kmc_hip.hip (included there, not compiled on its own): one database transformed on the device
 * (`kmc_tools transform`: reduce / compact / set_counts / sort, histogram, dump; the kernels are in order_db.hip.h). */
namespace {
template <int SIZE>
int db_reduce_t(Slot &s, u32 k, const kmc_hip_db_view &db, const TrCut &cut, u32 p_out, u32 cs_out, uint8_t *d_out, u64 *d_lut_out, u64 *h_res /* [4] */)
{
	constexpr int W = SIZE + 1;
	const u64 n = db.n_recs, tile = (u64)TR_THREADS * TR_REDUCE_IPT, n_tiles = (n + tile - 1) / tile;
	if (n_tiles > 0x7FFFFFFFull)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_reduce_device: more tiles than a launch has workgroups");
	/* work area: kept records per tile [n_tiles] | their exclusive sums [n_tiles + 1] (the last one: records written) | tallies [8] */
	int rc = 0;
	if ((rc = ensure(s.recA, n * W * 8 + 256)) || (rc = ensure(s.recC, n * W * 8 + 256)) || (rc = ensure(s.bounds, (size_t)(2 * n_tiles + 1 + 8) * 8)))
		return rc;
	u64 *unpacked = (u64 *)s.recA.p, *kept = (u64 *)s.recC.p;
	u64 *tile_count = (u64 *)s.bounds.p, *tile_base = tile_count + n_tiles, *stats = tile_base + n_tiles + 1;
	HIPCHK(hipMemsetAsync(tile_base, 0, (n_tiles + 1 + 8) * 8, s.stream)); /* no tile: the total is the 0 written here */
	HIPCHK(hipMemsetAsync(d_lut_out, 0, (1ull << (2 * p_out)) * 8, s.stream));
	if (n) {
		/* every record present for k_db_unpack: k_tr_compact applies the input's cutoffs itself, and tallies them */
		k_db_unpack<SIZE><<<dim3((u32)((n + 255) / 256)), dim3(256), 0, s.stream>>>(db.d_recs, n, (const u64 *)db.d_lut, 1u << (2 * db.lut_prefix_len), k, db.lut_prefix_len, (k - db.lut_prefix_len) / 4,
		                                                                           db.counter_size, unpacked, 0u, ~0ull);
		k_tr_compact<SIZE, false><<<dim3((u32)n_tiles), dim3(TR_THREADS), 0, s.stream>>>(unpacked, n, cut, (const u64 *)nullptr, tile_count, (u64 *)nullptr, stats);
		k_db_cumsum<<<dim3(1), dim3(256), 0, s.stream>>>(tile_count, n_tiles, tile_base);
		k_tr_compact<SIZE, true><<<dim3((u32)n_tiles), dim3(TR_THREADS), 0, s.stream>>>(unpacked, n, cut, tile_base, (u64 *)nullptr, kept, stats);
		k_db_pack<SIZE><<<dim3((u32)((n + 255) / 256)), dim3(256), 0, s.stream>>>(kept, n, k, p_out, cs_out, d_out, d_lut_out, tile_base + n_tiles);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(s.stream));
	HIPCHK(hipMemcpy(h_res, stats, 3 * 8, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(h_res + 3, tile_base + n_tiles, 8, hipMemcpyDeviceToHost));
	return 0;
}
} // namespace

int kmc_hip_db_reduce_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *db, uint32_t cutoff_min, uint64_t cutoff_max, uint32_t counter_max,
                             uint32_t counter_value, uint32_t out_lut_prefix_len, uint8_t *d_out, uint64_t out_capacity, uint64_t *d_lut_out, uint64_t *n_kmers, uint64_t stats[4])
{
	const char *who = "kmc_hip_db_reduce_device";
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (!d_out || !d_lut_out || !n_kmers || !stats)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_reduce_device: NULL argument");
	if (int rc = check_view(who, db, kmer_len, 1))
		return rc;
	const u32 p = out_lut_prefix_len;
	if (int rc = check_prefix_len(who, "out_lut_prefix_len", p, kmer_len))
		return rc;
	if (int rc = check_unpacked_width(who, kmer_len))
		return rc;
	if (cutoff_min < 1 || counter_max < 1)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_reduce_device: the output's cutoff_min and counter_max must be at least 1");
	if (int rc = kmc_hip_synchronize(ctx, dev)) /* the input may come from asynchronous calls on any stream slot */
		return rc;
	Slot &s = ctx->devs[dev]->slot[0];
	std::lock_guard<std::mutex> lck(s.mtx);
	if (int rc = check_view_lut(who, db, 1))
		return rc;
	/* kmc1_db_writer.h:154-156 */
	const u32 cs_out = counter_value ? setop_counter_bytes(counter_value, counter_value) : setop_counter_bytes(cutoff_max, counter_max), rb_out = (kmer_len - p) / 4 + cs_out;
	if (db->n_recs * rb_out > out_capacity)
		return fail(KMC_HIP_ECAPACITY, "kmc_hip_db_reduce_device: out_capacity too small for the input's records");
	const TrCut cut = {db->cutoff_min, db->cutoff_max, cutoff_min, cutoff_max, counter_max, counter_value};
	s.timed = false;
	if (int rc = by_words<7>((kmer_len + 31) / 32, [&](auto W) { return db_reduce_t<decltype(W)::value>(s, kmer_len, *db, cut, p, cs_out, d_out, (u64 *)d_lut_out, (u64 *)stats); }))
		return rc;
	*n_kmers = stats[KMC_HIP_DBT_STAT_WRITTEN];
	return finish(s);
}

int kmc_hip_db_histogram_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *db, uint32_t n_lut_segments, uint32_t cutoff_min, uint64_t cutoff_max,
                                uint64_t *d_hist, uint64_t stats[3])
{
	const char *who = "kmc_hip_db_histogram_device";
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (!d_hist || !stats)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_histogram_device: NULL argument");
	if (int rc = check_view(who, db, kmer_len, n_lut_segments))
		return rc;
	if (cutoff_min < 1 || cutoff_max < cutoff_min || cutoff_max > 0xFFFFFFFFull)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_histogram_device: 1 <= cutoff_min <= cutoff_max < 2^32");
	if (int rc = kmc_hip_synchronize(ctx, dev))
		return rc;
	Slot &s = ctx->devs[dev]->slot[0];
	std::lock_guard<std::mutex> lck(s.mtx);
	if (int rc = check_view_lut(who, db, n_lut_segments))
		return rc;
	if (int rc = ensure(s.bounds, 8 * 8))
		return rc;
	u64 *d_stats = (u64 *)s.bounds.p;
	const u64 n_bins = cutoff_max - cutoff_min + 1, n = db->n_recs;
	HIPCHK(hipMemsetAsync(d_stats, 0, 8 * 8, s.stream));
	HIPCHK(hipMemsetAsync(d_hist, 0, n_bins * 8, s.stream));
	s.timed = false;
	if (n) {
		const u32 groups = (u32)std::min<u64>((n + TR_THREADS - 1) / TR_THREADS, TR_HIST_MAX_GROUPS), sbytes = (kmer_len - db->lut_prefix_len) / 4;
		if (n_bins <= TR_HIST_LDS_BINS)
			k_tr_hist<true><<<dim3(groups), dim3(TR_THREADS), (size_t)n_bins * 4, s.stream>>>(db->d_recs, n, sbytes, db->counter_size, db->cutoff_min, db->cutoff_max, cutoff_min, cutoff_max, (u32)n_bins,
			                                                                               (u64 *)d_hist, d_stats);
		else
			k_tr_hist<false><<<dim3(groups), dim3(TR_THREADS), 0, s.stream>>>(db->d_recs, n, sbytes, db->counter_size, db->cutoff_min, db->cutoff_max, cutoff_min, cutoff_max, 0u, (u64 *)d_hist, d_stats);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(s.stream));
	HIPCHK(hipMemcpy(stats, d_stats, 3 * 8, hipMemcpyDeviceToHost));
	return finish(s);
}

int kmc_hip_db_dump_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *db, uint32_t n_lut_segments, uint64_t first, uint64_t count, uint32_t cutoff_min,
                           uint64_t cutoff_max, uint32_t counter_max, uint8_t *d_text, uint64_t text_capacity, uint64_t *n_bytes, uint64_t stats[4])
{
	const char *who = "kmc_hip_db_dump_device";
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (!n_bytes || !stats || (count && !d_text))
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_dump_device: NULL argument");
	if (int rc = check_view(who, db, kmer_len, n_lut_segments))
		return rc;
	if (cutoff_min < 1 || counter_max < 1)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_dump_device: the output's cutoff_min and counter_max must be at least 1");
	if (first > db->n_recs || count > db->n_recs - first)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_dump_device: the record range ends behind the database");
	if (kmer_len + TR_REC_EXTRA > TR_IMAGE_MAX)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_dump_device: kmer_len too large for a tile of one record");
	if (count > text_capacity / (kmer_len + TR_REC_EXTRA))
		return fail(KMC_HIP_ECAPACITY, "kmc_hip_db_dump_device: text_capacity below count x (kmer_len + 12)");
	if (int rc = kmc_hip_synchronize(ctx, dev))
		return rc;
	Slot &s = ctx->devs[dev]->slot[0];
	std::lock_guard<std::mutex> lck(s.mtx);
	if (int rc = check_view_lut(who, db, n_lut_segments))
		return rc;
	u32 tile = env_positive("KMC_HIP_DUMP_TILE", tr_default_tile(kmer_len)); /* records of a tile (tests: a few hundred, so that a small database crosses tile seams) */
	tile = std::max(1u, std::min(tile, TR_IMAGE_MAX / (kmer_len + TR_REC_EXTRA)));
	const u64 n_tiles = (count + tile - 1) / tile;
	if (n_tiles > 0x7FFFFFFFull)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_dump_device: more tiles than a launch has workgroups");
	/* work area: text bytes per tile [n_tiles] | their exclusive sums [n_tiles + 1] (the last one: bytes written) | tallies [8] */
	if (int rc = ensure(s.bounds, (size_t)(2 * n_tiles + 1 + 8) * 8))
		return rc;
	u64 *tile_bytes = (u64 *)s.bounds.p, *tile_base = tile_bytes + n_tiles, *d_stats = tile_base + n_tiles + 1;
	HIPCHK(hipMemsetAsync(tile_base, 0, (n_tiles + 1 + 8) * 8, s.stream));
	s.timed = false;
	if (n_tiles) {
		const TrDump d = {kmer_len, db->lut_prefix_len, (kmer_len - db->lut_prefix_len) / 4, db->counter_size, (u32)((u64)n_lut_segments << (2 * db->lut_prefix_len)), tile};
		const TrCut cut = {db->cutoff_min, db->cutoff_max, cutoff_min, cutoff_max, counter_max, 0u};
		k_tr_dump<false><<<dim3((u32)n_tiles), dim3(TR_THREADS), 0, s.stream>>>(db->d_recs, (const u64 *)db->d_lut, first, count, d, cut, (const u64 *)nullptr, tile_bytes, (uint8_t *)nullptr, d_stats);
		k_db_cumsum<<<dim3(1), dim3(256), 0, s.stream>>>(tile_bytes, n_tiles, tile_base);
		k_tr_dump<true><<<dim3((u32)n_tiles), dim3(TR_THREADS), tr_dump_lds_bytes(tile, kmer_len), s.stream>>>(db->d_recs, (const u64 *)db->d_lut, first, count, d, cut, tile_base, (u64 *)nullptr, d_text, d_stats);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(s.stream));
	HIPCHK(hipMemcpy(stats, d_stats, 3 * 8, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(n_bytes, tile_base + n_tiles, 8, hipMemcpyDeviceToHost));
	/* records written = the range's records less the three kinds that are not */
	stats[KMC_HIP_DBT_STAT_WRITTEN] = count - stats[0] - stats[1] - stats[2];
	return finish(s);
}
