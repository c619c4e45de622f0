/* kmc_amd/csrc/host_query.hip.h — part of kmc_hip.hip (included there, not compiled on its own): the reads of a file against an ordered database on the device
 * (`kmc_tools filter`; the kernels are in order_db.hip.h). */
namespace {
template <int SIZE>
int db_query_lookup_t(Slot &s, const kmc_hip_db_view &db, u32 k, u32 both, const uint8_t *d_seq, u64 n_bytes, u32 *d_counters, u64 *d_stats)
{
	u32 ipt = std::min(env_positive("KMC_HIP_QUERY_IPT", dq_default_ipt<SIZE>()), DQ_IPT_MAX);
	while (ipt > 1 && dq_lds_bytes(ipt, k) > 64 * 1024)
		--ipt;
	const u64 tile = (u64)DQ_THREADS * ipt, n_tiles = (n_bytes + tile - 1) / tile;
	if (n_tiles > 0x7FFFFFFFull)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_query_reads_device: more tiles than a launch has workgroups");
	k_dbq_lookup<SIZE><<<dim3((u32)n_tiles), dim3(DQ_THREADS), dq_lds_bytes(ipt, k), s.stream>>>(d_seq, n_bytes, k, both, db.d_recs, db.n_recs, (const u64 *)db.d_lut, db.lut_prefix_len, db.counter_size,
	                                                                                         db.cutoff_min, db.cutoff_max, ipt, d_counters, d_stats);
	return 0;
}
} // namespace

int kmc_hip_db_query_reads_device(kmc_hip_ctx *ctx, int dev, const kmc_hip_db_view *db, uint32_t kmer_len, uint32_t both_strands, const uint8_t *d_seq, uint64_t n_bytes,
                                  const uint64_t *d_read_off, uint64_t n_reads, uint32_t threshold, uint32_t *d_counters, uint32_t *d_n_valid, uint32_t *d_trim_len,
                                  uint8_t *d_masked, uint64_t stats[4])
{
	const char *who = "kmc_hip_db_query_reads_device";
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (!db || !stats || (n_bytes && (!d_seq || !d_counters)))
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_query_reads_device: NULL argument");
	if (!d_read_off && (n_reads || d_n_valid || d_trim_len || d_masked))
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_query_reads_device: NULL argument (reads or per-read outputs without a table of read offsets)");
	if (int rc = check_view(who, db, kmer_len, 1))
		return rc;
	if (int rc = check_unpacked_width(who, kmer_len))
		return rc;
	if (int rc = kmc_hip_synchronize(ctx, dev)) /* the database may come from asynchronous calls on any stream slot */
		return rc;
	Slot &s = ctx->devs[dev]->slot[0];
	std::lock_guard<std::mutex> lck(s.mtx);
	if (int rc = check_view_lut(who, db, 1))
		return rc;
	for (int q = 0; q < 4; ++q)
		stats[q] = 0;
	/* work area: the four tallies [8] | non-zero bits, low bits, their counts per 64 positions [4 x chunks] | the counts' prefix sums [2 x (chunks + 1)] */
	const u64 n_chunks = (n_bytes + 63) / 64;
	if (n_chunks > 0x7FFFFFFFull * 4)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_query_reads_device: more positions than a launch has threads");
	if (int rc = ensure(s.bounds, (size_t)(8 + 6 * n_chunks + 2) * 8))
		return rc;
	u64 *d_stats = (u64 *)s.bounds.p, *nz_bits = d_stats + 8, *low_bits = nz_bits + n_chunks, *nz_cnt = low_bits + n_chunks, *low_cnt = nz_cnt + n_chunks, *nz_sum = low_cnt + n_chunks,
	    *low_sum = nz_sum + n_chunks + 1;
	HIPCHK(hipMemsetAsync(d_stats, 0, 8 * 8, s.stream));
	s.timed = false;
	if (n_bytes)
		if (int rc = by_words<7>((kmer_len + 31) / 32, [&](auto W) { return db_query_lookup_t<decltype(W)::value>(s, *db, kmer_len, both_strands ? 1u : 0u, d_seq, n_bytes, d_counters, d_stats); }))
			return rc;
	if (n_reads) {
		const u64 n_read_blocks = (n_reads + 255) / 256;
		if (n_read_blocks > 0x7FFFFFFFull)
			return fail(KMC_HIP_EINVAL, "kmc_hip_db_query_reads_device: more reads than a launch has threads");
		if (n_chunks) {
			k_dbq_reads<0><<<dim3((u32)((n_chunks + 3) / 4)), dim3(256), 0, s.stream>>>(d_seq, n_bytes, kmer_len, (const u64 *)d_read_off, n_reads, threshold, d_counters, nz_bits, low_bits, nz_cnt, low_cnt, (u32 *)nullptr,
			                                                                          (u32 *)nullptr, (uint8_t *)nullptr, err_ptr(s));
			k_db_cumsum<<<dim3(1), dim3(256), 0, s.stream>>>(nz_cnt, n_chunks, nz_sum);
			k_db_cumsum<<<dim3(1), dim3(256), 0, s.stream>>>(low_cnt, n_chunks, low_sum);
		} else
			HIPCHK(hipMemsetAsync(nz_sum, 0, 2 * 8, s.stream)); /* nz_sum[0], low_sum[0]: every read is then an error of its offsets */
		k_dbq_reads<1><<<dim3((u32)n_read_blocks), dim3(256), 0, s.stream>>>(d_seq, n_bytes, kmer_len, (const u64 *)d_read_off, n_reads, threshold, d_counters, nz_bits, low_bits, nz_sum, low_sum, d_n_valid, d_trim_len,
		                                                                  (uint8_t *)nullptr, err_ptr(s));
		if (d_masked && n_bytes)
			k_dbq_reads<2><<<dim3((u32)((n_bytes + 255) / 256)), dim3(256), 0, s.stream>>>(d_seq, n_bytes, kmer_len, (const u64 *)d_read_off, n_reads, threshold, d_counters, nz_bits, low_bits, nz_sum, low_sum,
			                                                                            (u32 *)nullptr, (u32 *)nullptr, d_masked, err_ptr(s));
	} else if (d_masked && n_bytes)
		HIPCHK(hipMemcpyAsync(d_masked, d_seq, n_bytes, hipMemcpyDeviceToDevice, s.stream)); /* no reads: nothing to mask */
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(s.stream));
	HIPCHK(hipMemcpy(stats, d_stats, 4 * 8, hipMemcpyDeviceToHost));
	u32 err = 0; /* finish(s), with what KERR_CORRUPT means in this entry in front of err_to_code's words for it */
	if (int rc = read_and_clear_sticky(s, err))
		return rc;
	if (err & KERR_CORRUPT)
		return fail(KMC_HIP_ECORRUPT, "kmc_hip_db_query_reads_device: the read offsets do not ascend, end behind n_bytes, or a read is not followed by an invalid symbol");
	return err_to_code(err);
}
