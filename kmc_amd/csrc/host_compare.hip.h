/* kmc_amd/csrc/host_compare.hip.h — part of kmc_hip.hip (included there, not compiled on its own): two ordered databases compared on the device
 * (`kmc_tools compare`; the kernels are in order_db.hip.h). */
namespace {
template <int SIZE> int db_compare_t(Slot &s, u32 k, const kmc_hip_db_view &A, const kmc_hip_db_view &B, u64 *h_res /* [8] */)
{
	constexpr int W = SIZE + 1;
	const u32 steps_log2 = std::min(31u - (u32)__builtin_clz(env_positive("KMC_HIP_COMPARE_STEPS", 1u << DC_STEPS_LOG2)), DC_STEPS_LOG2_MAX); /* rounded down to a power of two */
	const u32 tile_shift = steps_log2 + (31u - (u32)__builtin_clz((u32)DC_THREADS)), reversed = env_positive("KMC_HIP_COMPARE_REVERSED", 0) ? 1u : 0u;
	static_assert((DC_THREADS & (DC_THREADS - 1)) == 0, "a tile of k_db_compare is a power of two of words");
	const u64 ctile = (u64)TR_THREADS * TR_REDUCE_IPT;
	const kmc_hip_db_view *in[2] = {&A, &B};
	DevTemps tmp;
	u64 *unp[2] = {nullptr, nullptr}, *tile_count[2], *tile_base[2], *stats[2], n_tiles[2];
	DcInput di[2];
	int rc = 0;
	for (int q = 0; q < 2; ++q) {
		const u64 n = in[q]->n_recs;
		n_tiles[q] = (n + ctile - 1) / ctile;
		if (n_tiles[q] > 0x7FFFFFFFull)
			return fail(KMC_HIP_EINVAL, "kmc_hip_db_compare_device: more tiles than a launch has workgroups");
		/* work area: kept records per tile [n_tiles] | their exclusive sums [n_tiles + 1] (the last one: present records) | tallies [8] */
		if ((rc = tmp.alloc((void **)&unp[q], n * W * 8 + 256)) || (rc = tmp.alloc((void **)&tile_count[q], (size_t)(2 * n_tiles[q] + 1 + 8) * 8)))
			return rc;
		tile_base[q] = tile_count[q] + n_tiles[q], stats[q] = tile_base[q] + n_tiles[q] + 1;
		HIPCHK(hipMemsetAsync(tile_base[q], 0, (n_tiles[q] + 1 + 8) * 8, s.stream));
		if (n) {
			/* every record present for k_db_unpack: k_tr_compact applies the input's cutoffs itself, and tallies them */
			const TrCut cut = {in[q]->cutoff_min, in[q]->cutoff_max, 0u, ~0ull, ~0u, 0u};
			k_db_unpack<SIZE><<<dim3((u32)((n + 255) / 256)), dim3(256), 0, s.stream>>>(in[q]->d_recs, n, (const u64 *)in[q]->d_lut, 1u << (2 * in[q]->lut_prefix_len), k, in[q]->lut_prefix_len,
			                                                                           (k - in[q]->lut_prefix_len) / 4, in[q]->counter_size, unp[q], 0u, ~0ull);
			k_tr_compact<SIZE, false><<<dim3((u32)n_tiles[q]), dim3(TR_THREADS), 0, s.stream>>>(unp[q], n, cut, (const u64 *)nullptr, tile_count[q], (u64 *)nullptr, stats[q]);
		}
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(s.stream));
	for (int q = 0; q < 2; ++q) {
		const u64 n = in[q]->n_recs;
		u64 cut_in = 0;
		HIPCHK(hipMemcpy(&cut_in, stats[q] + TR_ST_CUT_IN, 8, hipMemcpyDeviceToHost));
		if (cut_in > n)
			return fail(KMC_HIP_EINTERNAL, "kmc_hip_db_compare_device: more records cut than the input holds");
		di[q] = DcInput{unp[q], n - cut_in, unp[q], n, nullptr, n_tiles[q], in[q]->cutoff_min, in[q]->cutoff_max};
		if (cut_in) { /* the input lost records: the present ones, in their order, in an array of their own */
			u64 *dense = nullptr;
			const TrCut cut = {in[q]->cutoff_min, in[q]->cutoff_max, 0u, ~0ull, ~0u, 0u};
			if ((rc = tmp.alloc((void **)&dense, (n - cut_in) * W * 8 + 256)))
				return rc;
			k_db_cumsum<<<dim3(1), dim3(256), 0, s.stream>>>(tile_count[q], n_tiles[q], tile_base[q]);
			k_tr_compact<SIZE, true><<<dim3((u32)n_tiles[q]), dim3(TR_THREADS), 0, s.stream>>>(unp[q], n, cut, tile_base[q], (u64 *)nullptr, dense, stats[q]);
			di[q].dense = dense, di[q].tile_base = tile_base[q];
		}
	}
	u64 *d_first = nullptr; /* the minimum | result [8] */
	if ((rc = tmp.alloc((void **)&d_first, 9 * 8)))
		return rc;
	HIPCHK(hipMemsetAsync(d_first, 0xFF, 8, s.stream));
	const u64 n_words = std::min(di[0].n, di[1].n) * W, n_ctiles = (n_words + (1ull << tile_shift) - 1) >> tile_shift;
	if (n_ctiles > 0x7FFFFFFFull)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_compare_device: more tiles than a launch has workgroups");
	if (n_ctiles)
		k_db_compare<SIZE><<<dim3((u32)n_ctiles), dim3(DC_THREADS), 0, s.stream>>>(di[0].dense, di[1].dense, n_words, tile_shift, reversed, d_first);
	k_db_compare_finish<SIZE><<<dim3(1), dim3(TR_THREADS), 0, s.stream>>>(di[0], di[1], d_first, d_first + 1);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(s.stream));
	HIPCHK(hipMemcpy(h_res, d_first + 1, 8 * 8, hipMemcpyDeviceToHost));
	return 0;
}
} // namespace

int kmc_hip_db_compare_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *a, const kmc_hip_db_view *b, uint64_t result[8])
{
	const char *who = "kmc_hip_db_compare_device";
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (!a || !b || !result)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_compare_device: NULL argument");
	int rc = 0;
	if ((rc = check_view(who, a, kmer_len, 1)) || (rc = check_view(who, b, kmer_len, 1)) || (rc = check_unpacked_width(who, kmer_len)))
		return rc;
	if ((rc = kmc_hip_synchronize(ctx, dev))) /* the inputs may come from asynchronous calls on any stream slot */
		return rc;
	Slot &s = ctx->devs[dev]->slot[0];
	std::lock_guard<std::mutex> lck(s.mtx);
	if ((rc = check_view_lut(who, a, 1)) || (rc = check_view_lut(who, b, 1)))
		return rc;
	s.timed = false;
	if ((rc = by_words<7>((kmer_len + 31) / 32, [&](auto W) { return db_compare_t<decltype(W)::value>(s, kmer_len, *a, *b, (u64 *)result); })))
		return rc;
	return finish(s);
}
