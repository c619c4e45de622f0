/* kmc_amd/csrc/host_setops.hip.h — part of kmc_hip.hip (included there, not compiled on its own): set operations between two ordered databases on the device
 * (`kmc_tools simple`; the kernels are in order_db.hip.h). */
namespace {
/* counter bytes of the database CKMC1DbWriter writes (kmc_tools/kmc1_db_writer.h:154): MIN(BYTE_LOG(counter_max), BYTE_LOG(cutoff_max)). kmc_hip_counter_size
 * (defs.h:154-159, the counting side) is the same number except at counter_max == 1, where the counter stores no counter at all and kmc_tools still writes one byte. */
u32 setop_counter_bytes(u64 cutoff_max, u64 counter_max) { return counter_max == 1 ? 1u : counter_bytes(cutoff_max, counter_max); }

template <int SIZE>
int db_set_op_t(Slot &s, u32 k, const kmc_hip_db_view &A, const kmc_hip_db_view &B, const SoOp &op, u32 p_out, u32 cs_out, u64 bound, uint8_t *d_out, u64 *d_lut_out, u64 *h_res /* [6] */)
{
	constexpr int W = SIZE + 1;
	u32 ipt = std::min(env_positive("KMC_HIP_SETOP_IPT", so_default_ipt<SIZE>()), SO_IPT_MAX);
	while (ipt > 1 && so_lds_bytes<SIZE>(ipt, true) > 64 * 1024)
		--ipt;
	const u64 n = A.n_recs + B.n_recs, tile = (u64)SO_THREADS * ipt, n_tiles = (n + tile - 1) / tile;
	if (n_tiles > 0x7FFFFFFFull)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_set_op_device: more tiles than a launch has workgroups");
	/* work area: split[n_tiles + 1] | kept records per tile [n_tiles] | their exclusive sums [n_tiles + 1] (the last one: records written) | tallies [8] */
	const size_t work_words = (size_t)(3 * n_tiles + 2 + 8);
	int rc = 0;
	if ((rc = ensure(s.recA, A.n_recs * W * 8 + 256)) || (rc = ensure(s.recB, B.n_recs * W * 8 + 256)) || (rc = ensure(s.recC, bound * W * 8 + 256)) || (rc = ensure(s.bounds, work_words * 8)))
		return rc;
	u64 *ua = (u64 *)s.recA.p, *ub = (u64 *)s.recB.p, *merged = (u64 *)s.recC.p;
	u64 *split = (u64 *)s.bounds.p, *tile_count = split + n_tiles + 1, *tile_base = tile_count + n_tiles, *stats = tile_base + n_tiles + 1;
	HIPCHK(hipMemsetAsync(tile_base, 0, (n_tiles + 1 + 8) * 8, s.stream)); /* no tile: the total is the 0 written here */
	const kmc_hip_db_view *in[2] = {&A, &B};
	u64 *un[2] = {ua, ub};
	for (int q = 0; q < 2; ++q)
		if (in[q]->n_recs)
			k_db_unpack<SIZE><<<dim3((u32)((in[q]->n_recs + 255) / 256)), dim3(256), 0, s.stream>>>(in[q]->d_recs, in[q]->n_recs, (const u64 *)in[q]->d_lut, 1u << (2 * in[q]->lut_prefix_len), k, in[q]->lut_prefix_len,
			                                                                                   (k - in[q]->lut_prefix_len) / 4, in[q]->counter_size, un[q], in[q]->cutoff_min,
			                                                                                   in[q]->cutoff_max - in[q]->cutoff_min);
	if (n_tiles) {
		k_so_partition<SIZE><<<dim3((u32)((n_tiles + 1 + 255) / 256)), dim3(256), 0, s.stream>>>(ua, A.n_recs, ub, B.n_recs, (u32)tile, n_tiles, split);
		k_so_tile<SIZE, false><<<dim3((u32)n_tiles), dim3(SO_THREADS), so_lds_bytes<SIZE>(ipt, false), s.stream>>>(ua, A.n_recs, ub, B.n_recs, split, ipt, op, (const u64 *)nullptr, tile_count,
		                                                                                                      (u64 *)nullptr, stats);
		k_db_cumsum<<<dim3(1), dim3(256), 0, s.stream>>>(tile_count, n_tiles, tile_base);
		k_so_tile<SIZE, true><<<dim3((u32)n_tiles), dim3(SO_THREADS), so_lds_bytes<SIZE>(ipt, true), s.stream>>>(ua, A.n_recs, ub, B.n_recs, split, ipt, op, tile_base, (u64 *)nullptr, merged, stats);
	}
	HIPCHK(hipMemsetAsync(d_lut_out, 0, (1ull << (2 * p_out)) * 8, s.stream));
	if (bound)
		k_db_pack<SIZE><<<dim3((u32)((bound + 255) / 256)), dim3(256), 0, s.stream>>>(merged, bound, k, p_out, cs_out, d_out, d_lut_out, tile_base + n_tiles);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(s.stream));
	HIPCHK(hipMemcpy(h_res, stats, 5 * 8, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(h_res + 5, tile_base + n_tiles, 8, hipMemcpyDeviceToHost));
	return 0;
}
} // namespace

int kmc_hip_db_set_op_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *a, const kmc_hip_db_view *b, const kmc_hip_db_op *op, uint8_t *d_out,
                             uint64_t out_capacity, uint64_t *d_lut_out, uint64_t *n_kmers, uint64_t stats[6])
{
	const char *who = "kmc_hip_db_set_op_device";
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (!a || !b || !op || !d_out || !d_lut_out || !n_kmers || !stats)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_set_op_device: NULL argument");
	int rc = 0;
	if ((rc = check_view(who, a, kmer_len, 1)) || (rc = check_view(who, b, kmer_len, 1)) || (rc = check_prefix_len(who, "out_lut_prefix_len", op->out_lut_prefix_len, kmer_len)) ||
	    (rc = check_unpacked_width(who, kmer_len)))
		return rc;
	if (op->op >= SO_N_OPS || op->counter_op >= SO_N_CNT)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_set_op_device: unknown operation or counter mode");
	if (op->cutoff_min < 1 || op->counter_max < 1)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_set_op_device: the output's cutoff_min and counter_max must be at least 1");
	if ((rc = kmc_hip_synchronize(ctx, dev))) /* the inputs may come from asynchronous calls on any stream slot */
		return rc;
	Slot &s = ctx->devs[dev]->slot[0];
	std::lock_guard<std::mutex> lck(s.mtx);
	if ((rc = check_view_lut(who, a, 1)) || (rc = check_view_lut(who, b, 1)))
		return rc;
	const u64 na = a->n_recs, nb = b->n_recs;
	const u64 bound = op->op == SO_UNION ? na + nb : op->op == SO_INTERSECT ? std::min(na, nb) : (op->op == SO_KMERS_SUBTRACT || op->op == SO_COUNTERS_SUBTRACT) ? na : nb;
	const u32 cs_out = setop_counter_bytes(op->cutoff_max, op->counter_max), rb_out = (kmer_len - op->out_lut_prefix_len) / 4 + cs_out;
	if (bound * rb_out > out_capacity)
		return fail(KMC_HIP_ECAPACITY, "kmc_hip_db_set_op_device: out_capacity too small for the operation's upper bound (union: both inputs' records; otherwise one input's)");
	const SoOp so = {op->op, op->counter_op, op->cutoff_min, op->counter_max, op->cutoff_max};
	s.timed = false;
	if ((rc = by_words<7>((kmer_len + 31) / 32, [&](auto W) {
		     return db_set_op_t<decltype(W)::value>(s, kmer_len, *a, *b, so, op->out_lut_prefix_len, cs_out, bound, d_out, (u64 *)d_lut_out, (u64 *)stats);
	     })))
		return rc;
	*n_kmers = stats[KMC_HIP_DB_STAT_WRITTEN];
	return finish(s);
}
