/* kmc_amd/csrc/host_expr.hip.h — part of kmc_hip.hip (included there, not compiled on its own): a set expression over several ordered databases on the device
 * (`kmc_tools complex`; the kernels are in order_db.hip.h). */
namespace {
struct ExprPlan {
	CxProg prog;
	u32 leaf_view[CX_MAX_LEAVES];
	u32 n_leaves = 0;
	u64 bound = 0; /* the tree's own upper bound of records */
};

/* the postfix program checked on a stack of upper bounds: union l + r, intersect min(l, r), the subtractions l */
int expr_plan(const kmc_hip_db_view *views, u32 n_views, const kmc_hip_db_expr_step *steps, u32 n_steps, ExprPlan &pl)
{
	u64 stack[CX_MAX_LEAVES];
	u32 depth = 0;
	if (n_steps == 0 || n_steps > CX_MAX_STEPS)
		return fail(KMC_HIP_EINVAL, n_steps ? "kmc_hip_db_expr_device: more than KMC_HIP_DB_EXPR_MAX_LEAVES (16) leaves" : "kmc_hip_db_expr_device: malformed program (no steps)");
	for (u32 i = 0; i < n_steps; ++i) {
		const u32 kind = steps[i].kind, arg = steps[i].arg;
		if (kind == KMC_HIP_DB_EXPR_INPUT) {
			if (arg >= n_views)
				return fail(KMC_HIP_EINVAL, "kmc_hip_db_expr_device: malformed program (step " + std::to_string(i) + ": input index " + std::to_string(arg) + " out of range)");
			if (pl.n_leaves == CX_MAX_LEAVES)
				return fail(KMC_HIP_EINVAL, "kmc_hip_db_expr_device: more than KMC_HIP_DB_EXPR_MAX_LEAVES (16) leaves");
			pl.leaf_view[pl.n_leaves++] = arg;
			stack[depth++] = views[arg].n_recs;
			pl.prog.step[i] = CX_INPUT;
			continue;
		}
		if (kind > SO_COUNTERS_SUBTRACT || arg >= SO_N_CNT)
			return fail(KMC_HIP_EINVAL, "kmc_hip_db_expr_device: malformed program (step " + std::to_string(i) + ": unknown operation or counter mode)");
		if (depth < 2)
			return fail(KMC_HIP_EINVAL, "kmc_hip_db_expr_device: malformed program (step " + std::to_string(i) + ": stack underflow)");
		const u64 r = stack[--depth], l = stack[depth - 1];
		stack[depth - 1] = kind == SO_UNION ? l + r : kind == SO_INTERSECT ? std::min(l, r) : l;
		pl.prog.step[i] = kind | arg << 8;
	}
	if (depth != 1)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_expr_device: malformed program (" + std::to_string(depth) + " values left, not one)");
	pl.prog.n_steps = n_steps;
	pl.bound = stack[0];
	return 0;
}

template <int SIZE>
int db_expr_t(Slot &s, u32 k, const kmc_hip_db_view *views, u32 n_views, const ExprPlan &pl, const CxOut &wr, u32 p_out, u32 cs_out, uint8_t *d_out, u64 *d_lut_out, u64 *h_res /* [5] */)
{
	constexpr int W = SIZE + 1;
	const u32 L = pl.n_leaves;
	const u32 T = std::max(std::min(env_positive("KMC_HIP_EXPR_TILE", cx_default_tile<SIZE>()), cx_default_tile<SIZE>()), CX_MIN_TILE);
	const u32 M = 2 * L, S = (T + L) / (4 * L - 1); /* S (M + 2L - 1) - L <= T: order_db.hip.h */
	/* the inputs the expression names, unpacked once each, one behind the other */
	u64 words = 0;
	std::vector<u64> at(n_views, 0);
	std::vector<char> named(n_views, 0);
	for (u32 l = 0; l < L; ++l)
		named[pl.leaf_view[l]] = 1;
	for (u32 v = 0; v < n_views; ++v)
		if (named[v]) {
			at[v] = words;
			words += (views[v].n_recs * W + 31) & ~31ull;
		}
	CxLeaves lv = {};
	lv.n_leaves = L;
	u64 n_samples = 0;
	for (u32 l = 0; l < L; ++l) {
		lv.n[l] = views[pl.leaf_view[l]].n_recs;
		lv.first_sample[l] = n_samples;
		n_samples += (lv.n[l] + S - 1) / S;
	}
	lv.first_sample[L] = n_samples;
	const u64 n_tiles = (n_samples + M - 1) / M;
	if (n_tiles > 0x7FFFFFFFull || (std::max<u64>(n_samples, L) + 255) / 256 > 0x7FFFFFFFull)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_expr_device: more tiles than a launch has workgroups");
	/* work area: bounds [n_tiles + 1][L] | kept records per tile [n_tiles] | their exclusive sums [n_tiles + 1] (the last one: records written) | tallies [8] */
	const size_t work_words = (size_t)((n_tiles + 1) * L + 2 * n_tiles + 1 + 8);
	int rc = 0;
	if ((rc = ensure(s.recA, words * 8 + 256)) || (rc = ensure(s.recC, pl.bound * W * 8 + 256)) || (rc = ensure(s.bounds, work_words * 8)))
		return rc;
	u64 *unpacked = (u64 *)s.recA.p, *merged = (u64 *)s.recC.p;
	u64 *bounds = (u64 *)s.bounds.p, *tile_count = bounds + (n_tiles + 1) * L, *tile_base = tile_count + n_tiles, *stats = tile_base + n_tiles + 1;
	HIPCHK(hipMemsetAsync(bounds, 0, work_words * 8, s.stream)); /* no tile: the total is the 0 written here */
	for (u32 l = 0; l < L; ++l)
		lv.rec[l] = unpacked + at[pl.leaf_view[l]];
	for (u32 v = 0; v < n_views; ++v)
		if (named[v] && views[v].n_recs)
			k_db_unpack<SIZE><<<dim3((u32)((views[v].n_recs + 255) / 256)), dim3(256), 0, s.stream>>>(views[v].d_recs, views[v].n_recs, (const u64 *)views[v].d_lut, 1u << (2 * views[v].lut_prefix_len), k,
			                                                                                        views[v].lut_prefix_len, (k - views[v].lut_prefix_len) / 4, views[v].counter_size, unpacked + at[v],
			                                                                                        views[v].cutoff_min, views[v].cutoff_max - views[v].cutoff_min);
	if (n_tiles) {
		k_cx_partition<SIZE><<<dim3((u32)((std::max<u64>(n_samples, L) + 255) / 256)), dim3(256), 0, s.stream>>>(lv, S, M, n_samples, n_tiles, bounds);
		k_cx_tile<SIZE, false><<<dim3((u32)n_tiles), dim3(CX_THREADS), cx_lds_bytes<SIZE>(T, false), s.stream>>>(lv, pl.prog, bounds, T, wr, (const u64 *)nullptr, tile_count, (u64 *)nullptr, 0ull, stats);
		k_db_cumsum<<<dim3(1), dim3(256), 0, s.stream>>>(tile_count, n_tiles, tile_base);
		k_cx_tile<SIZE, true><<<dim3((u32)n_tiles), dim3(CX_THREADS), cx_lds_bytes<SIZE>(T, true), s.stream>>>(lv, pl.prog, bounds, T, wr, tile_base, (u64 *)nullptr, merged, pl.bound, stats);
	}
	HIPCHK(hipMemsetAsync(d_lut_out, 0, (1ull << (2 * p_out)) * 8, s.stream));
	if (pl.bound)
		k_db_pack<SIZE><<<dim3((u32)((pl.bound + 255) / 256)), dim3(256), 0, s.stream>>>(merged, pl.bound, k, p_out, cs_out, d_out, d_lut_out, tile_base + n_tiles);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(s.stream));
	u64 h[8];
	HIPCHK(hipMemcpy(h, stats, 8 * 8, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(h_res + 4, tile_base + n_tiles, 8, hipMemcpyDeviceToHost));
	for (int q = 0; q < 4; ++q)
		h_res[q] = h[q];
	if (h[CX_ST_FLAG])
		return fail(KMC_HIP_ECORRUPT, "kmc_hip_db_expr_device: a tile's slices exceed the tile (an input is not an ordered set of k-mers)");
	return 0;
}
} // namespace

int kmc_hip_db_expr_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *views, uint32_t n_views, const kmc_hip_db_expr_step *steps, uint32_t n_steps,
                           const kmc_hip_db_op *out, uint8_t *d_out, uint64_t out_capacity, uint64_t *d_lut_out, uint64_t *n_kmers, uint64_t stats[5])
{
	const char *who = "kmc_hip_db_expr_device";
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (!views || !steps || !out || !d_out || !d_lut_out || !n_kmers || !stats)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_expr_device: NULL argument");
	int rc = 0;
	for (u32 v = 0; v < n_views; ++v)
		if ((rc = check_view(who, views + v, kmer_len, 1)))
			return rc;
	if ((rc = check_prefix_len(who, "out_lut_prefix_len", out->out_lut_prefix_len, kmer_len)) || (rc = check_unpacked_width(who, kmer_len)))
		return rc;
	ExprPlan pl;
	if ((rc = expr_plan(views, n_views, steps, n_steps, pl)))
		return rc;
	if (out->cutoff_min < 1 || out->counter_max < 1)
		return fail(KMC_HIP_EINVAL, "kmc_hip_db_expr_device: the output's cutoff_min and counter_max must be at least 1");
	if ((rc = kmc_hip_synchronize(ctx, dev))) /* the inputs may come from asynchronous calls on any stream slot */
		return rc;
	Slot &s = ctx->devs[dev]->slot[0];
	std::lock_guard<std::mutex> lck(s.mtx);
	for (u32 v = 0; v < n_views; ++v)
		if ((rc = check_view_lut(who, views + v, 1)))
			return rc;
	const u32 cs_out = setop_counter_bytes(out->cutoff_max, out->counter_max), rb_out = (kmer_len - out->out_lut_prefix_len) / 4 + cs_out;
	if (pl.bound * rb_out > out_capacity)
		return fail(KMC_HIP_ECAPACITY, "kmc_hip_db_expr_device: out_capacity too small for the expression's upper bound (union: both sides' records; intersect: the smaller side's; subtractions: the left side's)");
	const CxOut wr = {out->cutoff_min, out->counter_max, out->cutoff_max};
	s.timed = false;
	if ((rc = by_words<7>((kmer_len + 31) / 32, [&](auto W) {
		     return db_expr_t<decltype(W)::value>(s, kmer_len, views, n_views, pl, wr, out->out_lut_prefix_len, cs_out, d_out, (u64 *)d_lut_out, (u64 *)stats);
	     })))
		return rc;
	*n_kmers = stats[4];
	return finish(s);
}
