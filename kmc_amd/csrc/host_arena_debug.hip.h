/* kmc_amd/csrc/host_arena_debug.hip.h — part of kmc_hip.hip (included there, not compiled on its own): KMC_HIP_ARENA_DEBUG, the steps of the arena sort (arena_sort.hip.h) read back and checked by the host. Diagnostics only: every check drains the stream. */
/* Level 1: once the passes are done, is the arena in order and every entry's slice its bucket? Level 2: also the gather and every pass against what the host makes of the
 * step's input. Level 3: also every pass by the ordinary k_onesweep, its length read back by the host, instead of k_onesweep_dyn. */
struct ArenaDebug {
	int level;             /* 0: the variable is not set. Set to anything below 2 it is level 1 */
	std::vector<u64> prev; /* level 2: the arena as the step before left it */
	ArenaDebug()
	{
		static const int v = getenv("KMC_HIP_ARENA_DEBUG") ? std::max(1, env_int("KMC_HIP_ARENA_DEBUG", 1)) : 0;
		level = v;
	}
};

/* drains the stream and reads the arena's words */
int arena_debug_dyn(Slot &s, const GrpRank &gr, u32 (&h_dyn)[AR_DYN_WORDS])
{
	HIPCHK(hipStreamSynchronize(s.stream));
	HIPCHK(hipMemcpy(h_dyn, gr.arena_dyn, sizeof h_dyn, hipMemcpyDeviceToHost));
	return 0;
}

/* the arena after the gather: every entry's records under the entry's ordinal, the entries' offsets, the digit histograms */
int arena_debug_gather(Slot &s, const GrpRank &gr, const ArenaWork &aw, u32 rbits, ArenaDebug &dbg)
{
	u32 h_dyn[AR_DYN_WORDS];
	if (int rc = arena_debug_dyn(s, gr, h_dyn))
		return rc;
	const u32 M = h_dyn[AR_M], ne = h_dyn[AR_N_ENT], np = h_dyn[AR_N_PASS];
	if (!M)
		return 0;
	std::vector<u64> cur(M);
	HIPCHK(hipMemcpy(cur.data(), aw.A, (size_t)M * 8, hipMemcpyDeviceToHost));
	std::vector<u32> off(ne + 1);
	std::vector<ArenaEntry> ent(ne);
	HIPCHK(hipMemcpy(off.data(), aw.arena_off, (size_t)(ne + 1) * 4, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(ent.data(), gr.arena_ent, (size_t)ne * sizeof(ArenaEntry), hipMemcpyDeviceToHost));
	const u64 rmask = rbits >= 64 ? ~0ull : ((1ull << rbits) - 1);
	u64 bad = 0, first = ~0ull, badoff = 0, run = 0;
	std::vector<u64> slice;
	for (u32 e = 0; e < ne; ++e) {
		if (off[e] != run)
			++badoff;
		run += ent[e].len;
		slice.resize(ent[e].len);
		HIPCHK(hipMemcpy(slice.data(), aw.S0 + (ent[e].w0 & ((1ull << 40) - 1)), (size_t)ent[e].len * 8, hipMemcpyDeviceToHost));
		for (u32 i = 0; i < ent[e].len; ++i)
			if (off[e] + i < M && cur[off[e] + i] != (((u64)e << rbits) | (slice[i] & rmask))) {
				if (!bad)
					first = off[e] + i;
				++bad;
			}
	}
	std::vector<u64> gh((size_t)AR_MAX_PASS * 256), want((size_t)AR_MAX_PASS * 256, 0);
	HIPCHK(hipMemcpy(gh.data(), aw.ghist, gh.size() * 8, hipMemcpyDeviceToHost));
	for (u32 i = 0; i < M; ++i)
		for (u32 b = 0; b < np; ++b)
			++want[b * 256 + ((cur[i] >> (8 * b)) & 255)];
	u64 badh = 0;
	for (size_t i = 0; i < (size_t)np * 256; ++i)
		badh += gh[i] != want[i];
	fprintf(stderr, "[arena debug] gather: %llu of %u records differ from the host's (first %llu), %llu offsets off (sum %llu), %llu histogram cells differ\n", (unsigned long long)bad, M,
	        (unsigned long long)first, (unsigned long long)badoff, (unsigned long long)run, (unsigned long long)badh);
	dbg.prev.swap(cur);
	return 0;
}

/* the arena after pass `pass` against a stable sort of the pass's input (dbg.prev) by its digit */
int arena_debug_check_pass(Slot &s, const GrpRank &gr, const ArenaWork &aw, u32 pass, ArenaDebug &dbg)
{
	u32 h_dyn[AR_DYN_WORDS];
	if (int rc = arena_debug_dyn(s, gr, h_dyn))
		return rc;
	const u32 M = h_dyn[AR_M];
	if (!M || pass >= h_dyn[AR_N_PASS])
		return 0;
	std::vector<u64> cur(M);
	HIPCHK(hipMemcpy(cur.data(), (pass & 1) ? aw.A : aw.B, (size_t)M * 8, hipMemcpyDeviceToHost)); /* pass p writes B when p is even */
	std::vector<u64> want(dbg.prev);
	std::stable_sort(want.begin(), want.end(), [&](u64 a, u64 b) { return ((a >> (8 * pass)) & 255) < ((b >> (8 * pass)) & 255); });
	u64 bad = 0, first = ~0ull;
	for (u32 i = 0; i < M; ++i)
		if (cur[i] != want[i]) {
			if (!bad)
				first = i;
			++bad;
		}
	fprintf(stderr, "[arena debug] pass %d: %llu of %u records differ from a stable sort of the pass's input by its digit (first %llu)\n", (int)pass, (unsigned long long)bad, M,
	        (unsigned long long)first);
	u32 shown = 0;
	for (u32 i = 0; i < M && shown < 12; ++i)
		if (cur[i] != want[i]) {
			u64 where = ~0ull; /* where the host expected the record the device put here */
			for (u32 j = 0; j < M; ++j)
				if (want[j] == cur[i]) {
					where = j;
					break;
				}
			fprintf(stderr, "[arena debug]   at %u: device %016llx host %016llx (the device's record belongs at %lld)\n", i, (unsigned long long)cur[i], (unsigned long long)want[i], (long long)where);
			++shown;
		}
	dbg.prev.swap(cur);
	return 0;
}

/* level 3's substitute for k_onesweep_dyn: pass `pass` by the ordinary kernel, its length read back by the host */
int arena_debug_sweep(Slot &s, const GrpRank &gr, const ArenaWork &aw, u32 pass)
{
	u32 h_dyn[AR_DYN_WORDS];
	if (int rc = arena_debug_dyn(s, gr, h_dyn))
		return rc;
	if (h_dyn[AR_M] && pass < h_dyn[AR_N_PASS]) {
		const u32 tiles = (h_dyn[AR_M] + RsCfg<1>::TILE - 1) / RsCfg<1>::TILE;
		k_onesweep<1><<<dim3(tiles), dim3(RS_BLOCK), rs_lds_bytes<1>(), s.stream>>>((pass & 1u) ? aw.B : aw.A, (pass & 1u) ? aw.A : aw.B, h_dyn[AR_M], pass,
		                                                                         aw.dbase + (size_t)pass * 256, aw.dbase + (size_t)AR_MAX_PASS * 256,
		                                                                         aw.status + (size_t)pass * aw.status_stride, gr.arena_dyn + AR_PASS_TICKET + pass, tiles, err_ptr(s));
	}
	return 0;
}

/* is the arena in order, and is every entry's slice the multiset of its bucket? */
int arena_debug_order(Slot &s, const GrpRank &gr, const ArenaWork &aw, u32 rbits, u32 ar_pass_max)
{
	u32 h_dyn[AR_DYN_WORDS];
	if (int rc = arena_debug_dyn(s, gr, h_dyn))
		return rc;
	const u32 M = h_dyn[AR_M], ne = h_dyn[AR_N_ENT], np = h_dyn[AR_N_PASS];
	fprintf(stderr, "[arena debug] entries %u records %u passes %u (max %u) items %u heavy %u overflow %u rbits %u\n", ne, M, np, ar_pass_max, h_dyn[AR_N_ITEMS], 0u,
	        h_dyn[AR_OVERFLOW], rbits);
	if (!M)
		return 0;
	std::vector<u64> ar(M);
	std::vector<u32> off(ne + 1);
	std::vector<ArenaEntry> ent(ne);
	HIPCHK(hipMemcpy(ar.data(), (np & 1u) ? aw.B : aw.A, (size_t)M * 8, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(off.data(), aw.arena_off, (size_t)(ne + 1) * 4, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(ent.data(), gr.arena_ent, (size_t)ne * sizeof(ArenaEntry), hipMemcpyDeviceToHost));
	u64 inversions = 0, first_inv = ~0ull;
	for (u32 i = 1; i < M; ++i)
		if (ar[i - 1] > ar[i]) {
			if (!inversions)
				first_inv = i;
			++inversions;
		}
	u64 bad_entries = 0, first_bad = ~0ull, bad_ord = 0;
	const u64 rmask = rbits >= 64 ? ~0ull : ((1ull << rbits) - 1);
	std::vector<u64> slice;
	for (u32 e = 0; e < ne; ++e) {
		const u64 gpos = ent[e].w0 & ((1ull << 40) - 1);
		slice.resize(ent[e].len);
		HIPCHK(hipMemcpy(slice.data(), aw.S0 + gpos, (size_t)ent[e].len * 8, hipMemcpyDeviceToHost));
		for (auto &x : slice)
			x = ((u64)e << rbits) | (x & rmask);
		std::sort(slice.begin(), slice.end());
		bool ok = off[e + 1] - off[e] == ent[e].len;
		for (u32 i = 0; ok && i < ent[e].len; ++i)
			ok = ar[off[e] + i] == slice[i];
		for (u32 i = off[e]; i < off[e + 1] && i < M; ++i)
			if ((ar[i] >> rbits) != e)
				++bad_ord;
		if (!ok) {
			if (!bad_entries)
				first_bad = e;
			++bad_entries;
		}
	}
	fprintf(stderr, "[arena debug] inversions %llu (first at %llu), entries whose slice is not their bucket in order: %llu (first %llu), records under a foreign ordinal %llu\n",
	        (unsigned long long)inversions, (unsigned long long)first_inv, (unsigned long long)bad_entries, (unsigned long long)first_bad, (unsigned long long)bad_ord);
	return 0;
}

/* inside the pass loop, level 2 and up, in front of pass `pass`: the pass before it checked; level 3: the pass itself enqueued here (the caller skips its own launch) */
int arena_debug_pass(Slot &s, const GrpRank &gr, const ArenaWork &aw, u32 pass, ArenaDebug &dbg)
{
	if (pass)
		if (int rc = arena_debug_check_pass(s, gr, aw, pass - 1, dbg))
			return rc;
	return dbg.level >= 3 ? arena_debug_sweep(s, gr, aw, pass) : 0;
}

/* behind the pass loop, every level: the last pass checked (level 2 and up), then the arena's order */
int arena_debug_finish(Slot &s, const GrpRank &gr, const ArenaWork &aw, u32 rbits, u32 ar_pass_max, ArenaDebug &dbg)
{
	if (dbg.level >= 2)
		if (int rc = arena_debug_check_pass(s, gr, aw, ar_pass_max - 1, dbg))
			return rc;
	return arena_debug_order(s, gr, aw, rbits, ar_pass_max);
}
