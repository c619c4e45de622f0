/* kmc_amd/csrc/host_kff.hip.h — part of kmc_hip.hip (included there, not compiled on its own): the records of a KFF file imported as a database body on the device
 * (what kmc_tools' KFF readers hand to every mode, kmc_tools/kff_db_reader.h; the kernels are in kff_db.hip.h). */
namespace {
/* work area in s.bounds, which the stable LSD sort of records of two words and more leaves alone: the sections' first records [n_sections + 1] | the two flags */
struct KffWork {
	u64 *sec_start, *bad; /* bad[0]: k_kff_repack / k_kff_unpack (a record number of the file), bad[1]: k_kff_verify (a position of the sorted sequence) */
};

int kff_repack(Slot &s, const uint8_t *d_kff, u64 n, const KffWork &w, u32 n_sections, u32 k, u32 p, u32 cs, bool closing, uint8_t *d_out, u64 *d_lut)
{
	const u32 kbytes = (k + 3) / 4, sbytes = (k - p) / 4, rb_in = kbytes + cs, rb_out = sbytes + cs;
	u32 ipt = std::min(env_positive("KMC_HIP_KFF_IPT", kff_default_ipt(rb_in, rb_out)), KFF_IPT_MAX); /* tests: 1, so that a few hundred records cross tile seams */
	while (ipt > 1 && kff_lds_bytes(KFF_THREADS * ipt, rb_in, rb_out) > KFF_LDS_MAX)
		--ipt;
	const u64 tile = (u64)KFF_THREADS * ipt, n_tiles = (n + tile - 1) / tile;
	const u32 n_fill = std::max(1u, std::min(n_sections, KFF_FILL_GROUPS));
	if (n_tiles + n_fill > 0x7FFFFFFFull)
		return fail(KMC_HIP_EINVAL, "kmc_hip_kff_import_device: more tiles than a launch has workgroups");
	const KffGeo g = {k, p, kbytes, sbytes, cs, n_sections, ipt, closing ? 1u : 0u};
	k_kff_repack<<<dim3((u32)(n_tiles + n_fill)), dim3(KFF_THREADS), kff_lds_bytes((u32)tile, rb_in, rb_out), s.stream>>>(d_kff, n, (const u64 *)w.sec_start, g, (u32)n_tiles, d_out, d_lut, w.bad);
	HIPCHK(hipGetLastError());
	return 0;
}

/* several sections into one ascending body: order_database_t's pipeline with another front (k_kff_unpack) and a check of the sorted neighbours behind the sort */
template <int SIZE>
int kff_order_t(Slot &s, const uint8_t *d_kff, u64 n, const KffWork &w, u32 n_sections, u32 k, u32 p_out, u32 cs, uint8_t *d_out, u64 *d_lut_out)
{
	constexpr int W = SIZE + 1;
	int rc = 0;
	if ((rc = ensure(s.recA, n * W * 8 + 256)) || (rc = ensure(s.recB, n * W * 8 + 256)))
		return rc;
	u64 *recs = (u64 *)s.recA.p, *sorted = recs;
	const u32 blocks = (u32)((n + 255) / 256);
	k_kff_unpack<SIZE><<<dim3(blocks), dim3(256), 0, s.stream>>>(d_kff, n, (const u64 *)w.sec_start, n_sections, k, (k + 3) / 4, cs, recs, w.bad);
	HIPCHK(hipGetLastError());
	if ((rc = sort_device(s, recs, (u64 *)s.recB.p, n, W, (2 * k + 7) / 8, &sorted, true /* the count rides above the key: stable LSD passes */)))
		return rc;
	HIPCHK(hipMemsetAsync(d_lut_out, 0, (1ull << (2 * p_out)) * 8, s.stream));
	k_kff_verify<SIZE><<<dim3(blocks), dim3(256), 0, s.stream>>>((const u64 *)sorted, n, w.bad + 1);
	k_db_pack<SIZE><<<dim3(blocks), dim3(256), 0, s.stream>>>((const u64 *)sorted, n, k, p_out, cs, d_out, d_lut_out, (const u64 *)nullptr);
	HIPCHK(hipGetLastError());
	return 0;
}
} // namespace

int kmc_hip_kff_import_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, uint32_t data_size, const uint8_t *d_kff, const uint64_t *section_n_recs, uint32_t n_sections,
                              uint32_t ordered, uint32_t out_lut_prefix_len, uint8_t *d_out, uint64_t out_capacity, uint64_t *d_lut_out, uint64_t *n_kmers)
{
	const char *who = "kmc_hip_kff_import_device";
	const std::string w(who);
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (!d_out || !d_lut_out || !n_kmers || (n_sections && !section_n_recs))
		return fail(KMC_HIP_EINVAL, w + ": NULL argument");
	if (data_size < 1 || data_size > 4)
		return fail(KMC_HIP_EINVAL, w + ": a KFF file's data_size must be 1..4 (kmc_tools refuses k-mers without counters, parameters_parser.cpp:788-793)");
	if (kmer_len < 1)
		return fail(KMC_HIP_EINVAL, w + ": kmer_len must be 1..224");
	if (int rc = check_unpacked_width(who, kmer_len))
		return rc;
	const u32 p = out_lut_prefix_len;
	if (int rc = check_prefix_len(who, "out_lut_prefix_len", p, kmer_len))
		return rc;
	if (ordered > 1)
		return fail(KMC_HIP_EINVAL, w + ": ordered must be 0 (the body as it lies in the file) or 1 (one ascending body)");
	if (!ordered && (((u64)n_sections << (2 * p)) + 1 > 0x7FFFFFFFull))
		return fail(KMC_HIP_EINVAL, w + ": a segmented LUT of n_sections x 4^out_lut_prefix_len entries must be shorter than 2^31 entries");
	/* the sections' first records; for one ascending body the empty sections are left out: they hold nothing to order */
	std::vector<u64> start{0};
	const u32 rb_in = (kmer_len + 3) / 4 + data_size, rb_out = (kmer_len - p) / 4 + data_size;
	for (u32 i = 0; i < n_sections; ++i) {
		if (section_n_recs[i] > (1ull << 56) / rb_in - start.back())
			return fail(KMC_HIP_EINVAL, w + ": more records than a 64-bit byte offset reaches");
		if (section_n_recs[i] || !ordered)
			start.push_back(start.back() + section_n_recs[i]);
	}
	const u32 n_sec = (u32)start.size() - 1;
	const u64 n = start.back();
	if (n && !d_kff)
		return fail(KMC_HIP_EINVAL, w + ": NULL argument (records without d_kff)");
	*n_kmers = n;
	if (n * rb_out > out_capacity)
		return fail(KMC_HIP_ECAPACITY, w + ": out_capacity too small for the file's records");
	if (int rc = kmc_hip_synchronize(ctx, dev)) /* the input may come from asynchronous calls on any stream slot */
		return rc;
	Slot &s = ctx->devs[dev]->slot[0];
	std::lock_guard<std::mutex> lck(s.mtx);
	if (int rc = ensure(s.bounds, (start.size() + 2) * 8))
		return rc;
	const KffWork work = {(u64 *)s.bounds.p, (u64 *)s.bounds.p + start.size()};
	start.push_back(KFF_NONE);
	start.push_back(KFF_NONE);
	HIPCHK(hipMemcpy(work.sec_start, start.data(), start.size() * 8, hipMemcpyHostToDevice));
	s.timed = false;
	if (!ordered || n_sec <= 1) {
		if (int rc = kff_repack(s, d_kff, n, work, n_sec, kmer_len, p, data_size, !ordered, d_out, (u64 *)d_lut_out))
			return rc;
		if (ordered && !n_sec) /* no record: the LUT of an empty body */
			HIPCHK(hipMemsetAsync(d_lut_out, 0, (1ull << (2 * p)) * 8, s.stream));
	} else if (int rc = by_words<7>((kmer_len + 31) / 32, [&](auto W) { return kff_order_t<decltype(W)::value>(s, d_kff, n, work, n_sec, kmer_len, p, data_size, d_out, (u64 *)d_lut_out); }))
		return rc;
	HIPCHK(hipStreamSynchronize(s.stream));
	if (int rc = harvest(s))
		return rc;
	u64 bad[2] = {KFF_NONE, KFF_NONE};
	HIPCHK(hipMemcpy(bad, work.bad, 16, hipMemcpyDeviceToHost));
	if (int rc = finish(s))
		return rc;
	if (bad[0] != KFF_NONE) { /* name the record as the caller numbers its sections */
		u64 before = 0;
		u32 sec = 0;
		while (sec + 1 < n_sections && before + section_n_recs[sec] <= bad[0])
			before += section_n_recs[sec++];
		return fail(KMC_HIP_ECORRUPT, w + ": KFF record " + std::to_string(bad[0]) + " (record " + std::to_string(bad[0] - before) + " of section " + std::to_string(sec) +
		                                  "): padding bits set, a prefix beyond 4^out_lut_prefix_len, or not greater than its predecessor in the section");
	}
	if (bad[1] != KFF_NONE)
		return fail(KMC_HIP_ECORRUPT, w + ": a k-mer is present in two KFF sections (records " + std::to_string(bad[1] - 1) + " and " + std::to_string(bad[1]) + " of the ordered sequence)");
	return 0;
}
