/* kmc_amd/csrc/host_kff_export.hip.h — part of kmc_hip.hip (included there, not compiled on its own): a database body framed as the records of a KFF file on the device
 * (what CKFFDbWriter<SIZE>::add_kmer does per k-mer on the CPU, kmc_tools/kff_db_writer.h:98-118; the kernel k_kff_frame is in kff_db.hip.h). */
int kmc_hip_db_kff_export_device(kmc_hip_ctx *ctx, int dev, uint32_t kmer_len, const kmc_hip_db_view *db, uint32_t n_lut_segments, uint64_t first, uint64_t count, uint32_t data_size,
                                 uint8_t *d_kff, uint64_t kff_capacity)
{
	const char *who = "kmc_hip_db_kff_export_device";
	const std::string w(who);
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (int rc = check_view(who, db, kmer_len, n_lut_segments))
		return rc;
	if (int rc = check_unpacked_width(who, kmer_len)) /* a KFF file's k: at most 224, as the import takes it */
		return rc;
	if (data_size < db->counter_size || data_size > 4)
		return fail(KMC_HIP_EINVAL, w + ": data_size must be the body's counter_size..4");
	if (first > db->n_recs || count > db->n_recs - first)
		return fail(KMC_HIP_EINVAL, w + ": the record range ends behind the database");
	if (count && !d_kff)
		return fail(KMC_HIP_EINVAL, w + ": NULL argument (records without d_kff)");
	const u32 p = db->lut_prefix_len, kbytes = (kmer_len + 3) / 4, sbytes = (kmer_len - p) / 4, rb_in = sbytes + db->counter_size, rb_out = kbytes + data_size;
	if (count > kff_capacity / rb_out)
		return fail(KMC_HIP_ECAPACITY, w + ": kff_capacity below count x (ceil(kmer_len / 4) + data_size)");
	if (int rc = kmc_hip_synchronize(ctx, dev)) /* the body may come from asynchronous calls on any stream slot */
		return rc;
	Slot &s = ctx->devs[dev]->slot[0];
	std::lock_guard<std::mutex> lck(s.mtx);
	if (int rc = check_view_lut(who, db, n_lut_segments))
		return rc;
	u32 dflt = kff_default_ipt(rb_in, rb_out);
	/* neighbouring lanes work ipt records apart: where that distance is a multiple of 64 bytes in either image, 16 lanes of a half-wave meet on one LDS bank with
	 * every byte they move (measured at k = 55: 16-byte KFF records, ipt 4 took 1.7 times as long as ipt 3) */
	while (dflt > 1 && ((dflt * rb_in) % 64 == 0 || (dflt * rb_out) % 64 == 0))
		--dflt;
	u32 ipt = std::min(env_positive("KMC_HIP_KFF_IPT", dflt), KFF_IPT_MAX); /* tests: 1, so that a few hundred records cross tile seams */
	while (ipt > 1 && kff_frame_lds_bytes(KFF_THREADS * ipt, rb_in, rb_out) > KFF_LDS_MAX)
		--ipt;
	const u64 tile = (u64)KFF_THREADS * ipt, n_tiles = (count + tile - 1) / tile;
	if (n_tiles > 0x7FFFFFFFull)
		return fail(KMC_HIP_EINVAL, w + ": more tiles than a launch has workgroups");
	s.timed = false;
	if (n_tiles) {
		const KffFrame g = {p, kbytes, sbytes, db->counter_size, data_size, (u32)((u64)n_lut_segments << (2 * p)), ipt};
		k_kff_frame<<<dim3((u32)n_tiles), dim3(KFF_THREADS), kff_frame_lds_bytes((u32)tile, rb_in, rb_out), s.stream>>>(db->d_recs, (const u64 *)db->d_lut, first, count, g, d_kff);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipStreamSynchronize(s.stream));
	return finish(s);
}
