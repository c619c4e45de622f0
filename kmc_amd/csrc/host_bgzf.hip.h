/* kmc_amd/csrc/host_bgzf.hip.h — part of kmc_hip.hip (included there, not compiled on its own): BGZF input (BAM files, bgzipped FASTA / FASTQ). The member table is a
 * walk over the gzip headers on the host, the members are inflated and their CRCs checked on the device (k_bgzf_inflate, bgzf.hip.h), and inflated BAM text is cut
 * into parts of whole alignment records on the host (what CFastqReader does with zlib on one thread, kmc_core/fastq_reader.cpp:72-189 and :191-362). */
namespace {
const char *bgzf_reason(u32 e)
{
	switch (e) {
	case BGZF_E_BTYPE: return "block type 3";
	case BGZF_E_STORED: return "a stored block whose LEN is not the complement of NLEN or runs past the member";
	case BGZF_E_CODESET: return "an over-subscribed or incomplete set of code lengths";
	case BGZF_E_NO_EOB: return "no end-of-block code";
	case BGZF_E_REPEAT: return "a repeat code with nothing before it, or one that runs past the code lengths";
	case BGZF_E_SYMBOL: return "bits that are no code, or a symbol that deflate does not define";
	case BGZF_E_DISTANCE: return "a distance that reaches in front of the member's output";
	case BGZF_E_OUT_SHORT: return "the output ends short of ISIZE";
	case BGZF_E_OUT_LONG: return "the output goes beyond ISIZE";
	case BGZF_E_IN_LEFT: return "compressed bytes left over behind the final block";
	case BGZF_E_IN_SHORT: return "the compressed bytes end before the final block does";
	case BGZF_E_CRC: return "CRC32 mismatch";
	case BGZF_E_TABLE: return "a table entry no BGZF member can have";
	}
	return "unknown error";
}
inline u32 le16(const uint8_t *p) { return (u32)p[0] | (u32)p[1] << 8; }
inline u32 le32(const uint8_t *p) { return le16(p) | le16(p + 2) << 16; }
} // namespace

int kmc_hip_bgzf_scan(const uint8_t *src, uint64_t size, uint64_t max_out_bytes, kmc_hip_bgzf_member *members, uint64_t cap, uint64_t *n_members, uint64_t *src_used,
                      uint64_t *out_bytes)
{
	const std::string w("kmc_hip_bgzf_scan");
	if ((size && !src) || (cap && !members) || !n_members || !src_used || !out_bytes)
		return fail(KMC_HIP_EINVAL, w + ": NULL argument");
	u64 pos = 0, n = 0, out = 0;
	auto at = [&](const char *what) { return fail(KMC_HIP_ECORRUPT, w + ": " + what + " at byte " + std::to_string(pos)); };
	while (n < cap && size - pos >= 4) {
		const uint8_t *h = src + pos;
		if (h[0] != 0x1F || h[1] != 0x8B || h[2] != 8 || !(h[3] & 4))
			return at("no BGZF member (gzip magic, CM 8 and FLG.FEXTRA)");
		if (size - pos < 12)
			break;
		const u64 xlen = le16(h + 10);
		if (size - pos < 12 + xlen)
			break;
		u64 bsize = 0;
		for (u64 x = 0; x + 4 <= xlen;) {
			const u64 slen = le16(h + 12 + x + 2);
			if (h[12 + x] == 'B' && h[12 + x + 1] == 'C' && slen == 2 && x + 6 <= xlen) {
				bsize = (u64)le16(h + 12 + x + 4) + 1;
				break;
			}
			x += 4 + slen;
		}
		if (!bsize)
			return at("a gzip member without the BC subfield (not BGZF)");
		if (bsize < 12 + xlen + 8)
			return at("BSIZE too small for the member's own header and trailer");
		if (size - pos < bsize)
			break;
		u64 hd = 12 + xlen;
		for (u32 flag : {8u, 16u}) /* FNAME, FCOMMENT: zero-terminated */
			if (h[3] & flag) {
				while (hd + 8 < bsize && h[hd])
					++hd;
				++hd;
			}
		if (h[3] & 2) /* FHCRC */
			hd += 2;
		if (hd + 8 > bsize)
			return at("BSIZE too small for the member's own header and trailer");
		const u32 isize = le32(h + bsize - 4);
		if (isize > 65536)
			return at("ISIZE above 65536");
		if (isize > max_out_bytes - out)
			break;
		members[n].src_off = pos + hd;
		members[n].dst_off = out;
		members[n].comp_len = (u32)(bsize - 8 - hd);
		members[n].isize = isize;
		members[n].crc = le32(h + bsize - 8);
		members[n].reserved = 0;
		out += isize;
		pos += bsize;
		++n;
	}
	*n_members = n;
	*src_used = pos;
	*out_bytes = out;
	return 0;
}

int kmc_hip_bam_whole_records(const uint8_t *buf, uint64_t size, uint64_t *n_bytes, uint64_t *n_records)
{
	const std::string w("kmc_hip_bam_whole_records");
	if ((size && !buf) || !n_bytes || !n_records)
		return fail(KMC_HIP_EINVAL, w + ": NULL argument");
	u64 pos = 0, n = 0;
	while (size - pos >= 4) {
		const int32_t bs = (int32_t)le32(buf + pos);
		if (bs < 32)
			return fail(KMC_HIP_ECORRUPT, w + ": block_size " + std::to_string(bs) + " of record " + std::to_string(n) + " at byte " + std::to_string(pos) + " (an alignment record has 32 fixed bytes)");
		if (size - pos - 4 < (u64)bs)
			break;
		pos += 4 + (u64)bs;
		++n;
	}
	*n_bytes = pos;
	*n_records = n;
	return 0;
}

namespace {
int bgzf_check_table(const std::string &w, u64 src_size, const kmc_hip_bgzf_member *members, u64 n, u64 dst_capacity, u64 &total)
{
	if (n > 0x7FFFFFFFull)
		return fail(KMC_HIP_EINVAL, w + ": more members than a launch has workgroups");
	total = 0;
	for (u64 i = 0; i < n; ++i) {
		const kmc_hip_bgzf_member &m = members[i];
		if (m.isize > 65536 || m.comp_len > 65536)
			return fail(KMC_HIP_EINVAL, w + ": member " + std::to_string(i) + ": isize and comp_len are at most 65536");
		if (m.src_off > src_size || m.comp_len > src_size - m.src_off)
			return fail(KMC_HIP_EINVAL, w + ": member " + std::to_string(i) + " ends behind the source bytes");
		if (m.dst_off < total)
			return fail(KMC_HIP_EINVAL, w + ": member " + std::to_string(i) + ": dst_off must ascend, each output behind the one before");
		total = m.dst_off + m.isize;
	}
	if (total > dst_capacity)
		return fail(KMC_HIP_ECAPACITY, w + ": dst_capacity below the " + std::to_string(total) + " bytes of the table");
	return 0;
}

/* the launch and its verdict; the slot's mutex is held */
int bgzf_run(const std::string &w, Slot &s, const uint8_t *d_src, const kmc_hip_bgzf_member *members, u64 n, uint8_t *d_dst, uint32_t *first_bad, uint32_t *member_errors)
{
	static_assert(sizeof(kmc_hip_bgzf_member) == sizeof(BgzfMember) && sizeof(BgzfMember) == 32, "the table is uploaded as it is");
	*first_bad = KMC_HIP_BGZF_NONE;
	if (member_errors)
		std::fill(member_errors, member_errors + n, 0u);
	s.timed = false;
	s.bgzf_ms = 0;
	if (!n)
		return 0;
	if (int rc = ensure(s.bgzf_work, n * 36 + 16))
		return rc;
	BgzfMember *d_tab = (BgzfMember *)s.bgzf_work.p;
	u32 *d_err = (u32 *)((char *)s.bgzf_work.p + n * 32), *d_bad = d_err + n;
	HIPCHK(hipMemcpyAsync(d_tab, members, n * 32, hipMemcpyHostToDevice, s.stream));
	HIPCHK(hipMemsetAsync(d_err, 0, n * 4, s.stream));
	HIPCHK(hipMemsetAsync(d_bad, 0xFF, 4, s.stream));
	HIPCHK(hipEventRecord(s.ev[0], s.stream));
	k_bgzf_inflate<<<dim3((u32)n), dim3(64), 0, s.stream>>>((const BgzfMember *)d_tab, (u32)n, d_src, d_dst, d_err, d_bad);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(s.ev[1], s.stream));
	u32 bad = KMC_HIP_BGZF_NONE;
	HIPCHK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s.stream));
	HIPCHK(hipStreamSynchronize(s.stream));
	HIPCHK(hipEventElapsedTime(&s.bgzf_ms, s.ev[0], s.ev[1]));
	if (bad == KMC_HIP_BGZF_NONE)
		return 0;
	std::vector<u32> errs(n);
	HIPCHK(hipMemcpy(errs.data(), d_err, n * 4, hipMemcpyDeviceToHost));
	if (member_errors)
		std::copy(errs.begin(), errs.end(), member_errors);
	*first_bad = bad;
	return fail(KMC_HIP_ECORRUPT, w + ": BGZF member " + std::to_string(bad) + " (compressed data at byte " + std::to_string(members[bad].src_off) + "): " + bgzf_reason(errs[bad]));
}
} // namespace

int kmc_hip_bgzf_inflate_device(kmc_hip_ctx *ctx, int dev, int slot, const uint8_t *d_src, uint64_t src_size, const kmc_hip_bgzf_member *members, uint64_t n_members,
                                uint8_t *d_dst, uint64_t dst_capacity, uint32_t *first_bad, uint32_t *member_errors)
{
	const std::string w("kmc_hip_bgzf_inflate_device");
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (slot < 0 || slot >= N_SLOTS)
		return fail(KMC_HIP_EINVAL, w + ": bad slot");
	if (!first_bad || (n_members && !members))
		return fail(KMC_HIP_EINVAL, w + ": NULL argument");
	u64 total = 0;
	if (int rc = bgzf_check_table(w, src_size, members, n_members, dst_capacity, total))
		return rc;
	if ((src_size && !d_src) || (total && !d_dst))
		return fail(KMC_HIP_EINVAL, w + ": NULL argument (bytes without a buffer)");
	if (int rc = kmc_hip_synchronize(ctx, dev)) /* the bytes may come from asynchronous calls on any stream slot */
		return rc;
	Slot &s = ctx->devs[dev]->slot[slot];
	std::lock_guard<std::mutex> lck(s.mtx);
	if (int rc = bgzf_run(w, s, d_src, members, n_members, d_dst, first_bad, member_errors))
		return rc;
	return finish(s);
}

int kmc_hip_bgzf_inflate(kmc_hip_ctx *ctx, int dev, int slot, const uint8_t *src, uint64_t src_size, const kmc_hip_bgzf_member *members, uint64_t n_members, uint8_t *dst,
                         uint64_t dst_capacity, uint32_t *first_bad, uint32_t *member_errors)
{
	const std::string w("kmc_hip_bgzf_inflate");
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (slot < 0 || slot >= N_SLOTS)
		return fail(KMC_HIP_EINVAL, w + ": bad slot");
	if (!first_bad || (n_members && !members))
		return fail(KMC_HIP_EINVAL, w + ": NULL argument");
	u64 total = 0;
	if (int rc = bgzf_check_table(w, src_size, members, n_members, dst_capacity, total))
		return rc;
	if ((src_size && !src) || (total && !dst))
		return fail(KMC_HIP_EINVAL, w + ": NULL argument (bytes without a buffer)");
	Slot &s = ctx->devs[dev]->slot[slot];
	std::lock_guard<std::mutex> lck(s.mtx);
	if (int rc = ensure(s.bgzf_src, src_size + 16))
		return rc;
	if (int rc = ensure(s.bgzf_dst, total + 16))
		return rc;
	if (src_size)
		HIPCHK(hipMemcpyAsync(s.bgzf_src.p, src, src_size, hipMemcpyHostToDevice, s.stream));
	const int rc = bgzf_run(w, s, (const uint8_t *)s.bgzf_src.p, members, n_members, (uint8_t *)s.bgzf_dst.p, first_bad, member_errors);
	if (rc && rc != KMC_HIP_ECORRUPT)
		return rc;
	/* what the good members wrote comes back also when one was refused (a refused member's range is left as it was in the slot's buffer) */
	if (total)
		HIPCHK(hipMemcpy(dst, s.bgzf_dst.p, total, hipMemcpyDeviceToHost));
	if (rc) {
		const std::string msg = g_err;
		if (int rc2 = finish(s))
			return rc2;
		return fail(rc, msg);
	}
	return finish(s);
}

int kmc_hip_bgzf_last_ms(kmc_hip_ctx *ctx, int dev, int slot, float *ms)
{
	if (int rc = set_dev(ctx, dev))
		return rc;
	if (slot < 0 || slot >= N_SLOTS || !ms)
		return fail(KMC_HIP_EINVAL, "kmc_hip_bgzf_last_ms: bad slot or NULL argument");
	Slot &s = ctx->devs[dev]->slot[slot];
	std::lock_guard<std::mutex> lck(s.mtx);
	*ms = s.bgzf_ms;
	return 0;
}
