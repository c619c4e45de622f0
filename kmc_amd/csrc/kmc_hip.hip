/*
 * kmc_amd/csrc/kmc_hip.hip — host side of libkmc_hip.so: the C-ABI of include/kmc_hip.h over the gfx950
 * kernels in kernels.hip.h. One context owns, per device, N_SLOTS "slots" (stream + grow-only HBM buffers), so
 * callers can keep several bins in flight (H2D of one bin under the kernels of another; small bins fill each other's
 * launch gaps).
 *
 * Reference mapping: this file plays the role of CKmerBinSorter<SIZE>::ProcessBins' body
 * (kmc_core/kb_sorter.h:210-237): Expand -> Sort -> Compact for one bin, but as a queue of kernels on a
 * HIP stream. No CPU fallback exists: if HIP is unusable every entry point fails with KMC_HIP_EDEVICE.
 */
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/kmc_hip.h"
#include "kernels.hip.h"
#include "bucket_sort.hip.h"
#include "arena_sort.hip.h"
#include "order_db.hip.h"
#include "stage1_kernels.hip.h"
#include "count_gather.hip.h"
#include "kff_db.hip.h"
#include "smallk_db.hip.h"
#include "bgzf.hip.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
	g_err = msg;
	return code;
}
int fail_hip(const char *what, hipError_t e)
{
	g_err = std::string(what) + ": " + hipGetErrorString(e);
	return e == hipErrorOutOfMemory ? KMC_HIP_ENOMEM : KMC_HIP_EDEVICE;
}
#define HIPCHK(call)                                                                                                   \
	do {                                                                                                               \
		hipError_t e__ = (call);                                                                                       \
		if (e__ != hipSuccess)                                                                                         \
			return fail_hip(#call, e__);                                                                               \
	} while (0)

struct DBuf {
	void *p = nullptr;
	size_t cap = 0;
	bool carved = false; /* p lies inside a slot's slab (kmc_hip_reserve_slot): never freed on its own */
};

/* A slot's slab: ONE device allocation made ahead of time (kmc_hip_reserve_slot: the drop-in's loader calls it while KMC's stage 1 runs) from which the slot's grow-only
 * buffers are carved. Why: the drop-in's workers allocate ~10 buffers each when stage 2 starts, through a runtime that takes the process's mmap lock — and the reference's
 * reader holds that lock while it unmaps every bin part it has copied (mem_disk_file.cpp:84-100): 16 workers spent 6.6 of 11.9 engine-seconds in those allocations on an
 * 8 Gbp input (profiles/r06/e2e_sweep_8gbp_session_n.jsonl). A buffer that does not fit what is left of the slab is allocated on its own, as before. */
struct Slab {
	void *p = nullptr;
	size_t cap = 0, used = 0;
};
thread_local Slab *t_slab = nullptr; /* the slab of the slot whose mutex this thread holds (SlabScope), if it has one */
struct SlabScope {
	Slab *prev;
	explicit SlabScope(Slab &sl) : prev(t_slab) { t_slab = sl.p ? &sl : nullptr; }
	~SlabScope() { t_slab = prev; }
};

int ensure(DBuf &b, size_t bytes)
{
	if (bytes <= b.cap)
		return 0;
	const size_t want = (bytes + 255) & ~(size_t)255;
	if (t_slab && t_slab->used + want <= t_slab->cap) { /* (what the buffer held before stays where it was: a little of the slab lost when a buffer grows) */
		if (b.p && !b.carved)
			HIPCHK(hipFree(b.p));
		b.p = (char *)t_slab->p + t_slab->used;
		b.cap = want;
		b.carved = true;
		t_slab->used += want;
		return 0;
	}
	if (b.p && !b.carved)
		HIPCHK(hipFree(b.p));
	b.p = nullptr;
	b.cap = 0;
	b.carved = false;
	HIPCHK(hipMalloc(&b.p, want));
	b.cap = want;
	return 0;
}

/* tuning and test switches, read from the environment variable `name` (a caller that must not read its switch twice keeps the value in a function-local static):
 * the positive integer in it, else `dflt` */
u32 env_positive(const char *name, u32 dflt)
{
	const char *e = getenv(name);
	return e && atoi(e) > 0 ? (u32)atoi(e) : dflt;
}
/* on, unless the variable holds 0 (or no number at all) */
bool env_on(const char *name)
{
	const char *e = getenv(name);
	return !e || atoi(e) != 0;
}
/* the integer in it, of either sign, else `dflt` */
int env_int(const char *name, int dflt)
{
	const char *e = getenv(name);
	return e ? atoi(e) : dflt;
}
/* the count (of bytes, of entries) in it, at most `cap`, else `dflt` */
u64 env_count(const char *name, u64 dflt, u64 cap = ~0ull)
{
	const char *e = getenv(name);
	return e ? std::min<u64>(strtoull(e, nullptr, 10), cap) : dflt;
}

/* is `p` host memory the device can reach by DMA as it is (hipHostMalloc / hipHostRegister)? Ordinary memory is staged through a pinned buffer of the slot. */
bool host_ptr_is_pinned(const void *p)
{
	static const bool always = !env_on("KMC_HIP_STAGE_PAGEABLE"); /* 0: copy straight from / to pageable memory (rounds 1-3) */
	if (always || !p)
		return true;
	hipPointerAttribute_t at;
	if (hipPointerGetAttributes(&at, p) != hipSuccess) {
		(void)hipGetLastError(); /* "invalid value" for memory the runtime has never seen: ordinary memory */
		return false;
	}
	return at.type == hipMemoryTypeHost || at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}
int ensure_pinned(void *&p, size_t &cap, size_t bytes)
{
	if (bytes <= cap)
		return 0;
	if (p) {
		HIPCHK(hipHostFree(p));
		p = nullptr;
		cap = 0;
	}
	const size_t want = (bytes + (bytes >> 2) + 4095) & ~(size_t)4095; /* grow-only, with room: bins come in descending size order at first, then vary */
	HIPCHK(hipHostMalloc(&p, want, hipHostMallocDefault));
	cap = want;
	return 0;
}

/* layout of the per-slot "small" device block (bytes): the first SM_BYTES of the slot's zero region, cleared with it at the start
 * of every bin */
/* bytes 0..15: unused */
constexpr size_t SM_STATS = 16;      /* u64[4]                           */
constexpr size_t SM_OUTBYTES = 48;   /* u64                              */
/* bytes 56..59: unused */
constexpr size_t SM_REDO = 60;       /* u32: set by the LDS finisher when a tile of the hybrid sort did not fit: the host sorts the group again, LSD over all bytes */
constexpr size_t SM_DBASE_WORK = 256; /* u64[2][256] per-portion digit bases (ping-pong) */
constexpr size_t SM_COUNTERS = 256 + 2 * 256 * 8; /* u32[N_COUNTERS] ticket counters, one per launch (the tally shards of the compaction are per bin, BinPlan) */
constexpr size_t N_COUNTERS = 4096;
constexpr size_t SM_BYTES = SM_COUNTERS + N_COUNTERS * 4;

#ifndef KMC_N_SLOTS
#define KMC_N_SLOTS 16 /* 512 bins of 3.2 M k-mers, device resident: 1 stream 237 ms, 2: 133, 4: 104, 8: 95 (then the host launch rate
                        * binds); the stage-2 worker spreads up to 16 sorter threads over them */
#endif
constexpr int N_SLOTS = KMC_N_SLOTS;
constexpr int N_BATCH_STREAMS = 8; /* default fan-out of kmc_hip_process_bins_device for small bins */
constexpr u32 TIMING_SAMPLE = 8;   /* an event pair costs a few microseconds of stream time: asynchronous bins are timed 1 in 8 */
constexpr u64 PORTION_MAX = 1ull << 29; /* records per scatter launch (30-bit look-back counts) */
/* Tests shrink the portion ($KMC_HIP_DEBUG_PORTION_LOG2, 10..29, read at kmc_hip_init, kept per context) so that a small,
 * oracle-checkable sort crosses many portion boundaries (digit bases carried from launch to launch) — the path a bin of
 * more than 2^29 k-mers takes. */

struct HostRes { /* the head of the small block, as the multi-device bin and the compaction hook read it back */
	u64 totals[2];
	u64 stats[4];
	u64 out_bytes;
	u32 err;
	u32 redo;
};

/* Everything a bin needs zeroed on the device lies in ONE region (one memset per bin instead of ~14: with 512 small bins
 * per run the host launch rate is what binds): start bitmap | expand look-back words | digit histograms | compaction
 * look-back words | one scatter status area per onesweep launch. Offsets are 256-byte aligned. */
struct ZeroPlan {
	size_t ghist = 0, sc_status = 0, sc_stride = 0, total = 0; /* the per-bin parts are in BinPlan */
	size_t giant = 0; /* rank groups: the list of tiles handed to k_giant_tiles (count, taken, tile numbers) */
	size_t arena = 0; /* rank groups of one-word records: the arena's AR_DYN_WORDS words, then its AR_MAX_PASS x 256 digit counters (arena_sort.hip.h); 0: no arena */
};
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

/* results of a host-boundary call (kmc_hip_process_bin_submit: one bin; kmc_hip_process_bins_submit: up to HB_MAX): per bin out_bytes + the four tallies, per
 * sort group the hybrid sort's "again" word, the stream's sticky error word — one block on the device, copied to pinned memory when the call's kernels are done */
constexpr u32 HB_MAX = 16;
struct HbRes {
	u64 w[HB_MAX][8]; /* [0] out_bytes, [1..4] stats */
	u32 flag[HB_MAX];
	u32 err, pad[15];
};

struct Slot {
	hipStream_t stream = nullptr;
	Slab slab; /* kmc_hip_reserve_slot */
	std::mutex mtx; /* serialises enqueueing on this slot (asynchronous device-resident calls may come from several threads) */
	u64 portion = PORTION_MAX;
	DBuf in, pack_start;
	DBuf recA, recB, recC, pairA, pairB, zero, dbase, out, lut, sticky;
	DBuf bounds;   /* hybrid sort: tile boundaries of k_bucket_bounds, u64[windows + 1] */
	DBuf arena_work; /* rank groups of one-word records: entries, offsets, bucket numbers, heavy chunks, digit bases and look-back rows of the arena's passes (the arenas: pairA / pairB) */
	DBuf bgzf_src, bgzf_dst, bgzf_work; /* BGZF (host_bgzf.hip.h): the compressed bytes and the inflated ones of the host-to-host entry; the member table, the error words and the smallest failing member */
	float bgzf_ms = 0; /* HIP events around the last k_bgzf_inflate of this slot */
	DBuf redo_log; /* hybrid sort: one "sort me again" word per asynchronous group since the last drain (drain_redo) */
	/* pinned staging for callers whose buffers are ordinary (pageable) memory — the drop-in worker's arena: a copy straight from / to such memory makes the
	 * runtime pin the caller's pages on the fly, and the unmapping of an arena that has been pinned piecewise costs twice as much at the end of KMC's stage 2
	 * (tools/ubench_munmap_hip.py: 0.23 s instead of 0.12 s for 2.3 GB; nothing left after a parallel MADV_DONTNEED only when nothing was ever pinned) */
	void *h_stage_in = nullptr, *h_stage_out = nullptr;
	size_t h_stage_in_cap = 0, h_stage_out_cap = 0;
	bool out_staged = false;
	u64 groups_run = 0;     /* groups enqueued on this slot since the context was made */
	bool zero_grew = false; /* the last group's zero region had to be re-allocated (diagnostics: reported with a watchdog error) */
	hipEvent_t ev[6] = {};
	hipEvent_t done_ev = nullptr; /* blocking-sync event: _wait must not spin (stage-2 workers outnumber the cores a container may use) */
	/* one event pair per scatter launch since the last harvest (roofline input) */
	std::vector<hipEvent_t> sc_ev;
	std::vector<u64> sc_cnt; /* records of the launch; bit 63: the pair brackets the LDS sort (k_bucket_bounds + k_bucket_rank), not a scatter pass */
	u32 sc_used = 0;
	double sc_ms_total = 0, ls_ms_total = 0;
	u64 sc_keys_total = 0, sc_launch_total = 0, ls_keys_total = 0, ls_launch_total = 0;
	bool timed = false;
	u32 async_seq = 0; /* asynchronous device-resident bins on this slot: every TIMING_SAMPLE-th one carries events */
	/* asynchronous device-resident groups since the last drain, in redo_log order */
	struct PendingGroup {
		DevParams P;
		u64 lut_entries;
		std::vector<kmc_hip_bin_desc> descs;
	};
	std::vector<PendingGroup> pending_groups;
	/* host-boundary call in flight — one bin (kmc_hip_process_bin_submit) or a group of bins (kmc_hip_process_bins_submit): what _wait and a redo need */
	enum HbCall { HB_NONE, HB_ONE_BIN, HB_GROUP };
	HbCall hb_call = HB_NONE; /* the entry that submitted: its _wait alone may collect (the callers' result arrays differ in length) */
	struct HostBin {
		kmc_hip_bin_desc d; /* device side */
		uint8_t *h_out;
		u64 *h_lut;
	};
	std::vector<HostBin> hb;
	std::vector<std::pair<u32, u32>> hb_chunks; /* (first bin, bins) of every sort group */
	std::vector<char> hb_hybrid;
	std::vector<u64> h_pack_start;
	DBuf hb_res;               /* both from slot_init: no allocation at the moment stage 2 starts */
	HbRes *h_hb_res = nullptr; /* pinned */
	DevParams hb_P = {};
	u64 lut_entries = 0;
	bool without_output = false;
};

/* A device array that stage-1 part calls add into, one per device and kind (the estimator's counters, the small-k table, the signature statistics): opened with parameters — the same ones
 * open it again as a no-op, others are refused —, read by range once the slots' streams are idle, closed only when no part call holds it (accum_* below). */
struct Accum {
	void *p = nullptr; /* nullptr = none open */
	u32 par[3] = {0, 0, 0}; /* what it was opened with */
	u64 entries = 0;
	u32 users = 0; /* part calls that took p (AccumHold) and have not returned: the close waits for them */
	std::mutex mtx;
	std::condition_variable idle;
};
/* A part call holds the array from its check of the parameters, under a.mtx, to its return, without the mutex: a concurrent close cannot free it in front of the kernel. */
struct AccumHold {
	Accum *a = nullptr;
	void take(Accum &acc) /* the caller holds acc.mtx */
	{
		++acc.users;
		a = &acc;
	}
	~AccumHold()
	{
		if (!a)
			return;
		std::lock_guard<std::mutex> lck(a->mtx);
		if (--a->users == 0)
			a->idle.notify_all();
	}
};

struct Dev {
	int ordinal = 0;
	u32 rr = 0; /* round-robin slot choice of asynchronous device-resident calls (under rr_mtx) */
	std::mutex rr_mtx;
	Slot slot[N_SLOTS];
	DBuf rccl_buf;
	DBuf xchg; /* kmc_hip_process_bin_multi: the records this device receives from the others */
	int *d_sig_map = nullptr; /* stage 1: the signature -> bin map of kmc_hip_split_set_map */
	u32 sig_map_entries = 0;
	std::mutex map_mtx;
	DBuf s1_arena[N_SLOTS]; /* stage 1: grow-only work area of kmc_hip_split_part, one per stream slot */
	Accum est;    /* stage 1: the two u32 counter arrays of kmc_hip_estimate_open (type 0, then type 1: 2^r entries each); par: kmer_len, s, r */
	Accum smallk; /* stage 1, small k: the 4^k u64 counters of kmc_hip_smallk_open; par: kmer_len, both_strands */
	Accum sigstats; /* stage 0: the 4^m + 1 u32 counters of kmc_hip_sigstats_open; par: kmer_len, signature_len */
};

u32 counter_bytes(u64 cutoff_max, u64 counter_max) { return kmc_counter_bytes(cutoff_max, counter_max); }

} // namespace

struct kmc_hip_ctx {
	std::vector<std::unique_ptr<Dev>> devs;
	std::vector<ncclComm_t> comms;
	bool comms_ready = false;
	u64 portion = PORTION_MAX;
	std::mutex mtx;
	std::vector<struct kmc_hip_count *> counts; /* open counting sessions (host_count.hip.h): kmc_hip_destroy closes them */
};

namespace {

/* The one dispatch on the record width: f(std::integral_constant<int, W>) with W == words, and what it returns; KMC_HIP_EINVAL for a width outside 1..MAX. MAX is 8
 * (k <= 256) for the entries that count, 7 for kmc_hip_order_database_device and the database family, whose records are SIZE + 1 words (k <= 224): no width above
 * MAX is instantiated. Kernel launches stay in the _t functions f calls, not in f itself (tests/emu.py rewrites them textually). */
template <int MAX, int W = 1, class F> int by_words(u32 words, F &&f)
{
	if (words == (u32)W)
		return f(std::integral_constant<int, W>{});
	if constexpr (W < MAX)
		return by_words<MAX, W + 1>(words, f);
	else
		return fail(KMC_HIP_EINVAL, "records of " + std::to_string(words) + " words: this entry takes 1.." + std::to_string(MAX));
}

int set_dev(kmc_hip_ctx *ctx, int dev)
{
	if (!ctx || dev < 0 || dev >= (int)ctx->devs.size())
		return fail(KMC_HIP_EINVAL, "bad ctx/dev");
	HIPCHK(hipSetDevice(ctx->devs[dev]->ordinal));
	return 0;
}

/* Kernels that want more than 64 KiB of dynamic LDS must opt in, per device (the attribute belongs to the device's copy of
 * the function): k_onesweep<SIZE> for SIZE >= 6 (k > 160), the histogram-fusing k_expand at 16 passes (k = 61..64). */
template <int SIZE> int set_func_attrs()
{
	if (rs_lds_bytes<SIZE>() + 32 * 1024 > 65536 && rs_lds_bytes<SIZE>() + 32 * 1024 <= 160 * 1024) /* + room for $KMC_HIP_SCATTER_LDS_PAD */
		HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_onesweep<SIZE>), hipFuncAttributeMaxDynamicSharedMemorySize,
		                           (int)rs_lds_bytes<SIZE>() + 32 * 1024));
	else if (rs_lds_bytes<SIZE>() > 65536)
		HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_onesweep<SIZE>), hipFuncAttributeMaxDynamicSharedMemorySize,
		                           (int)rs_lds_bytes<SIZE>()));
	if (br_lds_bytes<SIZE>() > 65536) {
		HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bucket_rank<SIZE, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)br_lds_bytes<SIZE>() + 32 * 1024)); /* + room for $KMC_HIP_RANK_LDS_PAD */
		if (SIZE == 1) {
			HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bucket_rank<1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)br_lds_bytes<1>()));
		}
	}
	if (exp_lds_bytes<true>(EXP_FUSE_MAX_PASS, 1) > 65536) /* worst case: the shortest records (smallest k) and 16 fused passes */
		HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_expand<SIZE, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
		                           (int)exp_lds_bytes<true>(EXP_FUSE_MAX_PASS, 1)));
	return 0;
}
int set_all_func_attrs()
{
	for (u32 words = 1; words <= 8; ++words)
		if (int rc = by_words<8>(words, [](auto W) { return set_func_attrs<decltype(W)::value>(); }))
			return rc;
	return 0;
}

int slot_init(Slot &s, u64 portion)
{
	s.portion = portion;
	HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
	HIPCHK(hipHostMalloc((void **)&s.h_hb_res, sizeof(HbRes), hipHostMallocDefault));
	memset(s.h_hb_res, 0, sizeof(HbRes));
	if (int rc = ensure(s.hb_res, sizeof(HbRes)))
		return rc;
	for (auto &e : s.ev)
		HIPCHK(hipEventCreate(&e));
	HIPCHK(hipEventCreateWithFlags(&s.done_ev, hipEventBlockingSync | hipEventDisableTiming));
	if (int rc = ensure(s.zero, SM_BYTES))
		return rc;
	HIPCHK(hipMemset(s.zero.p, 0, SM_BYTES));
	if (int rc = ensure(s.sticky, 256))
		return rc;
	HIPCHK(hipMemset(s.sticky.p, 0, 256));
	return 0;
}

void slot_destroy(Slot &s)
{
	for (DBuf *b : {&s.in, &s.pack_start, &s.recA, &s.recB, &s.recC, &s.pairA, &s.pairB, &s.zero, &s.dbase, &s.out, &s.lut, &s.sticky, &s.bounds, &s.arena_work, &s.redo_log, &s.hb_res, &s.bgzf_src, &s.bgzf_dst, &s.bgzf_work})
		if (b->p && !b->carved)
			(void)hipFree(b->p);
	if (s.slab.p)
		(void)hipFree(s.slab.p);
	if (s.h_hb_res)
		(void)hipHostFree(s.h_hb_res);
	if (s.h_stage_in)
		(void)hipHostFree(s.h_stage_in);
	if (s.h_stage_out)
		(void)hipHostFree(s.h_stage_out);
	for (auto &e : s.ev)
		if (e)
			(void)hipEventDestroy(e);
	for (auto &e : s.sc_ev)
		(void)hipEventDestroy(e);
	if (s.done_ev)
		(void)hipEventDestroy(s.done_ev);
	if (s.stream)
		(void)hipStreamDestroy(s.stream);
}

template <typename T> T *small_ptr(Slot &s, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(s.zero.p) + off); }
template <typename T> T *zero_ptr(Slot &s, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(s.zero.p) + off); }
u32 *err_ptr(Slot &s) { return static_cast<u32 *>(s.sticky.p); }

int sc_event_pair(Slot &s, hipEvent_t &e0, hipEvent_t &e1, u64 cnt)
{
	while (s.sc_ev.size() < (size_t)s.sc_used + 2) {
		hipEvent_t ne;
		HIPCHK(hipEventCreate(&ne));
		s.sc_ev.push_back(ne);
	}
	e0 = s.sc_ev[s.sc_used];
	e1 = s.sc_ev[s.sc_used + 1];
	s.sc_used += 2;
	s.sc_cnt.push_back(cnt);
	return 0;
}

int ls_event_pair(Slot &s, hipEvent_t &e0, hipEvent_t &e1, u64 cnt) { return sc_event_pair(s, e0, e1, cnt | (1ull << 63)); }

/* after the slot's stream is idle: fold the recorded scatter launches into the slot's totals */
int harvest(Slot &s)
{
	for (u32 i = 0; i + 1 < s.sc_used; i += 2) {
		float t = 0;
		HIPCHK(hipEventElapsedTime(&t, s.sc_ev[i], s.sc_ev[i + 1]));
		const u64 c = s.sc_cnt[i / 2];
		if (c >> 63) {
			s.ls_ms_total += t;
			s.ls_keys_total += c & ~(1ull << 63);
			++s.ls_launch_total;
		} else {
			s.sc_ms_total += t;
			s.sc_keys_total += c;
			++s.sc_launch_total;
		}
	}
	s.sc_used = 0;
	s.sc_cnt.clear();
	return 0;
}

/* the slot's sticky device error word: kernels OR into it, nothing on the per-bin path clears it, so an error raised by an
 * earlier asynchronous bin on this slot survives until somebody looks (kmc_hip_synchronize, a synchronous call, _wait). Behind it, in the same
 * 256-byte block, what the first look-back that timed out saw (kernels.hip.h KERR_DIAG_WORDS): kept per host thread for err_to_code's message. */
thread_local u32 g_diag[KERR_DIAG_WORDS] = {};
thread_local char g_diag_slot[96] = "";
int clear_sticky(Slot &s, u32 err)
{
	if (err & (KERR_WATCHDOG | KERR_PEER)) {
		HIPCHK(hipMemcpy(g_diag, s.sticky.p, sizeof g_diag, hipMemcpyDeviceToHost));
		g_diag[0] = err;
		snprintf(g_diag_slot, sizeof g_diag_slot, "; group %llu of its stream, zero region %s for it", (unsigned long long)s.groups_run, s.zero_grew ? "re-allocated" : "reused");
	} else
		g_diag[0] = 0;
	HIPCHK(hipMemset(s.sticky.p, 0, 4 * KERR_DIAG_WORDS));
	return 0;
}
int read_and_clear_sticky(Slot &s, u32 &err)
{
	HIPCHK(hipMemcpy(&err, s.sticky.p, 4, hipMemcpyDeviceToHost));
	if (err)
		return clear_sticky(s, err);
	return 0;
}

int err_to_code(u32 err); /* host_plan_and_groups.hip.h */
/* the end of a synchronous entry whose stream is idle: the slot's sticky word, read and cleared, as the return code */
int finish(Slot &s)
{
	u32 err = 0;
	if (int rc = read_and_clear_sticky(s, err))
		return rc;
	return err_to_code(err);
}

/* ---- what the database entries (set operations, filter, transform) ask of a kmc_hip_db_view; `who`: the entry's name; n_seg: segments of the view's LUT ---- */
int check_prefix_len(const char *who, const char *name, u32 p, u32 kmer_len)
{
	if (p < 1 || p > 15 || p >= kmer_len || (kmer_len - p) % 4)
		return fail(KMC_HIP_EINVAL, std::string(who) + ": (kmer_len - " + name + ") must be a positive multiple of 4, " + name + " 1..15");
	return 0;
}
int check_view(const char *who, const kmc_hip_db_view *db, u32 kmer_len, u64 n_seg)
{
	const std::string w(who);
	if (!db || !db->d_lut || (db->n_recs && !db->d_recs))
		return fail(KMC_HIP_EINVAL, w + ": NULL argument (a view, its records or its LUT)");
	if (db->counter_size < 1 || db->counter_size > 4)
		return fail(KMC_HIP_EINVAL, w + ": a database's counter_size must be 1..4 (kmc_tools refuses databases without counters, parameters_parser.cpp:788-793)");
	if (int rc = check_prefix_len(who, "lut_prefix_len", db->lut_prefix_len, kmer_len))
		return rc;
	if (n_seg < 1 || (n_seg << (2 * db->lut_prefix_len)) > 0x7FFFFFFFull)
		return fail(KMC_HIP_EINVAL, w + ": n_lut_segments must be at least 1 and the LUT shorter than 2^31 entries");
	return 0;
}
/* the entries that unpack records (SIZE + 1 words, by_words<7>); the histogram and the dump read the packed records and take every kmer_len */
int check_unpacked_width(const char *who, u32 kmer_len)
{
	if ((kmer_len + 31) / 32 + 1 > 8)
		return fail(KMC_HIP_EINVAL, std::string(who) + ": kmer_len <= 224");
	return 0;
}
/* the LUT's last entry — and, of a segmented LUT, the closing one behind it — must not lie behind the records (read back: the caller's streams are idle) */
int check_view_lut(const char *who, const kmc_hip_db_view *db, u64 n_seg)
{
	const u64 n_entries = n_seg << (2 * db->lut_prefix_len);
	u64 last[2] = {0, 0};
	HIPCHK(hipMemcpy(last, db->d_lut + (n_entries - 1), n_seg > 1 ? 16 : 8, hipMemcpyDeviceToHost));
	if (last[0] > db->n_recs || last[1] > db->n_recs)
		return fail(KMC_HIP_ECORRUPT, std::string(who) + ": a database's LUT ends behind its records");
	return 0;
}

/* ---- Accum: open, read, close (`who`: the entry's name, `what`: the array in the messages' words) ---- */
int wait_slots(Dev &d) /* what the device's slots have launched adds to the arrays */
{
	for (auto &sl : d.slot)
		if (sl.stream)
			HIPCHK(hipStreamSynchronize(sl.stream));
	return 0;
}
int accum_open(Accum &a, const char *who, const char *what, u32 p0, u32 p1, u32 p2, u64 entries, size_t entry_bytes)
{
	std::lock_guard<std::mutex> lck(a.mtx);
	if (a.p) {
		if (a.par[0] == p0 && a.par[1] == p1 && a.par[2] == p2)
			return 0;
		return fail(KMC_HIP_EINVAL, std::string(who) + ": " + what + " with other parameters is open on this device");
	}
	void *p = nullptr;
	HIPCHK(hipMalloc(&p, entries * entry_bytes));
	hipError_t e = hipMemset(p, 0, entries * entry_bytes);
	if (e == hipSuccess)
		e = hipDeviceSynchronize();
	if (e != hipSuccess) {
		(void)hipFree(p);
		return fail_hip(who, e);
	}
	a.p = p;
	a.par[0] = p0, a.par[1] = p1, a.par[2] = p2;
	a.entries = entries;
	return 0;
}
int accum_read(Accum &a, Dev &d, const char *who, const char *what, u64 first, u64 count, void *dst, size_t entry_bytes)
{
	std::lock_guard<std::mutex> lck(a.mtx);
	if (!a.p)
		return fail(KMC_HIP_EINVAL, std::string(who) + ": no " + what + " is open on this device");
	if ((count && !dst) || first > a.entries || count > a.entries - first)
		return fail(KMC_HIP_EINVAL, std::string(who) + ": [first, first + count) lies outside the " + std::to_string(a.entries) + " entries");
	if (int rc = wait_slots(d))
		return rc;
	if (count)
		HIPCHK(hipMemcpy(dst, (const char *)a.p + first * entry_bytes, (size_t)count * entry_bytes, hipMemcpyDeviceToHost));
	return 0;
}
int accum_close(Accum &a, Dev &d)
{
	std::unique_lock<std::mutex> lck(a.mtx);
	a.idle.wait(lck, [&a] { return a.users == 0; }); /* the array outlives every part call that holds it */
	if (!a.p)
		return 0;
	if (int rc = wait_slots(d))
		return rc;
	HIPCHK(hipFree(a.p));
	a.p = nullptr;
	a.par[0] = a.par[1] = a.par[2] = 0;
	a.entries = 0;
	return 0;
}

/* temporary device allocations of one call (the test hook and the plan of stage 1's first kernels): freed when the owner goes out of scope */
struct DevTemps {
	std::vector<void *> held;
	DevTemps() = default;
	DevTemps(const DevTemps &) = delete;
	DevTemps &operator=(const DevTemps &) = delete;
	~DevTemps()
	{
		for (void *p : held)
			(void)hipFree(p);
	}
	int alloc(void **p, size_t bytes)
	{
		HIPCHK(hipMalloc(p, bytes));
		held.push_back(*p);
		return 0;
	}
};

/* The rest of this translation unit, in the order it is compiled (round 5: one 3 400-line file split along its entry families; no kernel and no statement changed).
 * tests/emu.py build_hostlib inlines these files again before it rewrites the kernel launches for the CPU emulation. */
#include "host_arena_debug.hip.h" /* KMC_HIP_ARENA_DEBUG: the arena's steps read back and checked by the host (diagnostics, off by default) */
#include "host_plan_and_groups.hip.h" /* the sort planner, the HBM passes, the groups of bins (front end, shared tail, LSD / rank finishers, the arena's plan and launches), the redo of flagged groups */
#include "host_hooks_and_order.hip.h" /* stage-isolating test hooks (device side) and the globally ordered database */
#include "host_multi_device_bin.hip.h" /* one bin over all devices of the context */
#include "host_cabi_stage2.hip.h" /* the C-ABI of stage 2: lifetime, narrow boundary, full boundary (one bin / several bins per call, device-resident batches) */
#include "host_cabi_stage1.hip.h" /* the C-ABI test hooks and stage 1 on the device (reads -> bins in HBM; one part of input text -> bin records) */
#include "host_count.hip.h" /* the counting session: parts of a reads file -> bin records kept in HBM -> gathered bins -> stage 2 -> one ordered database body */
#include "host_cabi_collective.hip.h" /* the tally all-reduce over the devices of a context (RCCL) and the instrumentation entries */
#include "host_setops.hip.h" /* set operations between two ordered databases (`kmc_tools simple`) */
#include "host_query.hip.h" /* the reads of a file against an ordered database (`kmc_tools filter`) */
#include "host_transform.hip.h" /* one database reduced, histogrammed or dumped as text (`kmc_tools transform`) */
#include "host_expr.hip.h" /* a set expression over several ordered databases (`kmc_tools complex`) */
#include "host_compare.hip.h" /* two ordered databases compared (`kmc_tools compare`) */
#include "host_kff.hip.h" /* the records of a KFF file imported as a database body (the KFF inputs of every `kmc_tools` database mode) */
#include "host_kff_export.hip.h" /* a database body framed as the records of a KFF file (KFF output) */
#include "host_smallk_db.hip.h" /* the small-k table (k <= 13) tallied and framed as a database body or as KFF records (`kmc` with its small-k optimisation, stage 2) */
#include "host_bgzf.hip.h" /* BGZF members inflated on the device (BAM and bgzipped reads for `count`), the member table and the cut of BAM text into whole records on the host */
