/*
 * tests/hipemu/emu_sigstats.cpp — TEST INFRASTRUCTURE: k_s1_sig_stats of kmc_amd/csrc/stage1_kernels.hip.h on the CPU under the emulation in
 * tests/hipemu/include/hip/hip_runtime.h, launched the way s1_sigstats_part (kmc_amd/csrc/stage1_chain.h) launches it on the GPU, and the constants its test
 * cases are sized from. Built by tests/sigstats_cases.py (kernel_lib) in either geometry of tests/emu.py; never linked into libkmc_hip.so.
 */
#include <hip/hip_runtime.h>

#include "../../kmc_amd/csrc/stage1_kernels.hip.h"

extern "C" {
#define EMU_API __attribute__((visibility("default")))

/* g[0] = start positions per tile, g[1] = per strip, g[2] = the largest m with an LDS table, g[3] = S1_WG_TILE */
EMU_API void emu_s1_sig_stats_geometry(u32 *g)
{
	g[0] = S1_STATS_TILE;
	g[1] = S1_STATS_PER;
	g[2] = S1_STATS_LDS_M;
	g[3] = S1_WG_TILE;
}

/* the signature statistics of a code stream ADDED into table[4^m + 1]; returns the windows added. grid: workgroups (0 = one per tile); lds != 0: the
 * workgroup-private LDS table (m <= S1_STATS_LDS_M) */
EMU_API u64 emu_s1_sig_stats(const int8_t *codes, u64 n, unsigned k, unsigned m, u32 *table, unsigned grid, int lds)
{
	u64 total = 0;
	if (n < k)
		return 0;
	const u64 tiles = (n - k + 1 + S1_STATS_TILE - 1) / S1_STATS_TILE;
	const u32 g = grid && grid < tiles ? grid : (u32)tiles;
	if (lds && m <= S1_STATS_LDS_M)
		hipemu::launch(dim3(g), dim3(S1_BLOCK), 0, [&] { k_s1_sig_stats<(int)S1_STATS_LDS_M>(codes, n, k, m, table, &total); });
	else
		hipemu::launch(dim3(g), dim3(S1_BLOCK), 0, [&] { k_s1_sig_stats<0>(codes, n, k, m, table, &total); });
	return total;
}
}
