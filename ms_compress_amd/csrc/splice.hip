// splice.hip -- the passes of a block splicer (mscomp_amd_splicer_*, include/mscomp_amd.h): a new block container made of picks
// (source, resource) out of up to four source containers. No block is decoded or encoded: the stored form of a block depends only on its
// data, the format and the block size, so the layout pass hands every row of the new table the ADDRESS of its stored bytes and the move
// pass (blocks.hip bk_move_kernel) carries them, back-to-back rows of one source as one copy. The sources travel by value in the kernel
// arguments. DESIGN.md 4.12.
#include "kernels.h"

namespace msc {

// Layout, one block, in the shape of rs_layout_kernel. A pass over the picks in tiles: rules 1 and 2 per pick, a scan of the block counts
// of the picks that passed them -- rule 3 holds it against the table --, then a scan of the counts that stayed, which is new_first; new_len
// and the provisional statuses. A scan over the NEW table rows then gives every row its stored length, checksum and address: a row finds
// its pick by binary search in new_first and is source row first[r] + k of it. Then rule 7 on the picks' last rows.
__global__ __launch_bounds__(DV_THREADS) void sp_layout_kernel(SpliceView v0, SpliceView v1, SpliceView v2, SpliceView v3, uint32_t n_src, uint32_t n_pick, uint32_t nbt, uint32_t shift, u64 cap,
                                                              const u64* __restrict__ pick, u64* new_first, u64* new_off, uint32_t* __restrict__ new_crc,
                                                              u64* __restrict__ new_len, int32_t* status, u64* __restrict__ addr)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const u64 B = (u64)1 << shift;
	u64 run[1] = {0}, rows[1] = {0};
	if (tid == 0) { new_first[0] = 0; new_off[0] = 0; }
	for (uint32_t base = 0; base < n_pick; base += DV_THREADS) {
		const uint32_t p = base + tid;
		const bool live = p < n_pick;
		u64 n = 0, L = 0;
		int32_t st = 0;
		if (live) {
			const u64 s = pick[2u * (u64)p], r = pick[2u * (u64)p + 1u];
			st = -2;                                                        // rule 1: nothing of the pick is read further
			if (s < n_src) {
				const SpliceView v = sp_view(v0, v1, v2, v3, s);
				if (r < v.n_res) {
					const u64 f0 = v.first[r], f1 = v.first[r + 1u];
					if (f0 <= f1 && f1 <= v.nbt) {
						L = v.res_len[r]; n = f1 - f0;
						st = n == (L >> shift) + ((L & (B - 1u)) ? 1u : 0u) ? 0 : -3;   // rule 2
						if (st) { n = 0; L = 0; }
					}
				}
			}
		}
		u64 a[1] = {n};
		dv_block_scan<1>(a, run, s_w);
		if (n && a[0] > nbt) { st = -2; n = 0; L = 0; }                      // rule 3: the total includes this pick and the refused ones
		u64 b[1] = {n};
		dv_block_scan<1>(b, rows, s_w);
		if (live) { new_first[p + 1u] = b[0]; new_len[p] = L; status[p] = st; }
	}
	const u64 nbn = rows[0];                                             // (<= nbt: every pick that stayed passed rule 3)
	__syncthreads();                                                     // new_first is read back below, by other threads of this block
	u64 sum[1] = {0};
	for (uint32_t base = 0; base < nbt; base += DV_THREADS) {
		const uint32_t j = base + tid;
		const bool live = j < nbt;
		u64 len = 0, at = 0;
		uint32_t crc = 0;
		if (live && j < nbn) {
			const uint32_t p = res_of_block(new_first, n_pick, j);
			const SpliceView v = sp_view(v0, v1, v2, v3, pick[2u * (u64)p]);
			const u64 jr = v.first[pick[2u * (u64)p + 1u]] + (j - new_first[p]);   // (< v.nbt: rule 1)
			const u64 o0 = v.off[jr], o1 = v.off[jr + 1u];
			if (o0 <= o1 && o1 <= v.packed_len) { len = o1 - o0; }
			if (new_crc) { crc = v.crc[jr]; }
			if (len) { at = (u64)(uintptr_t)(v.packed + o0); }
		}
		u64 e[1] = {len};
		dv_block_scan<1>(e, sum, s_w);
		if (live) { new_off[j + 1u] = e[0]; addr[j] = e[0] <= cap ? at : 0; if (new_crc) { new_crc[j] = crc; } }
	}
	__syncthreads();                                                     // new_off is read back below
	for (uint32_t p = tid; p < n_pick; p += DV_THREADS) {
		const u64 n0 = new_first[p], n1 = new_first[p + 1u];
		if (n1 > n0 && new_off[n1] > cap) { status[p] = -5; }               // MSCOMP_BUF_ERROR replaces MSCOMP_OK (the offsets only grow: the last block tells)
	}
}

void launch_splice_layout(hipStream_t st, const SpliceSrc& src, uint32_t n_src, uint32_t n_pick, uint32_t nbt, uint32_t shift, u64 cap, const u64* pick,
                          u64* new_first, u64* new_off, uint32_t* new_crc, u64* new_len, int32_t* status, u64* addr)
{
	hipLaunchKernelGGL(sp_layout_kernel, dim3(1), dim3(DV_THREADS), 0, st, src.v[0], src.v[1], src.v[2], src.v[3], n_src, n_pick, nbt, shift, cap, pick, new_first, new_off, new_crc, new_len, status, addr);
}

} // namespace msc
