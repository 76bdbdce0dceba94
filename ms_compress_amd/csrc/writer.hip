// writer.hip -- the passes of a block writer (mscomp_amd_writer_*, include/mscomp_amd.h): a batch of byte-range writes into a block container,
// out of place. The requests are admitted, the covering blocks get their owners, and the owners' blocks are decoded, checksummed and folded
// into verdicts by the reader's passes (reader.hip, unchanged: a write reads every block it touches first). Behind the fold the passes of
// this file load the raw owners into their cache slots and apply the MSCOMP_OK requests in request order, hand the dirty blocks to a
// compress dev plan and the CRC kernels (api.hip runs both between these passes, unchanged), lay the new container out around them and move
// every block -- clean ones from the old container, dirty ones from the staging area or the cache -- to its new place. DESIGN.md 4.10.
#include "kernels.h"

namespace msc {

#define WR_CLEAN 0u                                       // the move pass's word of a block: stored bytes carried over from d_packed
#define WR_NONE  1u                                       // nothing to move (no such block, a stored length of 0, an unreadable table entry)
#define WR_DIRTY 2u                                       // from here on: 2 + 2 * owner unit + (1: the staged bytes, 0: the cache slot, raw)

// One thread per possible unit: the unit joins the list of its block (head[j] = the last unit that came, + 1; next[u] = the one before it).
// The order of a list is the order the hardware ran the units in; the patch pass sorts it.
__global__ __launch_bounds__(256) void wr_link_kernel(uint32_t n_req, uint32_t m, WriterTab t)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u == 0) { t.r.cnt[2] = 0; }
	if (u >= m || u >= t.r.unit_first[n_req]) { return; }
	t.next[u] = atomicExch(&t.head[t.r.ublk[u]], u + 1u);
}

// The part of unit u's request that falls into the piece [a0, a1) of its block, from the caller's source to the block's cache slot.
__device__ __forceinline__ void wr_apply(const ReaderTab& r, uint32_t u, uint32_t shift, uint32_t a0, uint32_t a1, uint8_t* __restrict__ slot,
                                         const uint8_t* __restrict__ src, const u64* __restrict__ src_off, uint32_t lane)
{
	const uint32_t q = r.uq[u];
	const u64 o = r.q_off[q], end = o + r.q_want[q], b0 = ((o >> shift) + (u - r.unit_first[q])) << shift;
	const u64 lo = o > b0 + a0 ? o : b0 + a0, hi = end < b0 + a1 ? end : b0 + a1;
	if (lo >= hi) { return; }
	rd_wave_move(slot + (lo - b0), src + src_off[q] + (lo - o), (uint32_t)(hi - lo), lane);
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // the next unit's bytes may lie on these: its stores are issued behind them
}

// One wave, one piece [a0, a1) of the block that unit o owns: the block's units of MSCOMP_OK requests, in ascending unit number -- which
// is request order --, applied to the piece; a raw block's piece is first loaded into the cache slot (a decoded one lies there already).
// Pieces are disjoint, so the waves of one block do not meet, and within a piece the order is this wave's program order: the later request
// wins every byte, whatever order the units ran or linked in. Up to 64 units are ranked in the wave; a longer list is served by picking the
// smallest unit above the last one again and again, which is exact and merely slow. Piece 0 says whether the block is dirty.
__device__ __forceinline__ void wr_patch_piece(const WriterTab& t, uint32_t o, uint32_t a0, uint32_t a1, uint32_t m, uint32_t shift, uint8_t* __restrict__ cache,
                                               const uint8_t* __restrict__ src, const u64* __restrict__ src_off, uint32_t lane)
{
	const ReaderTab& r = t.r;
	const uint32_t j = r.ublk[o];
	uint32_t n = 0, mine = 0xFFFFFFFFu, steps = 0;
	for (uint32_t x = t.head[j]; x != 0 && steps < m; x = t.next[x - 1u], ++steps) {   // (a list holds at most every unit)
		if (r.q_stat[r.uq[x - 1u]] == 0) { if (n == lane) { mine = x - 1u; } ++n; }
	}
	if (a0 == 0 && lane == 0) { t.dirty[o] = n ? 1u : 0u; if (n) { atomicAdd(&r.cnt[2], 1u); } }
	if (n == 0) { return; }
	uint8_t* slot = cache + ((u64)o << shift);
	if ((r.act[o] & 3u) == RD_COPY) {
		rd_wave_move(slot + a0, reinterpret_cast<const uint8_t*>((uintptr_t)r.src[o]) + a0, a1 - a0, lane);
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	}
	if (n <= 64u) {
		uint32_t rank = 0;
		for (uint32_t k = 0; k < n; ++k) { rank += __shfl(mine, (int)k, 64) < mine ? 1u : 0u; }
		for (uint32_t k = 0; k < n; ++k) {
			const int l = __ffsll((unsigned long long)__ballot(lane < n && rank == k)) - 1;
			wr_apply(r, __shfl(mine, l, 64), shift, a0, a1, slot, src, src_off, lane);
		}
	} else {
		uint32_t last = 0;
		for (uint32_t k = 0; k < n; ++k) {
			uint32_t best = 0xFFFFFFFFu;
			steps = 0;
			for (uint32_t x = t.head[j]; x != 0 && steps < m; x = t.next[x - 1u], ++steps) {
				const uint32_t u = x - 1u;
				if ((k == 0 || u > last) && u < best && r.q_stat[r.uq[u]] == 0) { best = u; }
			}
			wr_apply(r, best, shift, a0, a1, slot, src, src_off, lane);
			last = best;
		}
	}
}

// Load and patch. An item is one (unit, 16 KiB piece) pair, dealt to the waves of a fixed grid as the reader's gather deals them: a LANE
// finds out whether its item is a piece of a readable owner's block -- the table loads of 64 items in flight together --, then the WAVE
// serves those one after the other. A thousand 64-byte writes so cost a wave a few round trips each, not a workgroup.
__global__ __launch_bounds__(256) void wr_patch_kernel(uint32_t n_req, uint32_t m, uint32_t shift, uint32_t ppu_shift, const uint8_t* __restrict__ src,
                                                      const u64* __restrict__ src_off, uint8_t* __restrict__ cache, WriterTab t)
{
	const uint32_t lane = threadIdx.x & 63u;
	const u64 items = t.r.unit_first[n_req] << ppu_shift, nw = (u64)gridDim.x * 4u, w = (u64)blockIdx.x * 4u + (threadIdx.x >> 6);
	u64 per = (items + nw - 1u) / nw;
	per = per < 1u ? 1u : per > 64u ? 64u : per;
	for (u64 base = w * per; base < items; base += nw * per) {
		uint32_t o = 0, a0 = 0, a1 = 0;
		const u64 i = base + lane;
		if (lane < per && i < items) {
			const uint32_t u = (uint32_t)(i >> ppu_shift), a = t.r.act[u], kind = a & 3u, e = a >> 2;   // (a unit that owns nothing: RD_SKIP)
			const u64 at = (i & (((u64)1 << ppu_shift) - 1u)) << RD_PIECE_SHIFT;
			if ((kind == RD_COPY || kind == RD_DECODE) && at < e) {
				o = u; a0 = (uint32_t)at; a1 = e - at < ((u64)1 << RD_PIECE_SHIFT) ? e : (uint32_t)at + (1u << RD_PIECE_SHIFT);
			} else if (at == 0) { t.dirty[u] = 0; }
		}
		u64 todo = __ballot(a1 > a0);
		while (todo) {
			const int l = __ffsll((unsigned long long)todo) - 1;
			todo &= todo - 1u;
			wr_patch_piece(t, __shfl(o, l, 64), __shfl(a0, l, 64), __shfl(a1, l, 64), m, shift, cache, src, src_off, lane);
		}
	}
}

// One thread per possible unit, behind the patch: a dirty owner becomes a unit of the inner compress plan -- its cache slot in, its staging
// slot out, capacity e - 1 as a block container gives it -- and of the CRC kernels; every other unit is empty in both. The columns are the
// ones the decompress plan and the old blocks' CRC used: the fold has read them.
__global__ __launch_bounds__(256) void wr_cunits_kernel(uint32_t n_req, uint32_t m, uint32_t shift, const uint8_t* __restrict__ cache, WriterTab t)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u >= m) { return; }
	const ReaderTab& r = t.r;
	const bool d = u < r.unit_first[n_req] && t.dirty[u] != 0;
	const u64 e = d ? r.act[u] >> 2 : 0, at = d ? (u64)u << shift : 0;
	r.in_off[u] = at; r.in_len[u] = e; r.out_off[u] = at; r.out_cap[u] = d ? e - 1u : 0;
	r.src[u] = d ? (u64)(uintptr_t)(cache + at) : 0; r.clen[u] = e;
}

// Layout, one block. Rule 0 first: the table as a whole (block_first[n_res] within the table, block_first never decreasing). Then one scan
// over the block table: the new stored length of every block -- a dirty one's from the compress plan (the staged bytes when they fitted
// into e - 1, the raw block otherwise: bk_select_kernel's rule), a clean one's from the old table, 0 for an entry that cannot be read --,
// new_block_off, the merged CRC table, and the move pass's word per block (in t.head, which the patch is done with). Then the resources'
// statuses by the capacity rule of a block container; a refused table overwrites what the fold reported for the requests.
__global__ __launch_bounds__(DV_THREADS) void wr_layout_kernel(uint32_t n_req, uint32_t n_res, uint32_t nbt, uint32_t m, u64 packed_len, u64 cap,
                                                              const u64* __restrict__ block_first, const u64* __restrict__ block_off, const uint32_t* __restrict__ block_crc,
                                                              WriterTab t, u64* new_off, uint32_t* __restrict__ new_crc, u64* __restrict__ d_written,
                                                              int32_t* __restrict__ d_status, int32_t* __restrict__ d_res_status)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const ReaderTab& r = t.r;
	const u64 nb = block_first[n_res];
	int wrong = nb > nbt ? 1 : 0;
	for (uint32_t i = tid; i < n_res; i += DV_THREADS) { if (block_first[i] > block_first[i + 1u]) { wrong = 1; } }
	const bool bad = __syncthreads_or(wrong) != 0;
	if (tid == 0) { r.cnt[3] = bad ? 1u : 0u; new_off[0] = 0; }
	u64 run[1] = {0};
	for (uint32_t base = 0; base < nbt; base += DV_THREADS) {
		const uint32_t j = base + tid;
		const bool live = j < nbt;
		u64 len = 0;
		uint32_t crc = 0, word = WR_NONE;
		if (live && !bad && j < nb) {
			const uint32_t bid = m ? r.own[j] : 0u, o = ~bid;                 // (own is cleared and bid for only when a call can have units)
			if (bid != 0 && t.dirty[o] != 0) {
				const u64 e = r.act[o] >> 2;
				const bool comp = r.ustat[o] == 0 && r.ulen[o] < e;
				len = comp ? r.ulen[o] : e; crc = r.ucrc[o]; word = WR_DIRTY + 2u * o + (comp ? 1u : 0u);
			} else {
				const u64 o0 = block_off[j], o1 = block_off[j + 1u];
				if (o0 <= o1 && o1 <= packed_len) { len = o1 - o0; }
				crc = block_crc ? block_crc[j] : 0u; word = len ? WR_CLEAN : WR_NONE;
			}
		}
		u64 v[1] = {len};
		dv_block_scan<1>(v, run, s_w);
		if (live) { new_off[j + 1u] = v[0]; t.head[j] = word; if (new_crc) { new_crc[j] = crc; } }
	}
	__syncthreads();                                                     // new_off is read back below, by other threads of this block
	for (uint32_t i = tid; i < n_res; i += DV_THREADS) {
		const u64 f0 = block_first[i], f1 = block_first[i + 1u];
		d_res_status[i] = bad ? -2 : (f1 > f0 && new_off[f1] > cap) ? -5 : 0;   // MSCOMP_ARG_ERROR; MSCOMP_BUF_ERROR (the offsets only grow: the last block tells)
	}
	if (bad) { for (uint32_t q = tid; q < n_req; q += DV_THREADS) { d_status[q] = -2; d_written[q] = 0; } }
}

// Move: the only pass over the whole container. The new byte range [0, min(total, cap)) is cut into equal slices, one per block of a fixed
// grid, as compaction cuts it (cpd_copy_kernel); a workgroup finds the block its slice starts in and walks on from there. 64 table rows
// are looked at at once, a row per lane: the clean blocks in front of the first row that is not clean lie back to back in d_packed and go
// back to back into the new container, so they are ONE copy that is shifted by a constant -- a container of small blocks with a few dirty
// ones moves in long runs, not block by block. A dirty block comes from its staging slot or, raw, from its cache slot. A block that would
// end beyond cap is not written, nor is anything behind it.
__global__ __launch_bounds__(CPD_THREADS) void wr_move_kernel(uint32_t nbt, uint32_t shift, u64 cap, const uint8_t* __restrict__ packed, const u64* __restrict__ block_off,
                                                             const uint8_t* __restrict__ stage, const uint8_t* __restrict__ cache, const u64* __restrict__ new_off,
                                                             const uint32_t* __restrict__ word, const uint32_t* __restrict__ cnt, uint8_t* __restrict__ dst)
{
	if (cnt[3] != 0) { return; }                                         // a refused table: nothing is written
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const u64 total = new_off[nbt], range = total < cap ? total : cap;
	u64 per = (range + gridDim.x - 1u) / gridDim.x;
	per = (per + 4095u) & ~(u64)4095u;
	const u64 lo = (u64)blockIdx.x * per;
	if (lo >= range) { return; }
	const u64 hi = range - lo < per ? range : lo + per;
	uint32_t j = 0, b = nbt;                                             // the first block with new_off[j + 1] > lo (there is one: new_off[nbt] > lo)
	while (j < b) { const uint32_t mid = j + (b - j) / 2u; if (new_off[mid + 1u] > lo) { b = mid; } else { j = mid + 1u; } }
	while (j < nbt) {
		const u64 o = new_off[j];
		if (o >= hi) { break; }
		const uint32_t row = j + lane;
		u64 e1 = 0;
		bool clean = false;
		if (row < nbt) { e1 = new_off[row + 1u]; clean = word[row] == WR_CLEAN && e1 <= cap; }
		const u64 others = ~__ballot(clean);
		const uint32_t k = others ? (uint32_t)__ffsll((unsigned long long)others) - 1u : 64u;   // clean rows from j on (the same in every wave of the block)
		const uint8_t* s = nullptr;
		u64 end = o;
		if (k) { end = __shfl(e1, (int)k - 1, 64); s = packed + block_off[j]; j += k; }
		else {
			const uint32_t wd = word[j];
			end = new_off[j + 1u];
			if (wd >= WR_DIRTY && end <= cap) { s = ((wd & 1u) ? stage : cache) + ((u64)((wd - WR_DIRTY) >> 1) << shift); }
			++j;
		}
		const u64 d0 = o > lo ? o : lo, d1 = end < hi ? end : hi;
		if (s && d0 < d1) { cpd_move<false>(dst + d0, s + (d0 - o), d1 - d0, tid); }
	}
}

void launch_writer_link(hipStream_t st, uint32_t n_req, uint32_t nbt, uint32_t m, const WriterTab& t)
{
	if (m == 0) { return; }
	launch_dev_zero(st, t.head, nbt);
	hipLaunchKernelGGL(wr_link_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, n_req, m, t);
}

void launch_writer_patch(hipStream_t st, uint32_t n_req, uint32_t m, uint32_t shift, const uint8_t* src, const u64* src_off, uint8_t* cache,
                         const WriterTab& t, uint32_t blocks)
{
	if (m == 0) { return; }
	const uint32_t ppu_shift = shift > RD_PIECE_SHIFT ? shift - RD_PIECE_SHIFT : 0u;
	const u64 need = (((u64)m << ppu_shift) + 255u) / 256u;                // a lane per item at the bound
	hipLaunchKernelGGL(wr_patch_kernel, dim3((uint32_t)(need < blocks ? need : blocks)), dim3(256), 0, st, n_req, m, shift, ppu_shift, src, src_off, cache, t);
	hipLaunchKernelGGL(wr_cunits_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, n_req, m, shift, cache, t);
}

void launch_writer_layout(hipStream_t st, uint32_t n_req, uint32_t n_res, uint32_t nbt, uint32_t m, u64 packed_len, u64 cap, const u64* block_first,
                          const u64* block_off, const uint32_t* block_crc, const WriterTab& t, u64* new_off, uint32_t* new_crc, u64* d_written,
                          int32_t* d_status, int32_t* d_res_status)
{
	hipLaunchKernelGGL(wr_layout_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_req, n_res, nbt, m, packed_len, cap, block_first, block_off, block_crc, t,
	                   new_off, new_crc, d_written, d_status, d_res_status);
}

void launch_writer_move(hipStream_t st, uint32_t nbt, uint32_t shift, u64 cap, const uint8_t* packed, const u64* block_off, const uint8_t* stage,
                        const uint8_t* cache, const u64* new_off, const WriterTab& t, uint8_t* dst, uint32_t blocks)
{
	if (nbt == 0) { return; }
	hipLaunchKernelGGL(wr_move_kernel, dim3(blocks), dim3(CPD_THREADS), 0, st, nbt, shift, cap, packed, block_off, stage, cache, new_off, t.head, t.r.cnt, dst);
}

} // namespace msc
