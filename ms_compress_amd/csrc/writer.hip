// writer.hip -- the passes of a block writer (mscomp_amd_writer_*, include/mscomp_amd.h): a batch of byte-range writes into a block container,
// out of place. The requests are admitted, the covering blocks get their owners, and the owners' blocks are decoded, checksummed and folded
// into verdicts by the reader's passes (reader.hip, unchanged: a write reads every block it touches first). Behind the fold the passes of
// this file load the raw owners into their cache slots and apply the MSCOMP_OK requests in request order, hand the dirty blocks to a
// compress dev plan and the CRC kernels (blockobj.hip runs both between these passes, unchanged) and lay the new container out around them:
// every block's new offset, checksum and the ADDRESS of its stored bytes -- a clean one's in the old container, a dirty one's in the staging
// area or the cache --, which the containers' move pass (blocks.hip bk_move_kernel) carries to their new places. DESIGN.md 4.10.
// mscomp_amd_writer_resize (the rs_* kernels below) is the writer's second call: every resource cut or zero-extended to a
// wanted length, the one block whose data length changes and the fresh blocks as the units, the same inner plans, CRC kernels and scratch.
#include "kernels.h"

namespace msc {

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

// Unit u of the inner compress plan and of the CRC kernels: with `on`, the e data bytes in its cache slot in, its staging slot out, capacity
// e - 1 as a block container gives it; otherwise empty in both (e = 0).
__device__ __forceinline__ void wr_cunit(const ReaderTab& r, uint32_t u, bool on, u64 e, uint32_t shift, const uint8_t* __restrict__ cache)
{
	const u64 at = on ? (u64)u << shift : 0;
	r.in_off[u] = at; r.in_len[u] = e; r.out_off[u] = at; r.out_cap[u] = on ? e - 1u : 0;
	r.src[u] = on ? (u64)(uintptr_t)(cache + at) : 0; r.clen[u] = e;
}

// One thread per possible unit, behind the patch: a dirty owner becomes a unit of the inner compress plan and of the CRC kernels; every
// other unit is empty in both. The columns are the ones the decompress plan and the old blocks' CRC used: the fold has read them.
__global__ __launch_bounds__(256) void wr_cunits_kernel(uint32_t n_req, uint32_t m, uint32_t shift, const uint8_t* __restrict__ cache, WriterTab t)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u >= m) { return; }
	const bool d = u < t.r.unit_first[n_req] && t.dirty[u] != 0;
	wr_cunit(t.r, u, d, d ? t.r.act[u] >> 2 : 0, shift, cache);
}

// Rule 0, asked by a whole block of DV_THREADS: the table as a whole (block_first[n_res] within the table, block_first never decreasing)
__device__ __forceinline__ bool wr_table_bad(uint32_t n_res, uint32_t nbt, const u64* __restrict__ block_first)
{
	int wrong = block_first[n_res] > nbt ? 1 : 0;
	for (uint32_t i = threadIdx.x; i < n_res; i += DV_THREADS) { if (block_first[i] > block_first[i + 1u]) { wrong = 1; } }
	return __syncthreads_or(wrong) != 0;
}

// One row of a new table: its stored length, checksum and where its stored bytes lie. A dirty row is unit u with e data bytes: its stored
// form by bk_select_kernel's rule from the compress plan's results (the staged bytes when they fitted into e - 1, the raw block in the cache
// otherwise). A clean row is row `old` of the old table, length 0 for an entry that cannot be read.
__device__ __forceinline__ void wr_row(const ReaderTab& r, bool dirty, u64 u, u64 e, uint32_t shift, const uint8_t* __restrict__ stage, const uint8_t* __restrict__ cache,
                                       u64 old, const uint8_t* __restrict__ packed, u64 packed_len, const u64* __restrict__ block_off, const uint32_t* __restrict__ block_crc,
                                       u64& len, uint32_t& crc, u64& at)
{
	if (dirty) {
		const bool comp = r.ustat[u] == 0 && r.ulen[u] < e;
		len = comp ? r.ulen[u] : e; crc = r.ucrc[u]; at = (u64)(uintptr_t)((comp ? stage : cache) + (u << shift));
	} else {
		const u64 o0 = block_off[old], o1 = block_off[old + 1u];
		len = o0 <= o1 && o1 <= packed_len ? o1 - o0 : 0; crc = block_crc ? block_crc[old] : 0u; at = (u64)(uintptr_t)(packed + o0);
	}
}

// Layout, one block. Rule 0 first. Then one scan over the block table: every block's row (wr_row: a dirty owner's block, or the same row
// of the old table), new_block_off, the merged CRC table, and the move pass's address per block -- 0 for a block without stored bytes or
// ending beyond cap. Then the resources' statuses by the capacity rule of a block container; a refused table is all empty rows (new_off
// all zeros: the move pass has no range), and overwrites what the fold reported for the requests.
__global__ __launch_bounds__(DV_THREADS) void wr_layout_kernel(uint32_t n_req, uint32_t n_res, uint32_t nbt, uint32_t m, uint32_t shift, u64 packed_len, u64 cap,
                                                              const uint8_t* __restrict__ packed, const uint8_t* __restrict__ stage, const uint8_t* __restrict__ cache,
                                                              const u64* __restrict__ block_first, const u64* __restrict__ block_off, const uint32_t* __restrict__ block_crc,
                                                              WriterTab t, u64* new_off, uint32_t* __restrict__ new_crc, u64* __restrict__ d_written,
                                                              int32_t* __restrict__ d_status, int32_t* __restrict__ d_res_status)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const ReaderTab& r = t.r;
	const u64 nb = block_first[n_res];
	const bool bad = wr_table_bad(n_res, nbt, block_first);
	if (tid == 0) { r.cnt[3] = bad ? 1u : 0u; new_off[0] = 0; }
	u64 run[1] = {0};
	for (uint32_t base = 0; base < nbt; base += DV_THREADS) {
		const uint32_t j = base + tid;
		const bool live = j < nbt;
		u64 len = 0, at = 0;
		uint32_t crc = 0;
		if (live && !bad && j < nb) {
			const uint32_t bid = m ? r.own[j] : 0u, o = ~bid;                 // (own is cleared and bid for only when a call can have units)
			const bool dirty = bid != 0 && t.dirty[o] != 0;
			wr_row(r, dirty, o, dirty ? r.act[o] >> 2 : 0, shift, stage, cache, j, packed, packed_len, block_off, block_crc, len, crc, at);
		}
		u64 v[1] = {len};
		dv_block_scan<1>(v, run, s_w);
		if (live) { new_off[j + 1u] = v[0]; t.addr[j] = (len != 0 && v[0] <= cap) ? at : 0; if (new_crc) { new_crc[j] = crc; } }
	}
	__syncthreads();                                                     // new_off is read back below, by other threads of this block
	for (uint32_t i = tid; i < n_res; i += DV_THREADS) {
		const u64 f0 = block_first[i], f1 = block_first[i + 1u];
		d_res_status[i] = bad ? -2 : (f1 > f0 && new_off[f1] > cap) ? -5 : 0;   // MSCOMP_ARG_ERROR; MSCOMP_BUF_ERROR (the offsets only grow: the last block tells)
	}
	if (bad) { for (uint32_t q = tid; q < n_req; q += DV_THREADS) { d_status[q] = -2; d_written[q] = 0; } }
}

// ---- resize (mscomp_amd_writer_resize) ----
// A resource of L bytes in n blocks becomes one of W bytes in n2 = ceil(W / B). Of the blocks both have, only the last one, kc, can change
// its data length (e -> e2): it is the resource's unit 0 when it does; the fresh blocks n .. n2 - 1 are the units behind it. Only called
// for a resource that passed rule 1 (n = ceil(L / B) < 2^31), so no product below overflows.
struct RsGeo { u64 n2, kc, cnt; uint32_t e, e2; bool changed; };
__device__ __forceinline__ RsGeo rs_geo(u64 L, u64 W, u64 n, uint32_t shift)
{
	const u64 B = (u64)1 << shift;
	RsGeo g;
	g.n2 = (W >> shift) + ((W & (B - 1u)) ? 1u : 0u);
	const u64 mn = n < g.n2 ? n : g.n2;
	g.kc = 0; g.e = 0; g.e2 = 0; g.changed = false;
	if (mn) {
		g.kc = mn - 1u;
		const u64 l = L - (g.kc << shift), w = W - (g.kc << shift);
		g.e = (uint32_t)(l < B ? l : B); g.e2 = (uint32_t)(w < B ? w : B); g.changed = g.e != g.e2;
	}
	g.cnt = (g.changed ? 1u : 0u) + (g.n2 > n ? g.n2 - n : 0u);
	return g;
}

// One block walks the resources in tiles of 1024. Rule 0 first (a refused table has no units, cnt[3] says so to the passes behind). Then
// rules 1-3 per resource, as rd_req_kernel runs the reader's: the cost of every resource that passed rules 1 and 2 in one scan (the
// budget's running total, refused ones included), the cost of the admitted ones in a second (the unit numbering, ru_first).
__global__ __launch_bounds__(DV_THREADS) void rs_res_kernel(uint32_t n_res, uint32_t nbt, uint32_t m, uint32_t shift, const u64* __restrict__ block_first,
                                                           const u64* __restrict__ res_len, const u64* __restrict__ want, ResizeTab t)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const u64 B = (u64)1 << shift;
	const bool bad = wr_table_bad(n_res, nbt, block_first);
	if (tid == 0) { t.ru_first[0] = 0; t.w.r.cnt[0] = 0; t.w.r.cnt[1] = 0; t.w.r.cnt[2] = 0; t.w.r.cnt[3] = bad ? 1u : 0u; }
	u64 run[1] = {0}, acc[1] = {0};
	for (uint32_t base = 0; base < n_res; base += DV_THREADS) {
		const uint32_t r = base + tid;
		const bool live = r < n_res;
		int32_t st = 0;
		u64 c = 0;
		bool moves = false;
		if (live && bad) { st = -2; }                                       // MSCOMP_ARG_ERROR
		else if (live) {
			const u64 f0 = block_first[r], n = block_first[r + 1u] - f0, L = res_len[r], W = want[r];
			if (n != (L >> shift) + ((L & (B - 1u)) ? 1u : 0u)) { st = -3; }    // MSCOMP_DATA_ERROR
			else if (W != L) { moves = true; c = rs_geo(L, W, n, shift).cnt; }
		}
		u64 v[1] = {c};
		dv_block_scan<1>(v, run, s_w);                                    // running total of the costs, this resource included
		if (moves && v[0] > m) { st = -2; c = 0; }                          // over the budget, as everything that changes behind it
		u64 k[1] = {c};
		dv_block_scan<1>(k, acc, s_w);
		if (live) { t.ru_first[r + 1u] = k[0]; t.rstat[r] = st; }
	}
}

// One thread per possible unit: its resource (binary search in ru_first) and its block. A changed block runs the container's table checks
// as rd_units_kernel runs them and becomes a unit of the inner decompress plan (cache slot u B, capacity e) or, raw, is read in d_packed;
// a fresh block has nothing to read. r.owner[u] = e2, the data length the unit will have. cnt[0] counts the changed blocks.
__global__ __launch_bounds__(256) void rs_units_kernel(uint32_t n_res, uint32_t m, uint32_t shift, u64 packed_len, const uint8_t* __restrict__ packed,
                                                      const uint8_t* __restrict__ cache, const u64* __restrict__ block_first, const u64* __restrict__ block_off,
                                                      const u64* __restrict__ res_len, const u64* __restrict__ want, ResizeTab t)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u >= m) { return; }
	const ReaderTab& rt = t.w.r;
	const u64 B = (u64)1 << shift;
	u64 io = 0, il = 0, oo = 0, oc = 0, sa = 0, cl = 0;
	uint32_t a = RD_SKIP, e2 = 0;
	bool chg = false;
	if (u < t.ru_first[n_res]) {
		const uint32_t r = res_of_block(t.ru_first, n_res, u);
		const u64 f0 = block_first[r], n = block_first[r + 1u] - f0, W = want[r], idx = u - t.ru_first[r];
		const RsGeo g = rs_geo(res_len[r], W, n, shift);
		u64 k;
		if (g.changed && idx == 0) {
			chg = true; k = g.kc; e2 = g.e2;
			const u64 j = f0 + k, e = g.e, o0 = block_off[j], o1 = block_off[j + 1u];   // (j < block_first[r + 1] <= nbt: rule 0)
			if (o1 < o0 || o1 > packed_len) { a = RD_FAIL; }
			else {
				const u64 s = o1 - o0;
				if (s == e) { a = RD_COPY; sa = (u64)(uintptr_t)(packed + o0); cl = e; }
				else if (s != 0 && s < e) { a = RD_DECODE; io = o0; il = s; oo = (u64)u << shift; oc = e; sa = (u64)(uintptr_t)(cache + oo); cl = e; }
				else { a = RD_FAIL; }
			}
			a |= (uint32_t)e << 2;
		} else {
			k = n + idx - (g.changed ? 1u : 0u);                              // (< n2 <= n + m < 2^32)
			const u64 left = W - (k << shift);
			e2 = (uint32_t)(left < B ? left : B);
		}
		rt.uq[u] = r; rt.ublk[u] = (uint32_t)k;
	}
	rt.in_off[u] = io; rt.in_len[u] = il; rt.out_off[u] = oo; rt.out_cap[u] = oc; rt.src[u] = sa; rt.clen[u] = cl; rt.act[u] = a; rt.owner[u] = e2;
	const u64 changed = __ballot(chg);
	if ((threadIdx.x & 63u) == 0 && changed) { atomicAdd(&rt.cnt[0], (uint32_t)__popcll(changed)); }
}

// One thread per resource, behind the decompress plan and the CRC kernels: rule 4, the verdict on its changed block as rd_fold_kernel folds
// an owner's (a failed table check; a decoder status other than MSCOMP_OK or a length other than e; with block_crc, another CRC-32).
__global__ __launch_bounds__(256) void rs_fold_kernel(uint32_t n_res, uint32_t shift, const u64* __restrict__ block_first, const u64* __restrict__ res_len,
                                                     const u64* __restrict__ want, const uint32_t* __restrict__ block_crc, ResizeTab t)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r >= n_res || t.rstat[r] != 0 || t.ru_first[r] == t.ru_first[r + 1u]) { return; }
	const ReaderTab& rt = t.w.r;
	const u64 f0 = block_first[r];
	const RsGeo g = rs_geo(res_len[r], want[r], block_first[r + 1u] - f0, shift);
	if (!g.changed) { return; }
	const u64 o = t.ru_first[r];
	const uint32_t a = rt.act[o], kind = a & 3u;
	bool bad = kind == RD_FAIL || (kind == RD_DECODE && (rt.ustat[o] != 0 || rt.ulen[o] != (u64)(a >> 2)));
	if (!bad && block_crc && rt.ucrc[o] != block_crc[f0 + g.kc]) { bad = true; }
	if (bad) { t.rstat[r] = -3; }                                         // MSCOMP_DATA_ERROR: the resource is carried
}

// cnt zero bytes at dst by one wave, in the shape of rd_wave_move's stores: a bytewise head up to the next 16-byte boundary, 16-byte
// stores, a bytewise tail (lanes 16..30)
__device__ __forceinline__ void rs_wave_zero(uint8_t* __restrict__ dst, uint32_t cnt, uint32_t lane)
{
	uint32_t head = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
	if (head > cnt) { head = cnt; }
	const uint32_t body = (cnt - head) >> 4, tail0 = head + body * 16u;
	if (lane < head) { dst[lane] = 0; }
	if (lane >= 16u && tail0 + (lane - 16u) < cnt) { dst[tail0 + (lane - 16u)] = 0; }
	uint4* __restrict__ d16 = reinterpret_cast<uint4*>(dst + head);
	for (uint32_t k = lane; k < body; k += 64u) { d16[k] = make_uint4(0, 0, 0, 0); }
}

// Trim and fill: the new data of the accepted resources' units, in their cache slots. An item is one (unit, 16 KiB piece) pair dealt to the
// waves of a fixed grid as wr_patch_kernel deals them. Of a changed block the first min(e, e2) bytes stay -- a decoded one has them in its
// slot, a raw one's piece is loaded from d_packed --, the bytes from there to e2 are zeros; a fresh block is e2 zeros.
__global__ __launch_bounds__(256) void rs_fill_kernel(uint32_t n_res, uint32_t shift, uint32_t ppu_shift, uint8_t* __restrict__ cache, ResizeTab t)
{
	const ReaderTab& rt = t.w.r;
	const uint32_t lane = threadIdx.x & 63u;
	const u64 items = t.ru_first[n_res] << ppu_shift, nw = (u64)gridDim.x * 4u, w = (u64)blockIdx.x * 4u + (threadIdx.x >> 6);
	u64 per = (items + nw - 1u) / nw;
	per = per < 1u ? 1u : per > 64u ? 64u : per;
	for (u64 base = w * per; base < items; base += nw * per) {
		uint32_t o = 0, a0 = 0, a1 = 0, keep = 0;
		u64 sa = 0;
		const u64 i = base + lane;
		if (lane < per && i < items) {
			const uint32_t u = (uint32_t)(i >> ppu_shift), e2 = rt.owner[u];
			const u64 at = (i & (((u64)1 << ppu_shift) - 1u)) << RD_PIECE_SHIFT;
			if (t.rstat[rt.uq[u]] == 0 && at < e2) {
				const uint32_t a = rt.act[u], e = a >> 2;                      // (a fresh block: RD_SKIP, e = 0)
				o = u; a0 = (uint32_t)at; a1 = e2 - at < ((u64)1 << RD_PIECE_SHIFT) ? e2 : (uint32_t)at + (1u << RD_PIECE_SHIFT);
				keep = e < e2 ? e : e2;
				if ((a & 3u) == RD_COPY) { sa = rt.src[u]; }
			}
		}
		u64 todo = __ballot(a1 > a0);
		while (todo) {
			const int l = __ffsll((unsigned long long)todo) - 1;
			todo &= todo - 1u;
			const uint32_t b0 = __shfl(a0, l, 64), b1 = __shfl(a1, l, 64), kp = __shfl(keep, l, 64);
			const u64 s = __shfl(sa, l, 64);
			uint8_t* slot = cache + ((u64)__shfl(o, l, 64) << shift);
			const uint32_t c1 = kp < b1 ? kp : b1, z0 = kp > b0 ? kp : b0;
			if (s && b0 < c1) { rd_wave_move(slot + b0, reinterpret_cast<const uint8_t*>((uintptr_t)s) + b0, c1 - b0, lane); }
			if (z0 < b1) { rs_wave_zero(slot + z0, b1 - z0, lane); }
		}
	}
}

// One thread per possible unit, behind the fill: a unit of an accepted resource becomes a unit of the inner compress plan and of the CRC
// kernels, e2 bytes long, as wr_cunits_kernel makes a dirty owner one; every other unit is empty in both. cnt[2] counts them: the blocks encoded.
__global__ __launch_bounds__(256) void rs_cunits_kernel(uint32_t n_res, uint32_t m, uint32_t shift, const uint8_t* __restrict__ cache, ResizeTab t)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u >= m) { return; }
	const ReaderTab& rt = t.w.r;
	const bool d = u < t.ru_first[n_res] && t.rstat[rt.uq[u]] == 0;
	wr_cunit(rt, u, d, d ? rt.owner[u] : 0, shift, cache);
	t.w.dirty[u] = d ? 1u : 0u;
	const u64 enc = __ballot(d);
	if ((threadIdx.x & 63u) == 0 && enc) { atomicAdd(&rt.cnt[2], (uint32_t)__popcll(enc)); }
}

// Layout, one block. A scan over the resources gives the final block counts -- n2 for an accepted resource, n for a carried one -- and
// new_first; rule 8 holds their sum against the table. A scan over the NEW table rows then gives every row its stored length, checksum and
// address (wr_row): a row finds its resource by binary search in new_first and is the changed block or a fresh one of an accepted
// resource -- dirty -- or a kept block, clean at old row block_first[r] + k. Then the resources' statuses and lengths. A refused table
// (rule 0 or 8) writes zeros and MSCOMP_ARG_ERROR only: new_off is all zeros, the move pass has no range and reads no address.
__global__ __launch_bounds__(DV_THREADS) void rs_layout_kernel(uint32_t n_res, uint32_t nbt, uint32_t shift, u64 packed_len, u64 cap, const uint8_t* __restrict__ packed,
                                                              const uint8_t* __restrict__ stage, const uint8_t* __restrict__ cache, const u64* __restrict__ block_first,
                                                              const u64* __restrict__ block_off, const u64* __restrict__ res_len, const u64* __restrict__ want,
                                                              const uint32_t* __restrict__ block_crc, ResizeTab t, u64* new_first, u64* new_off,
                                                              uint32_t* __restrict__ new_crc, u64* __restrict__ new_len, int32_t* __restrict__ res_status)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const ReaderTab& rt = t.w.r;
	const u64 B = (u64)1 << shift;
	const bool bad0 = rt.cnt[3] != 0;
	u64 run[1] = {0};
	if (tid == 0) { new_first[0] = 0; new_off[0] = 0; }
	for (uint32_t base = 0; base < n_res; base += DV_THREADS) {
		const uint32_t r = base + tid;
		const bool live = r < n_res;
		u64 c = 0;
		if (live && !bad0) {
			c = block_first[r + 1u] - block_first[r];
			if (t.rstat[r] == 0) { const u64 W = want[r]; c = (W >> shift) + ((W & (B - 1u)) ? 1u : 0u); }   // (W = L: the same count)
		}
		u64 v[1] = {c};
		dv_block_scan<1>(v, run, s_w);
		if (live) { new_first[r + 1u] = v[0]; }
	}
	const u64 nbn = run[0];
	__syncthreads();                                                     // new_first is read back below, by other threads of this block; cnt[3] was read above
	if (bad0 || nbn > nbt) {
		if (tid == 0) { rt.cnt[3] = 1u; }
		for (uint32_t i = tid; i <= n_res; i += DV_THREADS) { new_first[i] = 0; if (i < n_res) { new_len[i] = 0; res_status[i] = -2; } }
		for (uint32_t j = tid; j <= nbt; j += DV_THREADS) { new_off[j] = 0; if (new_crc && j < nbt) { new_crc[j] = 0; } }
		return;
	}
	u64 sum[1] = {0};
	for (uint32_t base = 0; base < nbt; base += DV_THREADS) {
		const uint32_t j = base + tid;
		const bool live = j < nbt;
		u64 len = 0, at = 0;
		uint32_t crc = 0;
		if (live && j < nbn) {
			const uint32_t r = res_of_block(new_first, n_res, j);
			const u64 k = j - new_first[r], f0 = block_first[r], n = block_first[r + 1u] - f0, L = res_len[r], W = want[r];
			bool dirty = false;
			u64 u = 0, e2 = 0;
			if (t.rstat[r] == 0 && W != L) {
				const RsGeo g = rs_geo(L, W, n, shift);
				if (g.changed && k == g.kc) { dirty = true; u = t.ru_first[r]; e2 = g.e2; }
				else if (k >= n) { dirty = true; u = t.ru_first[r] + (g.changed ? 1u : 0u) + (k - n); const u64 left = W - (k << shift); e2 = left < B ? left : B; }
			}
			wr_row(rt, dirty, u, e2, shift, stage, cache, f0 + k, packed, packed_len, block_off, block_crc, len, crc, at);
		}
		u64 v[1] = {len};
		dv_block_scan<1>(v, sum, s_w);
		if (live) { new_off[j + 1u] = v[0]; t.w.addr[j] = (len != 0 && v[0] <= cap) ? at : 0; if (new_crc) { new_crc[j] = crc; } }
	}
	__syncthreads();                                                     // new_off is read back below
	for (uint32_t r = tid; r < n_res; r += DV_THREADS) {
		const u64 n0 = new_first[r], n1 = new_first[r + 1u];
		const int32_t st = t.rstat[r];
		res_status[r] = (n1 > n0 && new_off[n1] > cap) ? -5 : st;           // MSCOMP_BUF_ERROR replaces what the resource had (the offsets only grow: the last block tells)
		new_len[r] = st == 0 ? want[r] : res_len[r];
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

void launch_writer_layout(hipStream_t st, uint32_t n_req, uint32_t n_res, uint32_t nbt, uint32_t m, uint32_t shift, u64 packed_len, u64 cap, const uint8_t* packed,
                          const uint8_t* stage, const uint8_t* cache, const u64* block_first, const u64* block_off, const uint32_t* block_crc, const WriterTab& t,
                          u64* new_off, uint32_t* new_crc, u64* d_written, int32_t* d_status, int32_t* d_res_status)
{
	hipLaunchKernelGGL(wr_layout_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_req, n_res, nbt, m, shift, packed_len, cap, packed, stage, cache, block_first, block_off,
	                   block_crc, t, new_off, new_crc, d_written, d_status, d_res_status);
}

void launch_resize_units(hipStream_t st, uint32_t n_res, uint32_t nbt, uint32_t m, uint32_t shift, u64 packed_len, const uint8_t* packed, const uint8_t* cache,
                         const u64* block_first, const u64* block_off, const u64* res_len, const u64* want, const ResizeTab& t)
{
	hipLaunchKernelGGL(rs_res_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_res, nbt, m, shift, block_first, res_len, want, t);
	if (m == 0) { return; }
	hipLaunchKernelGGL(rs_units_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, n_res, m, shift, packed_len, packed, cache, block_first, block_off, res_len, want, t);
}

void launch_resize_fold(hipStream_t st, uint32_t n_res, uint32_t m, uint32_t shift, const u64* block_first, const u64* res_len, const u64* want,
                        const uint32_t* block_crc, const ResizeTab& t)
{
	if (m == 0 || n_res == 0) { return; }
	hipLaunchKernelGGL(rs_fold_kernel, dim3((n_res + 255u) / 256u), dim3(256), 0, st, n_res, shift, block_first, res_len, want, block_crc, t);
}

void launch_resize_fill(hipStream_t st, uint32_t n_res, uint32_t m, uint32_t shift, uint8_t* cache, const ResizeTab& t, uint32_t blocks)
{
	if (m == 0) { return; }
	const uint32_t ppu_shift = shift > RD_PIECE_SHIFT ? shift - RD_PIECE_SHIFT : 0u;
	const u64 need = (((u64)m << ppu_shift) + 255u) / 256u;                // a lane per item at the bound
	hipLaunchKernelGGL(rs_fill_kernel, dim3((uint32_t)(need < blocks ? need : blocks)), dim3(256), 0, st, n_res, shift, ppu_shift, cache, t);
	hipLaunchKernelGGL(rs_cunits_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, n_res, m, shift, cache, t);
}

void launch_resize_layout(hipStream_t st, uint32_t n_res, uint32_t nbt, uint32_t shift, u64 packed_len, u64 cap, const uint8_t* packed, const uint8_t* stage,
                          const uint8_t* cache, const u64* block_first, const u64* block_off, const u64* res_len, const u64* want, const uint32_t* block_crc,
                          const ResizeTab& t, u64* new_first, u64* new_off, uint32_t* new_crc, u64* new_len, int32_t* res_status)
{
	hipLaunchKernelGGL(rs_layout_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_res, nbt, shift, packed_len, cap, packed, stage, cache, block_first, block_off, res_len, want,
	                   block_crc, t, new_first, new_off, new_crc, new_len, res_status);
}

} // namespace msc
