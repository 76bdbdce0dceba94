// search.hip -- the passes of a block searcher (mscomp_amd_searcher_*, include/mscomp_amd_search.h): where up to 64 byte patterns occur
// in byte ranges of a block container. The reader's passes (reader.hip, unchanged) own, decode, checksum and judge the covering blocks;
// the admission in front of them is a sibling of the reader's that counts the look-ahead blocks, and behind the fold the bytes are
// scanned where the reader would gather them: count per (unit, tile), a running sum, emit. DESIGN.md 4.24.
#include "kernels.h"

namespace msc {

// rd_req_kernel<false> (reader.hip) with one difference, the budget: the covering blocks of [o, min(L, o + w + look)), look = len_max - 1,
// so a hit that starts on the last position of the range has its tail decoded. A sibling and not a third instantiation: the reader's and
// the writer's admission keep their code object byte for byte.
__global__ __launch_bounds__(DV_THREADS) void sr_req_kernel(uint32_t n_req, uint32_t n_res, uint32_t nbt, uint32_t m, uint32_t shift, uint32_t look,
                                                           const u64* __restrict__ res_len, const u64* __restrict__ block_first, const u64* __restrict__ req, ReaderTab t)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const u64 B = (u64)1 << shift;
	u64 run[1] = {0}, cnt[1] = {0};
	if (tid == 0) { t.unit_first[0] = 0; t.cnt[0] = 0; t.cnt[1] = 0; }
	for (uint32_t base = 0; base < n_req; base += DV_THREADS) {
		const uint32_t q = base + tid;
		const bool live = q < n_req;
		int32_t st = 0;
		u64 o = 0, w = 0, j0 = 0, L = 0, c = 0;
		if (live) {
			const u64 r = req[3u * (size_t)q], off = req[3u * (size_t)q + 1u], len = req[3u * (size_t)q + 2u];
			if (r >= n_res) { st = -2; }                                       // MSCOMP_ARG_ERROR
			else {
				const u64 f0 = block_first[r], f1 = block_first[r + 1u];
				L = res_len[r];
				if (f0 > nbt || f1 > nbt) { st = -2; }
				else if (f1 - f0 != (L >> shift) + ((L & (B - 1u)) ? 1u : 0u)) { st = -3; }   // MSCOMP_DATA_ERROR (from here on L < 2^50)
				else {
					o = off < L ? off : L; w = len < L - o ? len : L - o;
					if (w) {
						const u64 end = L - (o + w) < look ? L : o + w + look;       // (o + w <= L: no wrap)
						c = ((end - 1u) >> shift) - (o >> shift) + 1u; j0 = f0 + (o >> shift);
					}
				}
			}
		}
		u64 v[1] = {c};
		dv_block_scan<1>(v, run, s_w);
		if (c && v[0] > m) { st = -2; c = 0; w = 0; }                       // over the budget: MSCOMP_ARG_ERROR
		u64 k[1] = {c};
		dv_block_scan<1>(k, cnt, s_w);
		if (live) { t.unit_first[q + 1u] = k[0]; t.q_off[q] = o; t.q_want[q] = w; t.q_j0[q] = j0; t.q_len[q] = L; t.q_stat[q] = st; }
	}
}

// One block. A lane per pattern: its offsets, its length (0: refused -- empty, longer than len_max, offsets running backwards), its
// status, its first four bytes. Then a thread per byte value: the four mask words of that value. The patterns are read here, on the
// device, and again by the prologue of every scan workgroup (its copy in LDS): whatever wrote them earlier on the stream is seen.
__global__ __launch_bounds__(256) void sr_pat_kernel(uint32_t n_pat, uint32_t len_max, const uint8_t* __restrict__ pat, const u64* __restrict__ pat_off, SearchTab s,
                                                    int32_t* __restrict__ pat_status)
{
	__shared__ uint32_t s_len[SR_PAT_MAX];
	__shared__ uint32_t s_b4[SR_PAT_MAX];
	const uint32_t tid = threadIdx.x;
	if (tid < SR_PAT_MAX) {
		uint32_t len = 0, b4 = 0;
		u64 a = 0;
		if (tid < n_pat) {
			a = pat_off[tid];
			const u64 b = pat_off[tid + 1u];
			if (b > a && b - a <= len_max) { len = (uint32_t)(b - a); }
			pat_status[tid] = len ? 0 : -2;                                // MSCOMP_ARG_ERROR
			for (uint32_t k = 0; k < 4u && k < len; ++k) { b4 |= (uint32_t)pat[a + k] << (8u * k); }
		}
		s_len[tid] = len; s_b4[tid] = b4; s.plen[tid] = len; s.poff[tid] = a;
	}
	__syncthreads();
	for (uint32_t k = 0; k < 4u; ++k) {
		u64 v = 0;
		for (uint32_t p = 0; p < n_pat; ++p) {
			const uint32_t len = s_len[p];
			if (len && (len <= k || ((s_b4[p] >> (8u * k)) & 0xFFu) == tid)) { v |= (u64)1 << p; }
		}
		s.mask[k * 256u + tid] = v;
	}
	if (tid < 8u) {
		u64 v = 0;
		for (uint32_t p = 0; p < n_pat; ++p) {
			const uint32_t len = s_len[p];
			if (len && (tid < 4u ? len <= tid : tid == 4u && len > 4u)) { v |= (u64)1 << p; }
		}
		s.aux[tid] = v;
	}
}

// a wave's tile in LDS: up to 15 bytes in front of the first position (the staging loads whole aligned 16-byte words), SR_TILE positions,
// SR_LEN_MAX - 1 bytes of look-ahead, and the word the filter's second dword load may touch behind them. With the tables (8.5 KiB) and
// the patterns' copy (n_pat len_max bytes, 16 KiB at the most) a workgroup holds 26 to 43 KiB of LDS
#define SR_LDS_TILE 4400u
static_assert(SR_LDS_TILE % 16u == 0 && SR_LDS_TILE >= 15u + SR_TILE + SR_LEN_MAX - 1u + 16u, "the staged tile fits");

// The patterns that occur at the position whose bytes lie at tile[idx ..]: b = its first four bytes (whatever lies there behind the
// resource's end), avail = the resource's bytes from the position on. The four mask words settle every pattern of up to four bytes; a
// longer one that survives them is compared from its fifth byte on with its copy in LDS (pattern p at s_pat + p len_max).
__device__ __forceinline__ u64 sr_hits_at(const u64* s_mask, const u64* s_aux, const uint32_t* s_plen, const uint8_t* s_pat, uint32_t len_max, const uint8_t* tile, uint32_t idx,
                                          u64 bytes, u64 avail)
{
	u64 c = s_mask[bytes & 0xFFu] & s_mask[256u + ((bytes >> 8) & 0xFFu)] & s_mask[512u + ((bytes >> 16) & 0xFFu)] & s_mask[768u + ((bytes >> 24) & 0xFFu)];
	if (avail < 4u) { c &= s_aux[avail]; }                                 // only what ends inside the resource
	u64 todo = c & s_aux[4];
	while (todo) {
		const uint32_t p = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
		todo &= todo - 1u;
		const uint32_t len = s_plen[p];
		bool ok = len <= avail;
		if (ok) {
			const uint8_t* g = s_pat + p * len_max;
			for (uint32_t j = 4u; j < len; ++j) { if (tile[idx + j] != g[j]) { ok = false; break; } }
		}
		if (!ok) { c &= ~((u64)1 << p); }
	}
	return c;
}

// Count (EMIT false) and emit (EMIT true), the same walk. A wave per item, the items dealt over a fixed grid. The item's start
// positions are those of its tile that lie in the request's range, [lo, hi); the bytes [lo, min(L, hi + len_max - 1)) are staged into the
// wave's LDS: the part in the unit's own block with aligned 16-byte loads from its owner's source (a cache slot, or a raw block at any
// address in d_packed; the first word may begin up to 15 bytes in front of lo, inside the same 16-byte word as a byte that is read),
// the part behind the block's end -- at most len_max - 1 bytes -- bytewise from the next unit's owner's source. A lane takes four
// consecutive positions of 256 per step, so lane order is position order: the (x, p) order of a tile's records is an exclusive prefix sum
// of the lanes' hit counts and, per lane, position by position, the set bits from the lowest on. The count pass leaves the item's hits in
// s.first[item]; the emit pass finds the item's first record there (launch_search_sum ran between) and skips an item without hits or
// with every record at or behind hits_max before it stages a byte.
template <bool EMIT>
__global__ __launch_bounds__(256) void sr_scan_kernel(uint32_t n_req, uint32_t shift, uint32_t n_pat, uint32_t len_max, u64 hits_max, const uint8_t* __restrict__ pat, SearchTab s,
                                                     ReaderTab t, u64* __restrict__ hits)
{
	__shared__ u64 s_mask[1024];
	__shared__ u64 s_aux[8];
	__shared__ uint32_t s_plen[SR_PAT_MAX];
	__shared__ __attribute__((aligned(16))) uint8_t s_tile[4][SR_LDS_TILE];
	extern __shared__ uint8_t s_pat[];                                     // n_pat len_max bytes (the launch's dynamic LDS)
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
	for (uint32_t i = tid; i < 1024u; i += 256u) { s_mask[i] = s.mask[i]; }
	if (tid < 8u) { s_aux[tid] = s.aux[tid]; }
	if (tid < SR_PAT_MAX) { s_plen[tid] = s.plen[tid]; }
	for (uint32_t i = tid; i < n_pat * len_max; i += 256u) {
		const uint32_t p = i / len_max, j = i - p * len_max;
		if (j < s.plen[p]) { s_pat[i] = pat[s.poff[p] + j]; }
	}
	__syncthreads();
	uint8_t* tile = s_tile[wv];
	const uint32_t* tile32 = reinterpret_cast<const uint32_t*>(tile);
	const uint32_t ts = shift - SR_TILE_SHIFT;
	const u64 B = (u64)1 << shift;
	const u64 items = t.unit_first[n_req] << ts, nw = (u64)gridDim.x * 4u;
	for (u64 it = (u64)blockIdx.x * 4u + wv; it < items; it += nw) {
		u64 run = 0;
		if (EMIT) {
			run = s.first[it];
			if (s.first[it + 1u] == run || run >= hits_max) { continue; }
		}
		const uint32_t u = (uint32_t)(it >> ts), q = t.uq[u];
		u64 lo = 0, hi = 0, L = 0, b0 = 0, e = 0;
		if (t.q_stat[q] == 0) {
			const u64 o = t.q_off[q], end = o + t.q_want[q];
			L = t.q_len[q];
			b0 = ((o >> shift) + (u - t.unit_first[q])) << shift;          // (< L: the unit covers bytes of the resource)
			e = L - b0 < B ? L - b0 : B;
			const u64 t0 = b0 + ((it & (((u64)1 << ts) - 1u)) << SR_TILE_SHIFT), t1 = t0 + SR_TILE < b0 + e ? t0 + SR_TILE : b0 + e;
			lo = o > t0 ? o : t0; hi = end < t1 ? end : t1;
		}
		if (lo >= hi) {                                                    // no start position: another request's status, the look-ahead block, a tile outside the range
			if (!EMIT && lane == 0) { s.first[it] = 0; }
			continue;
		}
		const u64 need = L - hi < (u64)(len_max - 1u) ? L : hi + (len_max - 1u), a_end = need < b0 + e ? need : b0 + e;
		const uint32_t n_a = (uint32_t)(a_end - lo), n_b = (uint32_t)(need - a_end);   // (n_b > 0: e = B and hi + len_max - 1 > b0 + B, so unit u + 1 is the request's too)
		const u64 src = t.src[t.owner[u]] + (lo - b0);
		const uint32_t head = (uint32_t)(src & 15u);
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");      // (the lanes' reads of the item before)
		{
			const uint4* __restrict__ g = reinterpret_cast<const uint4*>((uintptr_t)(src - head));
			uint4* d = reinterpret_cast<uint4*>(tile);
			const uint32_t ng = (head + n_a + 15u) >> 4;                       // (<= 273 words: 4368 bytes)
			for (uint32_t k = lane; k < ng; k += 64u) { d[k] = g[k]; }
		}
		if (n_b) {
			const uint8_t* __restrict__ g = reinterpret_cast<const uint8_t*>((uintptr_t)t.src[t.owner[u + 1u]]);
			for (uint32_t i = lane; i < n_b; i += 64u) { tile[head + n_a + i] = g[i]; }
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local");
		const uint32_t span = head + (uint32_t)(hi - lo);                  // the start positions are the LDS bytes [head, span)
		uint32_t total = 0;
		for (uint32_t i0 = 0; i0 < span; i0 += 256u) {
			if (EMIT && run >= hits_max) { break; }
			const uint32_t idx = i0 + 4u * lane;
			u64 h[4] = {0, 0, 0, 0};
			uint32_t n = 0;
			if (idx < span && idx + 4u > head) {
				const u64 ww = (u64)tile32[idx >> 2] | ((u64)tile32[(idx >> 2) + 1u] << 32);
				#pragma unroll
				for (uint32_t k = 0; k < 4u; ++k) {
					const uint32_t i = idx + k;
					if (i >= head && i < span) {
						const u64 x = lo + (i - head);
						h[k] = sr_hits_at(s_mask, s_aux, s_plen, s_pat, len_max, tile, i, ww >> (8u * k), L - x);
						n += (uint32_t)__popcll(h[k]);
					}
				}
			}
			uint32_t inc = n;
			#pragma unroll
			for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) { inc += o; } }
			const uint32_t tot = __shfl(inc, 63, 64);
			if (EMIT && n) {
				u64 r = run + (inc - n);
				#pragma unroll
				for (uint32_t k = 0; k < 4u; ++k) {
					const u64 x = lo + (idx + k - head);
					u64 bits = h[k];
					while (bits) {
						const uint32_t p = (uint32_t)__ffsll((unsigned long long)bits) - 1u;
						bits &= bits - 1u;
						if (r < hits_max) { hits[2u * r] = x; hits[2u * r + 1u] = ((u64)q << 32) | p; }
						++r;
					}
				}
			}
			run += tot; total += tot;
		}
		if (!EMIT && lane == 0) { s.first[it] = total; }
	}
}

// One block: s.first[0 .. items) from the items' hit counts to their exclusive running sum, in place, s.first[items] = the total; count;
// then a thread per request: the hits between its first unit's first item and the next request's (a request that is not MSCOMP_OK has
// only empty items).
__global__ __launch_bounds__(DV_THREADS) void sr_sum_kernel(uint32_t n_req, uint32_t shift, u64 hits_max, SearchTab s, ReaderTab t, u64* __restrict__ req_hits, u64* __restrict__ count)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x, ts = shift - SR_TILE_SHIFT;
	const u64 items = t.unit_first[n_req] << ts;
	u64 run[1] = {0};
	for (u64 base = 0; base < items; base += DV_THREADS) {
		const u64 i = base + tid;
		const u64 c = i < items ? s.first[i] : 0;
		u64 v[1] = {c};
		dv_block_scan<1>(v, run, s_w);
		if (i < items) { s.first[i] = v[0] - c; }
	}
	if (tid == 0) { s.first[items] = run[0]; count[0] = run[0]; count[1] = run[0] < hits_max ? run[0] : hits_max; }
	__syncthreads();
	for (uint32_t q = tid; q < n_req; q += DV_THREADS) { req_hits[q] = s.first[t.unit_first[q + 1u] << ts] - s.first[t.unit_first[q] << ts]; }
}

void launch_search_requests(hipStream_t st, uint32_t n_req, uint32_t n_res, uint32_t nbt, uint32_t m, uint32_t shift, uint32_t look, const u64* res_len,
                            const u64* block_first, const u64* req, const ReaderTab& t)
{
	hipLaunchKernelGGL(sr_req_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_req, n_res, nbt, m, shift, look, res_len, block_first, req, t);
}

void launch_search_patterns(hipStream_t st, uint32_t n_pat, uint32_t len_max, const uint8_t* pat, const u64* pat_off, const SearchTab& s, int32_t* pat_status)
{
	hipLaunchKernelGGL(sr_pat_kernel, dim3(1), dim3(256), 0, st, n_pat, len_max, pat, pat_off, s, pat_status);
}

void launch_search_count(hipStream_t st, uint32_t n_req, uint32_t m, uint32_t shift, uint32_t n_pat, uint32_t len_max, const uint8_t* pat, const SearchTab& s, const ReaderTab& t,
                         uint32_t blocks)
{
	if (m == 0) { return; }
	hipLaunchKernelGGL(sr_scan_kernel<false>, fixed_grid((u64)m << (shift - SR_TILE_SHIFT), 4u, blocks), dim3(256), n_pat * len_max, st, n_req, shift, n_pat, len_max, (u64)0, pat,
	                   s, t, static_cast<u64*>(nullptr));
}

void launch_search_sum(hipStream_t st, uint32_t n_req, uint32_t shift, u64 hits_max, const SearchTab& s, const ReaderTab& t, u64* req_hits, u64* count)
{
	hipLaunchKernelGGL(sr_sum_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_req, shift, hits_max, s, t, req_hits, count);
}

void launch_search_emit(hipStream_t st, uint32_t n_req, uint32_t m, uint32_t shift, uint32_t n_pat, uint32_t len_max, u64 hits_max, const uint8_t* pat, const SearchTab& s,
                        const ReaderTab& t, u64* hits, uint32_t blocks)
{
	if (m == 0 || hits_max == 0) { return; }
	hipLaunchKernelGGL(sr_scan_kernel<true>, fixed_grid((u64)m << (shift - SR_TILE_SHIFT), 4u, blocks), dim3(256), n_pat * len_max, st, n_req, shift, n_pat, len_max, hits_max, pat,
	                   s, t, hits);
}

} // namespace msc
