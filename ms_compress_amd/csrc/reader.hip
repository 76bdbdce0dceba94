// reader.hip -- the passes of a block reader (mscomp_amd_reader_*, include/mscomp_amd.h): a batch of byte-range requests against the tables
// a block container wrote. The requests are checked and counted, every covering block gets one owner among the (request, block) pairs that
// want it, the owners' blocks are decoded into a cache by a decompress dev plan over them as units (blockobj.hip runs it between these passes,
// unchanged) or read where they lie when stored raw, optionally held to their CRC-32 (crc32.hip, unchanged), the verdicts are folded per
// request, and only then the slices move to the caller's buffer. DESIGN.md 4.9.
#include "kernels.h"

namespace msc {

// One block walks the requests in tiles of 1024: checks 1-5 of the header in their order, the clipped range, the first covering block, and
// unit_first (n + 1). Two scans: the covering blocks of every request that passed checks 1-4 (the budget's running total, which does not
// know about sharing), and those of the admitted requests (the unit numbering). CAP: check 4, the reader's capacity rule -- a block writer
// (writer.hip) admits its requests with the same pass and has no such rule (out_cap is not read).
template <bool CAP>
__global__ __launch_bounds__(DV_THREADS) void rd_req_kernel(uint32_t n_req, uint32_t n_res, uint32_t nbt, uint32_t m, uint32_t shift,
                                                           const u64* __restrict__ res_len, const u64* __restrict__ block_first, const u64* __restrict__ req,
                                                           const u64* __restrict__ out_cap, ReaderTab t)
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
				else if (f1 - f0 != (L >> shift) + ((L & (B - 1u)) ? 1u : 0u)) { st = -3; }   // MSCOMP_DATA_ERROR (from here on L < 2^50: nbt < 2^31 blocks)
				else {
					o = off < L ? off : L; w = len < L - o ? len : L - o;
					if (CAP && w > out_cap[q]) { st = -5; w = 0; }                       // MSCOMP_BUF_ERROR
					else if (w) { c = ((o + w - 1u) >> shift) - (o >> shift) + 1u; j0 = f0 + (o >> shift); }
				}
			}
		}
		u64 v[1] = {c};
		dv_block_scan<1>(v, run, s_w);                                    // running total of covering blocks, this request included
		if (c && v[0] > m) { st = -2; c = 0; w = 0; }                       // over the budget: MSCOMP_ARG_ERROR, as everything with blocks behind it
		u64 k[1] = {c};
		dv_block_scan<1>(k, cnt, s_w);
		if (live) { t.unit_first[q + 1u] = k[0]; t.q_off[q] = o; t.q_want[q] = w; t.q_j0[q] = j0; t.q_len[q] = L; t.q_stat[q] = st; }
	}
}

// One thread per possible unit: its request (binary search in unit_first), its block, and a bid for the block -- the largest ~u, so the
// lowest unit that covers a block owns it whatever the order the bids arrive in. own[] was cleared to 0 (no bid) before.
__global__ __launch_bounds__(256) void rd_owner_kernel(uint32_t n_req, uint32_t m, ReaderTab t)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u >= m || u >= t.unit_first[n_req]) { return; }
	const uint32_t q = res_of_block(t.unit_first, n_req, u);
	const u64 j = t.q_j0[q] + (u - t.unit_first[q]);                       // (< block_first[r + 1] <= nbt: rd_req_kernel)
	t.uq[u] = q; t.ublk[u] = (uint32_t)j;
	atomicMax(&t.own[j], ~u);
}

// One thread per possible unit. An owner runs the container's table checks on its block (mscomp_amd_blocks_decompress, step 4): a block to
// decode becomes a unit of the inner plan with its output at cache slot u B and capacity e; a raw block's source is its place in d_packed;
// a block that fails a check is never read. Every other unit is an empty unit of the inner plan that points at its owner. The owners are
// counted: distinct blocks, and those that are decoded.
__global__ __launch_bounds__(256) void rd_units_kernel(uint32_t n_req, uint32_t m, uint32_t shift, u64 packed_len, const uint8_t* __restrict__ packed,
                                                      const uint8_t* __restrict__ cache, const u64* __restrict__ block_off, ReaderTab t)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u >= m) { return; }
	const u64 B = (u64)1 << shift;
	u64 io = 0, il = 0, oo = 0, oc = 0, sa = 0, cl = 0;
	uint32_t a = RD_SKIP, o = u;
	bool mine = false;
	if (u < t.unit_first[n_req]) {
		const uint32_t j = t.ublk[u];
		o = ~t.own[j];
		mine = o == u;
		if (mine) {
			const uint32_t q = t.uq[u];
			const u64 jb = (t.q_off[q] >> shift) + (u - t.unit_first[q]), left = t.q_len[q] - (jb << shift), e = left < B ? left : B;
			const u64 o0 = block_off[j], o1 = block_off[j + 1u];
			if (o1 < o0 || o1 > packed_len) { a = RD_FAIL; }
			else {
				const u64 s = o1 - o0;
				if (s == e) { a = RD_COPY; sa = (u64)(uintptr_t)(packed + o0); cl = e; }
				else if (s != 0 && s < e) { a = RD_DECODE; io = o0; il = s; oo = (u64)u << shift; oc = e; sa = (u64)(uintptr_t)(cache + oo); cl = e; }
				else { a = RD_FAIL; }
			}
			a |= (uint32_t)e << 2;                                          // (e <= 512 KiB)
		}
	}
	t.in_off[u] = io; t.in_len[u] = il; t.out_off[u] = oo; t.out_cap[u] = oc; t.src[u] = sa; t.clen[u] = cl; t.act[u] = a; t.owner[u] = o;
	const u64 owners = __ballot(mine), decoded = __ballot((a & 3u) == RD_DECODE);
	if ((threadIdx.x & 63u) == 0 && owners) { atomicAdd(&t.cnt[0], (uint32_t)__popcll(owners)); if (decoded) { atomicAdd(&t.cnt[1], (uint32_t)__popcll(decoded)); } }
}

// One wave per request: the verdicts of its units' owners (a failed table check; a decoder status other than MSCOMP_OK or a length other
// than e; with block_crc, a CRC-32 other than the one given) folded behind the request's own, into d_status, d_out_len and q_stat -- which
// the gather reads: no byte moves for a request that is not MSCOMP_OK.
__global__ __launch_bounds__(256) void rd_fold_kernel(uint32_t n_req, const uint32_t* __restrict__ block_crc, ReaderTab t, u64* __restrict__ d_out_len, int32_t* __restrict__ d_status)
{
	const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (q >= n_req) { return; }
	const int32_t st = t.q_stat[q];
	bool bad = false;
	if (st == 0) {
		for (u64 u = t.unit_first[q] + lane; u < t.unit_first[q + 1u]; u += 64u) {
			const uint32_t o = t.owner[u], a = t.act[o], kind = a & 3u;
			if (kind == RD_FAIL || (kind == RD_DECODE && (t.ustat[o] != 0 || t.ulen[o] != (u64)(a >> 2)))) { bad = true; }
			else if (block_crc && t.ucrc[o] != block_crc[t.ublk[o]]) { bad = true; }
		}
	}
	const bool any_bad = __ballot(bad) != 0;
	if (lane == 0) {
		const int32_t s = st != 0 ? st : any_bad ? -3 : 0;                 // MSCOMP_DATA_ERROR
		d_status[q] = s; d_out_len[q] = s == 0 ? t.q_want[q] : 0; t.q_stat[q] = s;
	}
}

// The gather. A unit of an MSCOMP_OK request moves the part of its block that the request wants from its owner's source (cache slot or
// d_packed) to its place in d_out, in pieces of 16 KiB: an item is one (unit, piece) pair, items = units of this call << ppu_shift. The items
// are dealt to the waves of a fixed grid in runs of `per` <= 64, so that few items spread over many waves and many items keep every lane of
// a wave busy reading table rows: a LANE works out the source, destination and length of one item -- the dependent table loads of 64 items
// are in flight together --, then the WAVE moves the non-empty ones one after the other. A 64-byte request so costs a wave one round trip
// to memory, not a workgroup one.
__global__ __launch_bounds__(256) void rd_gather_kernel(uint32_t n_req, uint32_t shift, uint32_t ppu_shift, uint8_t* __restrict__ out, const u64* __restrict__ out_off, ReaderTab t)
{
	const uint32_t lane = threadIdx.x & 63u;
	const u64 items = t.unit_first[n_req] << ppu_shift, nw = (u64)gridDim.x * 4u, w = (u64)blockIdx.x * 4u + (threadIdx.x >> 6);
	u64 per = (items + nw - 1u) / nw;
	per = per < 1u ? 1u : per > 64u ? 64u : per;
	for (u64 base = w * per; base < items; base += nw * per) {
		u64 sa = 0, da = 0;
		uint32_t len = 0;
		const u64 i = base + lane;
		if (lane < per && i < items) {
			const uint32_t u = (uint32_t)(i >> ppu_shift), q = t.uq[u];
			if (t.q_stat[q] == 0) {
				const u64 o = t.q_off[q], end = o + t.q_want[q], b0 = ((o >> shift) + (u - t.unit_first[q])) << shift, b1 = b0 + ((u64)1 << shift);
				const u64 lo = o > b0 ? o : b0, hi = end < b1 ? end : b1;
				const u64 p0 = lo + ((i & (((u64)1 << ppu_shift) - 1u)) << RD_PIECE_SHIFT);
				if (p0 < hi) {
					len = (uint32_t)(hi - p0 < ((u64)1 << RD_PIECE_SHIFT) ? hi - p0 : (u64)1 << RD_PIECE_SHIFT);
					sa = t.src[t.owner[u]] + (p0 - b0); da = (u64)(uintptr_t)out + out_off[q] + (p0 - o);
				}
			}
		}
		u64 todo = __ballot(len != 0);
		while (todo) {
			const int l = __ffsll((unsigned long long)todo) - 1;
			todo &= todo - 1u;
			const u64 s = __shfl(sa, l, 64), d = __shfl(da, l, 64);
			const uint32_t c = __shfl(len, l, 64);
			rd_wave_move(reinterpret_cast<uint8_t*>((uintptr_t)d), reinterpret_cast<const uint8_t*>((uintptr_t)s), c, lane);
		}
	}
}

void launch_reader_requests(hipStream_t st, uint32_t n_req, uint32_t n_res, uint32_t nbt, uint32_t m, uint32_t shift, const u64* res_len,
                            const u64* block_first, const u64* req, const u64* out_cap, const ReaderTab& t)
{
	if (out_cap) { hipLaunchKernelGGL(rd_req_kernel<true>, dim3(1), dim3(DV_THREADS), 0, st, n_req, n_res, nbt, m, shift, res_len, block_first, req, out_cap, t); }
	else { hipLaunchKernelGGL(rd_req_kernel<false>, dim3(1), dim3(DV_THREADS), 0, st, n_req, n_res, nbt, m, shift, res_len, block_first, req, out_cap, t); }
}

void launch_reader_units(hipStream_t st, uint32_t n_req, uint32_t nbt, uint32_t m, uint32_t shift, u64 packed_len, const uint8_t* packed,
                         const uint8_t* cache, const u64* block_off, const ReaderTab& t)
{
	if (m == 0) { return; }
	launch_dev_zero(st, t.own, nbt);
	hipLaunchKernelGGL(rd_owner_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, n_req, m, t);
	hipLaunchKernelGGL(rd_units_kernel, dim3((m + 255u) / 256u), dim3(256), 0, st, n_req, m, shift, packed_len, packed, cache, block_off, t);
}

void launch_reader_fold(hipStream_t st, uint32_t n_req, const uint32_t* block_crc, const ReaderTab& t, u64* d_out_len, int32_t* d_status)
{
	hipLaunchKernelGGL(rd_fold_kernel, dim3((n_req + 3u) / 4u), dim3(256), 0, st, n_req, block_crc, t, d_out_len, d_status);
}

void launch_reader_gather(hipStream_t st, uint32_t n_req, uint32_t m, uint32_t shift, uint8_t* out, const u64* out_off, const ReaderTab& t, uint32_t blocks)
{
	if (m == 0) { return; }
	const uint32_t ppu_shift = shift > RD_PIECE_SHIFT ? shift - RD_PIECE_SHIFT : 0u;
	const u64 need = (((u64)m << ppu_shift) + 255u) / 256u;                // a lane per item at the bound
	hipLaunchKernelGGL(rd_gather_kernel, dim3((uint32_t)(need < blocks ? need : blocks)), dim3(256), 0, st, n_req, shift, ppu_shift, out, out_off, t);
}

} // namespace msc
