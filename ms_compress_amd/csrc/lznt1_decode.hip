// lznt1_decode.hip -- gfx950 LZNT1 decompressor, batch form: n independent units resident in HBM.
//
//   lzd_seg_kernel -> lzd_verify_kernel -> scan -> lzd_chunk_kernel<false> -> lzd_finalize_kernel -> lzd_chunk_kernel<true>
//   (chunk-parallel; the header chain and the output offsets are speculated and verified)
// Size query (mscomp_amd_plan_create_size): the same walk with every test and without the byte stage -- lzd_chunk_kernel<false, true> (token phase only).
// Per unit, status and length are what the reference's one-shot call returns (MSCOMP_OK / MSCOMP_BUF_ERROR / MSCOMP_DATA_ERROR); the
// oracle restates those semantics (oracle/mscomp_oracle.c) and tests/test_gpu_decompress.py compares both with the compiled reference.
//
// LZNT1 follows the one-shot semantics of the reference, which is its streaming inflate driven once over the whole
// buffer (/root/reference/src/lznt1_decompress.cpp:122-290 through ALL_AT_ONCE_WRAPPER_DECOMPRESS,
// /root/reference/include/mscomp/internal.h:616-630):
//   * chunk headers are walked while output room AND >= 2 input bytes remain (:252-259); header 0 ends the stream and is
//     DATA_ERROR unless it is the last two bytes (:128-134); a chunk longer than the remaining input is kept as partial
//     state, so the one-shot call ends in BUF_ERROR (:136-143, wrapper :627); the signature is checked after that (:151);
//   * every compressed chunk is decoded against a 4096-byte limit (:158,:179), any chunk error becomes DATA_ERROR;
//   * a chunk may decode to fewer than 4096 bytes anywhere in the stream - the next chunk continues right behind it;
//   * output that does not fit (or input left when the output is full) gives BUF_ERROR; a single trailing byte is accepted
//     when it is 0 (:223-227).
// The chunks of a unit are independent once their headers are known, but the headers form a chain (each gives the distance
// to the next). The chain is walked in parallel, speculatively: (1) the compressed input of a unit is cut into segments of
// LZD_SEG bytes; the block of segment s tries every offset of the 4098 bytes that start LZD_HEAD bytes before the segment
// as a header and follows it: wrong guesses die at the first header without the 011 signature (7 of 8 random words), the
// ones that live until the segment begins all arrive at the same header - the landing L_s - which is then followed through
// the segment to the first header of the next one, E_s. (2) One wave per unit checks E_s == L_(s+1) for all s (segment 0
// starts at offset 0, so by induction every chain is the true one), walks the segments again where that fails, and
// counts. (3) One wave per chunk decodes in LDS and writes the chunk where it lands if every earlier chunk holds 4096
// bytes, (4) one wave per unit adds the sizes up, decides the status and notices units with short chunks in the middle,
// (5) whose chunks are decoded again to their exact places.
#include "kernels.h"

namespace msc {

// ===================================================================================================================
// (1) header chain, speculative per segment
// ===================================================================================================================
#define LZD_THREADS 1024u
#define LZD_WINDOW (LZD_HEAD + LZD_SEG + 16u)                      // candidate region + segment + the header that ends it
#define LZD_LDS (LZD_WINDOW + 48u)
#define LZD_NONE  0xFFFFFFFFu                                      // no (unique) landing
#define LZD_ENDED 0xFFFFFFFEu                                      // the chain ended (end of input or a stop) before the segment / inside it
enum { LZD_EOI0 = 0, LZD_EOI1 = 1, LZD_ZERO_OK = 2, LZD_ZERO_BAD = 3, LZD_TRUNC = 4, LZD_BADSIG = 5 };

// One step of the walk of :122-153 at offset pos of a unit of n bytes whose bytes are read through rd(pos):
// returns 0 and advances pos, or 1 + the reason the walk ends here.
template <typename RD>
__device__ __forceinline__ uint32_t lzd_step(uint32_t& pos, uint32_t n, RD rd, uint32_t& last)
{
	if (pos + 2u > n) { if (pos < n) { last = rd(pos); return 1u + LZD_EOI1; } return 1u + LZD_EOI0; }
	const uint32_t hdr = rd(pos) | (rd(pos + 1u) << 8);
	if (hdr == 0) { return 1u + (n - pos == 2u ? LZD_ZERO_OK : LZD_ZERO_BAD); }      // :128-134
	const uint32_t sz = (hdr & 0xFFFu) + 3u;
	if (sz > n - pos) { return 1u + LZD_TRUNC; }                                     // :136-143
	if ((hdr & 0x7000u) != 0x3000u) { return 1u + LZD_BADSIG; }                      // :151
	pos += sz;
	return 0;
}

// per segment g and chain k < LZD_K: segL (landing), segE (first header of the next segment, or LZD_ENDED), segcnt (headers inside the segment),
// segstop (what ended the chain | last byte << 8), segoff (where its header offsets start in cin[g * LZD_SLOTS ...]; LZD_NONE: not recorded)
// DEV (plans whose tables are built on the device, mscomp_amd_plan_create_decompress_dev): the grid is sized for the plan's bound, and the blocks
// past the batch's real segment count (chunk_prefix[n_units], written by the table pass) return at once.
template <bool DEV = false>
__global__ __launch_bounds__(LZD_THREADS) void lzd_seg_kernel(const uint8_t* __restrict__ d_in, BatchTables bt, uint32_t* __restrict__ cin,
                                                            uint32_t* __restrict__ segL, uint32_t* __restrict__ segE,
                                                            uint32_t* __restrict__ segcnt, uint32_t* __restrict__ segstop, uint32_t* __restrict__ segoff)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t s_win[];
	__shared__ uint32_t s_min, s_land[LZD_K], s_cnt[LZD_K];
	const uint32_t tid = threadIdx.x, g = blockIdx.x;
	if (DEV && g >= bt.chunk_prefix[bt.n_units]) { return; }
	const uint32_t u = unit_of_chunk(bt.chunk_prefix, bt.n_units, g), s = g - bt.chunk_prefix[u];
	const uint32_t n = (uint32_t)bt.in_len[u];
	const uint8_t* base = d_in + bt.in_off[u];
	const uint32_t seg0 = s * LZD_SEG, seg1 = seg0 + LZD_SEG;           // the segment owns the headers in [seg0, seg1)
	const uint32_t w0 = s ? seg0 - LZD_HEAD : 0u;
	const uint32_t wend = n < seg1 + 2u ? n : seg1 + 2u;
	const uint32_t a0 = (uint32_t)((uintptr_t)(base + w0) & 15u);
	const uint8_t* ab = base + w0 - a0;
	const uint32_t nw = wend > w0 ? (a0 + (wend - w0) + 15u) >> 4 : 0u;
	for (uint32_t i = tid; i < nw; i += LZD_THREADS) { *reinterpret_cast<uint4*>(s_win + i * 16u) = *reinterpret_cast<const uint4*>(ab + (size_t)i * 16u); }
	if (tid < LZD_K) { s_land[tid] = LZD_NONE; s_cnt[tid] = 0; }
	if (tid == 0) { s_min = LZD_NONE; }
	__syncthreads();
	const uint8_t* wb = s_win + a0 - w0;                                // wb[pos] = byte at unit offset pos
	auto rd = [&](uint32_t p) -> uint32_t { return wb[p]; };
	if (s) {
		// every offset of the candidate region followed to the segment: where does it land (LZD_NONE: it died)
		uint32_t land[5];
		#pragma unroll
		for (int q = 0; q < 5; ++q) {
			const uint32_t c = (uint32_t)q * LZD_THREADS + tid;
			uint32_t pos = w0 + c, last = 0;
			land[q] = LZD_NONE;
			if (c < 4098u && pos <= n) {
				for (;;) {
					if (pos >= seg0) { land[q] = pos; break; }
					const uint32_t r = lzd_step(pos, n, rd, last);
					if (r) { break; }                                    // an end before the segment: nothing of this chain is ours
				}
			}
		}
		// the LZD_K smallest distinct landings
		uint32_t prev = 0; bool first = true;
		for (uint32_t k = 0; k < LZD_K; ++k) {
			#pragma unroll
			for (int q = 0; q < 5; ++q) { if (land[q] != LZD_NONE && (first || land[q] > prev)) { atomicMin(&s_min, land[q]); } }
			__syncthreads();
			const uint32_t m = s_min;
			__syncthreads();
			if (m == LZD_NONE) { break; }
			if (tid == 0) { s_land[k] = m; s_min = LZD_NONE; }
			prev = m; first = false;
			__syncthreads();
		}
		// more than LZD_K different landings: remember nothing (the verify kernel walks such a segment itself)
		bool more = false;
		#pragma unroll
		for (int q = 0; q < 5; ++q) { more |= land[q] != LZD_NONE && !first && land[q] > prev; }
		if (__syncthreads_or(more ? 1 : 0)) { if (tid < LZD_K) { s_land[tid] = LZD_NONE; } }
		__syncthreads();
	} else if (tid == 0) { s_land[0] = 0; }
	__syncthreads();
	// wave k follows chain k through the segment: first to count, then (offsets known) to record
	const uint32_t k = tid >> 6;
	uint32_t L = LZD_NONE, E = LZD_ENDED, count = 0, stopk = 0;
	if (k < LZD_K && (tid & 63u) == 0) {
		L = s_land[k];
		if (L != LZD_NONE) {
			uint32_t pos = L, last = 0;
			for (;;) {
				if (pos >= seg1) { E = pos; break; }
				const uint32_t r = lzd_step(pos, n, rd, last);
				if (r) { stopk = (r - 1u) | (last << 8); break; }
				++count;
			}
			s_cnt[k] = count;
		}
	}
	__syncthreads();
	if (k < LZD_K && (tid & 63u) == 0) {
		uint32_t off = 0;
		for (uint32_t q = 0; q < k; ++q) { off += s_cnt[q]; }
		if (L == LZD_NONE || off + count > LZD_SLOTS) { off = LZD_NONE; }
		else {
			uint32_t* __restrict__ my = cin + (size_t)g * LZD_SLOTS + off;
			uint32_t pos = L, last = 0;
			for (uint32_t i = 0; i < count; ++i) { my[i] = pos; (void)lzd_step(pos, n, rd, last); }
		}
		const size_t r = (size_t)g * LZD_K + k;
		segL[r] = L; segE[r] = E; segcnt[r] = count; segstop[r] = stopk; segoff[r] = off;
	}
}

__device__ unsigned int g_lzd_walked;                                // segments the verify kernel had to walk itself (test hook)
uint32_t lzd_read_walked()
{
	unsigned int v = 0xFFFFFFFFu, z = 0;
	if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_lzd_walked), 4) != hipSuccess) { return 0xFFFFFFFFu; }
	(void)hipMemcpyToSymbol(HIP_SYMBOL(g_lzd_walked), &z, 4);
	return v;
}

// (2) per unit, one wave: thread the true chain through the segments (segment 0 starts at offset 0; the chain of segment s + 1 is
// the one that lands where the chosen chain of segment s arrives); a segment without such a chain is walked here, by one lane
// from global memory. Leaves per segment: selcnt (chunks), seloff (where their header offsets are); per unit: stop.
__global__ __launch_bounds__(64) void lzd_verify_kernel(const uint8_t* __restrict__ d_in, BatchTables bt, uint32_t* __restrict__ cin,
                                                       const uint32_t* __restrict__ segL, const uint32_t* __restrict__ segE,
                                                       const uint32_t* __restrict__ segcnt, const uint32_t* __restrict__ segstop, const uint32_t* __restrict__ segoff,
                                                       uint32_t* __restrict__ selcnt, uint32_t* __restrict__ seloff, uint32_t* __restrict__ stop)
{
	const uint32_t lane = threadIdx.x, u = blockIdx.x;
	const uint32_t g0 = bt.chunk_prefix[u], S = bt.chunk_prefix[u + 1] - g0;
	const uint32_t n = (uint32_t)bt.in_len[u];
	const uint8_t* base = d_in + bt.in_off[u];
	auto rd = [&](uint32_t p) -> uint32_t { return base[p]; };
	uint32_t pos = 0, stopk = 0, last = 0;
	bool ended = false;
	for (uint32_t s0 = 0; s0 < S; s0 += 64u) {
		// lane t holds the LZD_K chains of segment s0 + t (an unrecorded chain cannot be used), and the landings of the segment behind it
		const uint32_t sl = s0 + lane;
		uint32_t cl[LZD_K], ce[LZD_K], nl[LZD_K];
		#pragma unroll
		for (uint32_t k = 0; k < LZD_K; ++k) {
			const size_t r = (size_t)(g0 + (sl < S ? sl : S - 1u)) * LZD_K + k;
			const bool usable = sl < S && segoff[r] != LZD_NONE;
			cl[k] = usable ? segL[r] : LZD_NONE; ce[k] = usable ? segE[r] : LZD_NONE;
			nl[k] = (sl + 1u < S && segoff[r + LZD_K] != LZD_NONE) ? segL[r + LZD_K] : LZD_NONE;
		}
		uint32_t mycnt = 0, mysel = LZD_K + 1u;                          // what lane t learns about its segment (LZD_K + 1: not reached, LZD_K: walked here)
		const uint32_t tiles = S - s0 < 64u ? S - s0 : 64u;
		if (ended) { if (sl < S) { selcnt[g0 + sl] = 0; seloff[g0 + sl] = 0; } continue; }
		// ---- all 64 segments at once: chain k of a segment continues as chain map[k] of the next (0xE: the stream ends in it, 0xF: nowhere) ----
		uint32_t map = 0;
		#pragma unroll
		for (uint32_t k = 0; k < LZD_K; ++k) {
			uint32_t to = 0xFu;
			if (ce[k] == LZD_ENDED) { to = 0xEu; }
			else if (ce[k] != LZD_NONE) {
				#pragma unroll
				for (uint32_t q = LZD_K; q-- > 0;) { if (nl[q] == ce[k]) { to = q; } }
			}
			map |= to << (4u * k);
		}
		auto compose = [](uint32_t a, uint32_t b) -> uint32_t {          // chain k -> a[b[k]]
			uint32_t r = 0;
			#pragma unroll
			for (uint32_t k = 0; k < LZD_K; ++k) { const uint32_t bk = (b >> (4u * k)) & 0xFu; r |= (bk < LZD_K ? (a >> (4u * bk)) & 0xFu : bk) << (4u * k); }
			return r;
		};
		uint32_t P = map;
		#pragma unroll
		for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)P, d, 64); if ((int)lane >= d) { P = compose(P, t); } }
		uint32_t carry = 0xFu;                                           // the chain of the tile's first segment that starts at pos
		#pragma unroll
		for (uint32_t k = LZD_K; k-- > 0;) { if ((uint32_t)__builtin_amdgcn_readlane((int)cl[k], 0) == pos) { carry = k; } }
		const uint32_t Pprev = (uint32_t)__shfl_up((int)P, 1, 64);
		const uint32_t sel = carry >= LZD_K ? 0xFu : (lane == 0 ? carry : (Pprev >> (4u * carry)) & 0xFu);
		const u64 fail = __ballot(sl < S && sel == 0xFu);
		if (!fail) {
			uint32_t nxt = 0xFu, e = LZD_NONE;
			#pragma unroll
			for (uint32_t k = 0; k < LZD_K; ++k) { if (sel == k) { nxt = (map >> (4u * k)) & 0xFu; e = ce[k]; } }
			if (sl < S && sel < LZD_K) { mysel = sel; }
			const u64 endm = __ballot(sl < S && sel < LZD_K && nxt == 0xEu);   // the segment in which the stream ends
			if (endm) {
				const uint32_t le = ctz64(endm);
				stopk = segstop[(size_t)(g0 + s0 + le) * LZD_K + (uint32_t)__builtin_amdgcn_readlane((int)sel, (int)le)];
				ended = true;
			} else { pos = (uint32_t)__builtin_amdgcn_readlane((int)e, (int)(tiles - 1u)); }
		} else {
		for (uint32_t t = 0; t < tiles; ++t) {
			if (ended) { break; }
			uint32_t sel1 = LZD_K, e = LZD_NONE;
			#pragma unroll
			for (uint32_t k = 0; k < LZD_K; ++k) {
				const uint32_t lk = (uint32_t)__builtin_amdgcn_readlane((int)cl[k], (int)t), ek = (uint32_t)__builtin_amdgcn_readlane((int)ce[k], (int)t);
				if (sel1 == LZD_K && lk == pos && ek != LZD_NONE) { sel1 = k; e = ek; }
			}
			const uint32_t g = g0 + s0 + t;
			if (sel1 < LZD_K) {
				if (lane == t) { mysel = sel1; }
				if (e == LZD_ENDED) { stopk = segstop[(size_t)g * LZD_K + sel1]; ended = true; } else { pos = e; }
			} else {                                                     // no recorded chain starts here: walk the segment now
				uint32_t count = 0;
				uint32_t* __restrict__ my = cin + (size_t)g * LZD_SLOTS;
				const uint32_t seg1 = (s0 + t + 1u) * LZD_SEG;
				for (;;) {
					if (pos >= seg1) { break; }
					const uint32_t at = pos;
					const uint32_t r = lzd_step(pos, n, rd, last);
					if (r) { stopk = (r - 1u) | (last << 8); ended = true; break; }
					if (lane == 0 && count < LZD_SLOTS) { my[count] = at; }
					++count;
				}
				if (lane == t) { mycnt = count; mysel = LZD_K; }
				if (lane == 0) { atomicAdd(&g_lzd_walked, 1u); }
			}
		}
		}
		if (sl < S) {
			uint32_t myoff = 0;
			if (mysel < LZD_K) { const size_t r = (size_t)(g0 + sl) * LZD_K + mysel; mycnt = segcnt[r]; myoff = segoff[r]; }
			selcnt[g0 + sl] = mycnt; seloff[g0 + sl] = myoff;
		}
	}
	if (lane == 0) { stop[u] = stopk; }
}

// ===================================================================================================================
// (2)/(4) chunk decode: one wave per chunk
// ===================================================================================================================
#define LZD_ERR 0x8000u
struct LzdLds {
	__attribute__((aligned(16))) uint8_t in[4128];     // the chunk (header + data) at its 16-byte phase in global memory
	__attribute__((aligned(16))) uint8_t out[4096 + 64];   // literals at once; a match leaves offset - 1 in its first two bytes until its row is resolved
	u64      bm[64];                                   // token starts over the output positions
	u64      mb[64];                                   // ... those that are matches
	uint16_t gs[464];                                  // start (data offset) of every flag group
};

// size (<= 4096) or LZD_ERR. BYTES: the decoded bytes are left in L.out; without it only the token phase runs (every test of the
// chunk is made there: the byte stage cannot fail), for the size query.
template <bool BYTES = true>
__device__ __forceinline__ uint32_t lzd_decode_chunk(LzdLds& L, const uint8_t* __restrict__ src, uint32_t in_size, uint32_t lane)
{
	// ---- load: 16-byte words that hold at least one byte of the chunk ----
	const uint32_t a0 = (uint32_t)((uintptr_t)src & 15u);
	const uint8_t* ab = src - a0;
	const uint32_t nw = (a0 + in_size + 15u) >> 4;                       // <= 258
	for (uint32_t i = lane; i < nw; i += 64u) { *reinterpret_cast<uint4*>(L.in + i * 16u) = *reinterpret_cast<const uint4*>(ab + i * 16u); }
	L.bm[lane] = 0; L.mb[lane] = 0;
	__syncthreads();
	const uint8_t* d = L.in + a0 + 2u;                                  // chunk data
	const uint32_t n = in_size - 2u;                                     // 1..4096
	// ---- flag groups: p -> p + 9 + popcount(flags) ----
	// 64 positions at a time: every lane knows the step that would follow if a group started at its byte; the chain through the
	// window is then followed with readlane (at most 8 steps of 9..17 bytes), and the visited lanes record themselves.
	uint32_t G = 0;
	{
		uint32_t e = 0;                                                  // where the chain enters the window
		for (uint32_t wbase = 0; wbase < n; wbase += 64u) {
			const uint32_t J = 9u + (uint32_t)__builtin_popcount(wbase + lane < n ? (uint32_t)d[wbase + lane] : 0u);
			u64 visited = 0; uint32_t q = e;
			while (q < 64u && wbase + q < n) { visited |= 1ull << q; q += (uint32_t)__builtin_amdgcn_readlane((int)J, (int)q); }
			if ((visited >> lane) & 1ull) { L.gs[G + popc_below(visited)] = (uint16_t)(wbase + lane); }
			G += (uint32_t)__builtin_popcountll(visited);
			e = q >= 64u ? q - 64u : 0u;
		}
	}
	__syncthreads();
	// ---- tokens, 64 at a time: input position, length (the offset/length split depends on the output position), output position ----
	uint32_t base_pos = 0, sh = 12, err = 0;                             // sh: per-lane copy of the (monotone) split
	const uint32_t nb = (G + 7u) >> 3;
	for (uint32_t tb = 0; tb < nb; ++tb) {
		const uint32_t t = tb * 64u + lane, g = t >> 3, k = t & 7u;
		uint32_t ipos = 0, flags = 0;
		if (g < G) { const uint32_t gp = L.gs[g]; flags = d[gp]; ipos = gp + 1u + k + (uint32_t)__builtin_popcount(flags & ((1u << k) - 1u)); }
		const bool valid = g < G && ipos < n;
		const bool is_match = valid && ((flags >> k) & 1u);
		if (is_match && ipos + 2u > n) { err = 1; }                     // :99 (two bytes needed)
		const uint32_t raw = valid ? ((uint32_t)d[ipos] | (is_match ? (uint32_t)d[ipos + 1u] << 8 : 0u)) : 0u;
		uint32_t len, pos;
		for (;;) {
			len = valid ? (is_match ? (raw & ((1u << sh) - 1u)) + 3u : 1u) : 0u;
			pos = base_pos + wave_incl_scan_add_u32(len) - len;
			const u64 m = __ballot(is_match && sh > 4u && pos > (16u << (12u - sh)));       // :100 (the split follows the position)
			if (!m) { break; }
			const uint32_t f = ctz64(m);
			const uint32_t pf = (uint32_t)__builtin_amdgcn_readlane((int)pos, (int)f);
			uint32_t ns = (uint32_t)__builtin_amdgcn_readlane((int)sh, (int)f);
			while (ns > 4u && pf > (16u << (12u - ns))) { --ns; }
			if (lane >= f) { sh = ns; }
		}
		const uint32_t off = (raw >> sh) + 1u;
		if (valid && (is_match ? (off > pos || pos + len > 4096u) : pos >= 4096u)) { err = 1; }   // :104-105; a literal beyond the chunk is our DATA_ERROR
		if (__ballot(err)) { return LZD_ERR; }
		if (BYTES && valid) {
			L.out[pos] = (uint8_t)(is_match ? off - 1u : raw);
			atomicOr(reinterpret_cast<uint32_t*>(L.bm) + (pos >> 5), 1u << (pos & 31u));
			if (is_match) { L.out[pos + 1u] = (uint8_t)((off - 1u) >> 8); atomicOr(reinterpret_cast<uint32_t*>(L.mb) + (pos >> 5), 1u << (pos & 31u)); }
		}
		base_pos = (uint32_t)__builtin_amdgcn_readlane((int)(pos + len), 63);
		sh = (uint32_t)__builtin_amdgcn_readlane((int)sh, 63);
	}
	const uint32_t total = base_pos;
	if (!BYTES) { return total; }
	__syncthreads();
	// ---- bytes, 64 at a time: every byte finds its token and its source; sources inside the row are chased with bpermute ----
	uint32_t carry = 0, carry_off = 0; bool carry_match = false;         // the token running when a row begins
	for (uint32_t rowbase = 0; rowbase < total; rowbase += 64u) {
		const u64 word = L.bm[rowbase >> 6], mword = L.mb[rowbase >> 6];
		const uint32_t i = rowbase + lane;
		const u64 mine = word & ((2ull << lane) - 1ull);
		const uint32_t s = mine ? rowbase + 63u - (uint32_t)__builtin_clzll(mine) : carry;
		const bool mat = mine ? ((mword >> (s - rowbase)) & 1ull) != 0 : carry_match;
		const uint32_t offm1 = mine ? ((uint32_t)L.out[s] | ((uint32_t)L.out[s + 1u] << 8)) : carry_off;     // only meaningful for a match
		uint32_t ptr = i, val = L.out[i];                                 // a literal is in place already
		if (word) {
			carry = rowbase + 63u - (uint32_t)__builtin_clzll(word);
			carry_match = ((mword >> (carry - rowbase)) & 1ull) != 0;
			carry_off = (uint32_t)L.out[carry] | ((uint32_t)L.out[carry + 1u] << 8);
		}
		bool resolved = !mat || i >= total;
		if (!resolved) {
			const uint32_t off = offm1 + 1u, dd = i - s;
			uint32_t rem = dd;
			if (dd >= off) {
				const uint32_t q = (uint32_t)((float)dd * __builtin_amdgcn_rcpf((float)off));
				int32_t rr = (int32_t)dd - (int32_t)(q * off);
				if (rr < 0) { rr += (int32_t)off; } else if (rr >= (int32_t)off) { rr -= (int32_t)off; }
				rem = (uint32_t)rr;
			}
			ptr = s - off + rem;
			if (ptr < rowbase) { val = L.out[ptr]; resolved = true; }
		}
		while (__ballot(!resolved)) {
			const uint32_t tl = resolved ? lane : ptr - rowbase;
			const uint32_t tv = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(tl << 2), (int)(val | (resolved ? 0x100u : 0u)));
			const uint32_t tp = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(tl << 2), (int)ptr);
			if (!resolved) { if (tv & 0x100u) { val = tv & 0xFFu; resolved = true; } else { ptr = tp; if (ptr < rowbase) { val = L.out[ptr]; resolved = true; } } }
		}
		L.out[i] = (uint8_t)val;
		__syncthreads();
	}
	return total;
}

// EXACT = false: every chunk, written where it lands if all earlier chunks hold 4096 bytes; records the size.
// EXACT = true: only units flagged irregular; chunks whose place differs are decoded again to the exact place.
// SIZE (with EXACT = false): every chunk is only sized -- the token phase of a compressed chunk, the header of a stored one -- and nothing is written
// but csize.
// Chunks are numbered through the batch in stream order (flat[g] = number of the first chunk of segment g).
template <bool EXACT, bool SIZE = false>
__global__ __launch_bounds__(64) void lzd_chunk_kernel(const uint8_t* __restrict__ d_in, BatchTables bt, const uint32_t* __restrict__ cin,
                                                      const uint32_t* __restrict__ seloff, const u64* __restrict__ flat, uint16_t* __restrict__ csize,
                                                      const uint32_t* __restrict__ irregular, uint8_t* __restrict__ d_out)
{
	__shared__ LzdLds L;
	const uint32_t lane = threadIdx.x;
	const u64 total_chunks = flat[bt.n_chunks];
	if (EXACT && irregular[bt.n_units] == 0) { return; }
	for (u64 c = blockIdx.x; c < total_chunks; c += gridDim.x) {
		const uint32_t g = seg_of_flat(flat, bt.n_chunks, c);
		const uint32_t u = unit_of_chunk(bt.chunk_prefix, bt.n_units, g);
		if (EXACT && !irregular[u]) { continue; }
		const u64 ufirst = flat[bt.chunk_prefix[u]];
		const u64 j = c - ufirst;
		const size_t slot = (size_t)g * LZD_SLOTS + seloff[g] + (size_t)(c - flat[g]);
		u64 pos = j * 4096u;
		if (EXACT) {
			u64 acc = 0;                                                 // sum of the sizes of the chunks before this one
			for (u64 i = lane; i < j; i += 64u) { acc += csize[ufirst + i] & 0x1FFFu; }
			for (int o = 32; o; o >>= 1) { acc += __shfl_xor(acc, o, 64); }
			if (acc == pos) { continue; }
			pos = acc;
		}
		const uint8_t* src = d_in + bt.in_off[u] + cin[slot];
		const uint32_t hdr = (uint32_t)src[0] | ((uint32_t)src[1] << 8);
		const uint32_t in_size = (hdr & 0xFFFu) + 3u;
		uint32_t size;
		if (hdr & 0x8000u) {
			size = lzd_decode_chunk<!SIZE>(L, src, in_size, lane);
		} else {                                                         // stored chunk (:192-209)
			size = in_size - 2u;
			for (uint32_t i = lane; !SIZE && i < size; i += 64u) { L.out[i] = src[2u + i]; }
			__syncthreads();
		}
		if (!EXACT && lane == 0) { csize[c] = (uint16_t)size; }
		const u64 cap = bt.out_cap[u];
		if (!SIZE && size != LZD_ERR && pos < cap) {
			const u64 room = cap - pos;
			lzd_store(d_out + bt.out_off[u] + pos, L.out, room < size ? (uint32_t)room : size, lane);
		}
		__syncthreads();
	}
}

// ===================================================================================================================
// (3) per unit: positions, status, out_len
// ===================================================================================================================
// d_need (size query, else null): the smallest capacity at which the unit decodes, on MSCOMP_OK -- one more than its length when the walk
// ended at the End_of_buffer header 00 00, which is only read while output room is left (:252)
__global__ __launch_bounds__(256) void lzd_finalize_kernel(BatchTables bt, const u64* __restrict__ flat, const uint32_t* __restrict__ stop,
                                                          const uint16_t* __restrict__ csize, uint32_t* __restrict__ irregular,
                                                          u64* __restrict__ d_out_len, int32_t* __restrict__ d_status, u64* __restrict__ d_need)
{
	__shared__ uint32_t s_wsum[4], s_wev[4], s_wirr[4];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, u = blockIdx.x;
	const u64 ufirst = flat[bt.chunk_prefix[u]], count = flat[bt.chunk_prefix[u + 1]] - ufirst;
	const uint32_t kind = stop[u] & 0xFFu, last = stop[u] >> 8;
	const u64 cap = bt.out_cap[u];
	const uint16_t* __restrict__ sz = csize + ufirst;
	u64 pos = 0; int32_t status = 1; bool irr = false;                   // status 1 = undecided
	for (u64 j0 = 0; j0 < count; j0 += 1024u) {                          // thread t: chunks j0 + 4t .. j0 + 4t + 3
		uint32_t raw[4], size[4], mine = 0;
		#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const u64 j = j0 + tid * 4u + q;
			raw[q] = j < count ? sz[j] : 0u;
			size[q] = raw[q] == LZD_ERR ? 0u : raw[q];
			mine += size[q];
			irr |= j + 1u < count && raw[q] != 4096u;
		}
		const uint32_t incl = wave_incl_scan_add_u32(mine);
		if (lane == 63u) { s_wsum[w] = incl; }
		__syncthreads();
		uint32_t before = incl - mine, total = 0;
		#pragma unroll
		for (uint32_t q = 0; q < 4u; ++q) { if (q < w) { before += s_wsum[q]; } total += s_wsum[q]; }
		// the walk of :252-259 at chunk j: no room left -> the caller sees BUF_ERROR; chunk error -> DATA_ERROR; chunk does not fit -> BUF_ERROR
		u64 p = pos + before; uint32_t ev = 0;
		#pragma unroll
		for (int q = 0; q < 4; ++q) {
			const u64 j = j0 + tid * 4u + q;
			if (!ev && j < count) { ev = p >= cap ? 5u : raw[q] == LZD_ERR ? 3u : p + size[q] > cap ? 5u : 0u; }
			p += size[q];
		}
		const u64 m = __ballot(ev != 0);
		if (lane == 0) { s_wev[w] = m ? (uint32_t)__builtin_amdgcn_readlane((int)ev, (int)ctz64(m)) : 0u; }
		__syncthreads();
		uint32_t first = 0;
		#pragma unroll
		for (uint32_t q = 0; q < 4u; ++q) { if (!first) { first = s_wev[q]; } }
		__syncthreads();
		if (first) { status = -(int32_t)first; break; }
		pos += total;
	}
	const u64 mi = __ballot(irr);
	if (lane == 0) { s_wirr[w] = mi != 0; }
	__syncthreads();
	if (status == 1) {
		const bool room = pos < cap;
		switch (kind) {
		case LZD_EOI0:     status = 0; break;
		case LZD_EOI1:     status = last == 0 ? 0 : -5; break;                       // :223-227
		case LZD_ZERO_OK:  status = room ? 0 : -5; break;                            // the header is only read while there is room (:252)
		case LZD_ZERO_BAD: status = room ? -3 : -5; break;
		case LZD_TRUNC:    status = -5; break;
		default:           status = room ? -3 : -5; break;                           // LZD_BADSIG
		}
	}
	if (tid == 0) {
		const bool any = s_wirr[0] | s_wirr[1] | s_wirr[2] | s_wirr[3];
		d_status[u] = status; d_out_len[u] = status == 0 ? pos : 0;
		if (d_need) { d_need[u] = status == 0 ? pos + (kind == LZD_ZERO_OK ? 1u : 0u) : 0; }
		irregular[u] = any ? 1u : 0u;
		if (any) { atomicOr(&irregular[bt.n_units], 1u); }
	}
}

__global__ void lzd_clear_kernel(uint32_t* p) { *p = 0; }

void prepare_lzd_segments(bool dev)
{
	static PerDeviceOnce attr, attr_dev;
	if (!dev && attr.needed()) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lzd_seg_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LZD_LDS); attr.done(); }
	if (dev && attr_dev.needed()) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(lzd_seg_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LZD_LDS); attr_dev.done(); }
}
void launch_lzd_segments(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const LzdBufs& b, bool dev)
{
	if (bt.n_units == 0) { return; }
	prepare_lzd_segments(dev);
	hipLaunchKernelGGL(lzd_clear_kernel, dim3(1), dim3(1), 0, st, b.irregular + bt.n_units);
	if (dev) { hipLaunchKernelGGL(lzd_seg_kernel<true>, dim3(bt.n_chunks), dim3(LZD_THREADS), LZD_LDS, st, d_in, bt, b.cin, b.segL, b.segE, b.segcnt, b.segstop, b.segoff); }
	else { hipLaunchKernelGGL(lzd_seg_kernel<false>, dim3(bt.n_chunks), dim3(LZD_THREADS), LZD_LDS, st, d_in, bt, b.cin, b.segL, b.segE, b.segcnt, b.segstop, b.segoff); }
}
void launch_lzd_verify(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const LzdBufs& b)
{
	if (bt.n_units == 0) { return; }
	hipLaunchKernelGGL(lzd_verify_kernel, dim3(bt.n_units), dim3(64), 0, st, d_in, bt, b.cin, b.segL, b.segE, b.segcnt, b.segstop, b.segoff, b.selcnt, b.seloff, b.stop);
}
// every chunk decoded (EXACT = false), the irregular units' chunks again to their places (EXACT), or every chunk only sized (SIZE; no d_out)
template <bool EXACT, bool SIZE>
static void lzd_chunks(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const LzdBufs& b, uint8_t* d_out)
{
	if (bt.n_units == 0) { return; }
	const u64 est = (u64)bt.n_chunks * (LZD_SEG / 2048u);            // the count lives on the device; typical chunks are 2-4 KiB
	const uint32_t grid = est < 16384u ? (uint32_t)est : 16384u;
	hipLaunchKernelGGL((lzd_chunk_kernel<EXACT, SIZE>), dim3(grid), dim3(64), 0, st, d_in, bt, b.cin, b.seloff, b.flat, b.csize, b.irregular, d_out);
}
void launch_lzd_chunks(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const LzdBufs& b, uint8_t* d_out) { lzd_chunks<false, false>(st, d_in, bt, b, d_out); }
void launch_lzd_replace(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const LzdBufs& b, uint8_t* d_out) { lzd_chunks<true, false>(st, d_in, bt, b, d_out); }
void launch_lzd_sizes(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const LzdBufs& b) { lzd_chunks<false, true>(st, d_in, bt, b, nullptr); }
void launch_lzd_finalize(hipStream_t st, const BatchTables& bt, const LzdBufs& b, u64* d_out_len, int32_t* d_status, u64* d_need)
{
	if (bt.n_units == 0) { return; }
	hipLaunchKernelGGL(lzd_finalize_kernel, dim3(bt.n_units), dim3(256), 0, st, bt, b.flat, b.stop, b.csize, b.irregular, d_out_len, d_status, d_need);
}

} // namespace msc
