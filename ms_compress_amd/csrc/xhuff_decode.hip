// xhuff_decode.hip -- gfx950 Xpress+Huffman decompressor, batch form: n independent units resident in HBM.
//   xhc_mark_kernel -> xhc_parse_kernel<1> -> xhc_chain_kernel -> xhc_parse_kernel<2>: the chunks of a buffer found speculatively and
//                         walked in parallel, one wave per chunk, writing 32-bit tokens                           [comments at the kernels]
//   xhd_parse_kernel      the serial walk of a whole buffer, for what the speculation cannot do
//   the bytes follow from the tokens (lz_copy.hip, lzglobal.hip)
// Size query (mscomp_amd_plan_create_size): the same walks with every test, no byte stage or token store -- xhc_parse_kernel<3> / xhd_parse_kernel<false>.
// Status and length per unit are those of the reference's one-shot call (lznt1_decode.hip says how that is checked).
#include "kernels.h"

namespace msc {

// xpress_huff_decompress (/root/reference/src/xpress_huff_decompress.cpp:130-162, chunk loop :39-129; InputBitstream Bitstream.h:34-106;
// HuffmanDecoder<15,512> HuffmanDecoder.h:28-114). Where a chunk's 256-byte table starts is only known when the chunk before it
// has been decoded (no sizes are stored), and inside a chunk every symbol starts where the previous one ends, so the SYMBOLS of
// a buffer are walked by one wave, buffers in parallel (xhd_parse_kernel). The wave builds the decoding tables of a chunk
// together (counts and canonical ranks by ballots), then all lanes walk the symbols; codes of up to 9 bits resolve with one LDS
// read (symbol << 4 | length). The walk needs the output only as a running length, so it writes 32-bit tokens (a literal, or
// offset | length << 16; a match longer than 32766 is cut into matches with the same offset, which copy the same bytes) and
// keeps 4.1 KiB of LDS: 32 buffers per CU instead of the 2 that a 64 KiB output window allows. The bytes are produced afterwards
// by lz_copy_kernel, in parallel.
#define XHD_INB  1024u                 // input ring: two blocks of this size (the walk looks at most 320 bytes ahead); 4.1 KiB of LDS per wave -> 32 waves per CU
struct XhdLds {
	__attribute__((aligned(16))) uint8_t in[2u * XHD_INB];
	uint16_t fast[512];                 // 9-bit prefix -> symbol << 4 | length (0: longer code)
	uint16_t syms[512];                 // symbols in canonical order
	uint32_t lims[16], poss[16];
};

// tokens of unit u: tok[tok_prefix[u] ...], ntok[u]; d_out_len / d_status as the caller sees them (the bytes follow in lz_copy_kernel).
// EMIT = false: the size query -- tokens only counted (tok / tok_prefix unused)
template <bool EMIT = true>
__global__ __launch_bounds__(64) void xhd_parse_kernel(const uint8_t* __restrict__ d_in, BatchTables bt, const u64* __restrict__ tok_prefix,
                                                      uint32_t* __restrict__ tok, u64* __restrict__ ntok,
                                                      u64* __restrict__ d_out_len, int32_t* __restrict__ d_status, const uint32_t* __restrict__ mode)
{
	__shared__ XhdLds S;
	const uint32_t lane = threadIdx.x, u = blockIdx.x;
	if (mode[u] != XHC_SERIAL) { return; }                               // the chunk-parallel path has done this buffer
	const uint32_t n = (uint32_t)bt.in_len[u];
	const u64 cap = bt.out_cap[u];
	const uint8_t* src = d_in + bt.in_off[u];
	uint32_t* __restrict__ mytok = EMIT ? tok + tok_prefix[u] : nullptr;
	u64 nt = 0; uint32_t ns = 0, treg = 0;                               // tokens in HBM; tokens staged: token k of the batch waits in lane k
	#define XHD_EMIT(w) { if (EMIT) { treg = lane == ns ? (w) : treg; } ++ns; if (ns == 64u) { if (EMIT) { mytok[nt + lane] = treg; } nt += 64u; ns = 0; } }
	int32_t status = 1; u64 op = 0;                                      // 1 = running
	// ---- input ring (see xpd_kernel) ----
	const uint32_t a0 = (uint32_t)((uintptr_t)src & 15u);
	const uint8_t* ab = src - a0;
	const uint32_t endq = a0 + n;                                        // units are below 4 GiB - 4096
	uint32_t loaded = 0;                                                 // blocks of XHD_INB input bytes brought to LDS so far (the last two are resident)
	// a block is loaded when the walk gets there (one HBM round trip per KiB of input: nothing next to ~2500 symbols); values that
	// live across the walk in registers (a prefetched block) made the compiler wait for memory and shuffle them on every symbol
	#define XHD_BLOCK() { uint8_t* b_ = S.in + (loaded & 1u) * XHD_INB; __syncthreads(); \
		_Pragma("unroll") for (int i_ = 0; i_ < (int)(XHD_INB / 1024u); ++i_) { const u64 q_ = (u64)loaded * XHD_INB + ((uint32_t)i_ * 64u + lane) * 16u; \
			*reinterpret_cast<uint4*>(b_ + ((uint32_t)i_ * 64u + lane) * 16u) = q_ < endq ? *reinterpret_cast<const uint4*>(ab + q_) : make_uint4(0, 0, 0, 0); } \
		++loaded; __syncthreads(); }
	// loaded * XHD_INB never lies behind the walk, so the distance to it is a plain 32-bit difference (units end below 4 GiB - 4096)
	#define XHD_NEED(q, margin) while (loaded * XHD_INB - (q) < (margin) && loaded * XHD_INB < endq) { XHD_BLOCK() }
	XHD_BLOCK() XHD_BLOCK()
	auto rb = [&](uint32_t q) -> uint32_t { return S.in[q & (2u * XHD_INB - 1u)]; };
	uint32_t ip = a0;
	while (status == 1) {
		// ---- a chunk: 256 bytes of code lengths, then its bit stream (:137-152) ----
		if (endq - ip < 260u) { status = (ip != endq) ? -3 : 0; break; } // :140-144
		XHD_NEED(ip, 320u)
		uint32_t cl[8];
		{
			const uint32_t w = rb(ip + 4u * lane) | (rb(ip + 4u * lane + 1u) << 8) | (rb(ip + 4u * lane + 2u) << 16) | (rb(ip + 4u * lane + 3u) << 24);
			#pragma unroll
			for (int k = 0; k < 8; ++k) { cl[k] = (w >> (4 * k)) & 0xFu; }   // symbols 8 lane .. 8 lane + 7
		}
		ip += 256u;
		__syncthreads();
		// SetCodeLengths (HuffmanDecoder.h:42-90): counts, limits, positions, canonical order
		uint32_t last = 0, pos_acc = 0, prevcnt = 0; bool bad = false;
		for (uint32_t i = lane; i < 512u; i += 64u) { S.syms[i] = 0xFFFFu; }
		if (lane == 0) { S.lims[0] = 0; S.poss[0] = 0; }
		for (uint32_t L = 1; L <= 15u; ++L) {
			u64 m[8]; uint32_t cnt = 0, before = 0;
			#pragma unroll
			for (int k = 0; k < 8; ++k) { m[k] = __ballot(cl[k] == L); cnt += (uint32_t)__builtin_popcountll(m[k]); before += popc_below(m[k]); }
			pos_acc += prevcnt; prevcnt = cnt;                           // poss[L] = poss[L-1] + cnts[L-1], cnts[0] = 0
			if (L < 15u) { const uint32_t inc = cnt << (15u - L); if (last + inc > 32768u) { bad = true; } last += inc; }
			else if (last + cnt > 32768u) { bad = true; }
			if (lane == 0) { S.lims[L] = L < 15u ? last : 32768u; S.poss[L] = pos_acc; }
			uint32_t mine = 0;
			#pragma unroll
			for (int k = 0; k < 8; ++k) { if (cl[k] == L) { const uint32_t at = pos_acc + before + mine; if (at < 512u) { S.syms[at] = (uint16_t)(lane * 8u + k); } ++mine; } }
		}
		if (bad) { status = -3; break; }                                 // :149
		__syncthreads();
		const uint32_t lims9 = S.lims[9];
		for (uint32_t i = lane; i < 512u; i += 64u) {
			uint32_t e = 0;
			const uint32_t x = i << 6;
			if (x < lims9) {
				uint32_t L = 1;
				while (x >= S.lims[L]) { ++L; }
				const uint32_t sidx = S.poss[L] + ((x - S.lims[L - 1u]) >> (15u - L));
				const uint32_t sym = sidx < 512u ? S.syms[sidx] : 0xFFFFu;
				e = sym == 0xFFFFu ? 0u : ((sym << 4) | L);
			}
			S.fast[i] = (uint16_t)e;
		}
		__syncthreads();
		// ---- the chunk's symbols (:87-127) ----
		XHD_NEED(ip, 320u)
		uint32_t mask = (rb(ip) << 16) | (rb(ip + 1) << 24) | rb(ip + 2) | (rb(ip + 3) << 8);   // Bitstream.h:44
		uint32_t bits = 32; ip += 4u;
		uint32_t prod = 0;                                               // bytes of this chunk so far, saturating
		bool stream_end = false;
		#define XHD_SKIP(k) { mask <<= (k); bits -= (k); if (bits < 16u && ip + 2u <= endq) { XHD_NEED(ip, 2u) mask |= (rb(ip) | (rb(ip + 1) << 8)) << (16u - bits); bits |= 16u; ip += 2u; } }
		#define XHD_MASK_ZERO() (bits == 0 || (mask >> (32u - bits)) == 0)
		#define XHD_DECODE(sym) { const uint32_t r_ = bits; const uint32_t x_ = r_ < 15u ? (((mask >> 16) >> (16u - r_)) << (15u - r_)) : (mask >> 17); \
			const uint32_t f_ = S.fast[x_ >> 6]; uint32_t n_; \
			if (f_) { n_ = f_ & 0xFu; sym = f_ >> 4; if (n_ > r_) { sym = 0xFFFFu; } else { XHD_SKIP(n_) } } \
			else { n_ = x_ >= lims9 ? 10u : 1u; while (x_ >= S.lims[n_]) { ++n_; } \
				if (n_ > r_) { sym = 0xFFFFu; } else { XHD_SKIP(n_) const uint32_t s_ = S.poss[n_] + ((x_ - S.lims[n_ - 1u]) >> (15u - n_)); sym = s_ >= 512u ? 0xFFFFu : S.syms[s_]; } } }
		while (prod < 65536u || !XHD_MASK_ZERO()) {
			uint32_t sym;
			XHD_DECODE(sym)
			if (sym < 0x100u) {
				if (op == cap) { status = -5; break; }
				XHD_EMIT(0x80000000u | sym)
				++op; ++prod;
			} else {
				if (sym == 0xFFFFu) { status = -3; break; }
				if (sym == 0x100u && ip == endq && XHD_MASK_ZERO()) { stream_end = true; break; }   // :91
				uint32_t len = sym & 0xFu;
				if (len == 0xFu) {
					XHD_NEED(ip, 8u)
					if (endq - ip < 1u) { status = -3; break; }
					len = rb(ip); ip += 1u;
					if (len == 0xFFu) {
						if (endq - ip < 2u) { status = -3; break; }
						len = rb(ip) | (rb(ip + 1) << 8); ip += 2u;
						if (len == 0) {
							if (endq - ip < 4u) { status = -3; break; }
							len = rb(ip) | (rb(ip + 1) << 8) | (rb(ip + 2) << 16) | (rb(ip + 3) << 24); ip += 4u;
						}
						if (len < 0xFu) { status = -3; break; }
						len -= 0xFu;
					}
					len += 0xFu;
				}
				len += 3u;
				const uint32_t ob = (sym >> 4) & 0xFu;
				if (ob > bits) { status = -3; break; }                   // :117
				const uint32_t off = ((mask >> 16) >> (16u - ob)) + (1u << ob);
				XHD_SKIP(ob)
				if (off > op) { status = -3; break; }                    // :120
				if (len > cap - op) { status = -5; break; }              // :121
				op += len; prod = prod + len < prod ? 0xFFFFFFFFu : prod + len;
				while (len > LZT_MAXLEN) { XHD_EMIT(off | (LZT_MAXLEN << 16)) len -= LZT_MAXLEN; }
				XHD_EMIT(off | (len << 16))
			}
		}
		if (status != 1) { break; }
		if (!stream_end) {                                               // :128-134: is the next symbol the end of the stream?
			const uint32_t ip_keep = ip;
			uint32_t sym;
			XHD_DECODE(sym)
			if (sym == 0x100u && ip == endq && XHD_MASK_ZERO()) { stream_end = true; } else { ip = ip_keep; }
		}
		if (stream_end) { status = 0; }
	}
	#undef XHD_BLOCK
	#undef XHD_NEED
	#undef XHD_SKIP
	#undef XHD_MASK_ZERO
	#undef XHD_DECODE
	if (EMIT && lane < ns) { mytok[nt + lane] = treg; }
	#undef XHD_EMIT
	if (lane == 0) { d_status[u] = status; d_out_len[u] = status == 0 ? op : 0; ntok[u] = status == 0 ? nt + ns : 0; }
}

// ===================================================================================================================
// Xpress+Huffman: the chunks of ONE buffer in parallel (speculative chunk starts)
// ===================================================================================================================
// Where a chunk starts is not stored, but its first 256 bytes are a complete prefix code: the 512 nibbles l satisfy sum 2^(15-l) = 2^15
// (tools/xh_marker_study.py: true for every chunk of the corpus, and for 78 other offsets in 80 MB of streams). xhc_mark_kernel lists the
// offsets of a buffer with that property (plus offset 0), xhc_parse_kernel<1> walks every candidate as ONE chunk on its own, xhc_chain_kernel
// follows end(k) == start(k+1) from offset 0, places the chunks in the output and the token stream and checks that no match reaches in
// front of the buffer; xhc_parse_kernel<2> then writes the tokens of the accepted chunks. Anything unexpected (more candidates than room,
// a broken chain, an error inside a chunk, output beyond the capacity) sends the buffer to the serial walk, which reports the reference's status.
#define XHC_TILE 16384u                 // input bytes per block of xhc_mark_kernel
#define XHC_MAXC 8192u                  // candidates of a buffer the chain check can hold
// DEV: as lzd_seg_kernel<true>, the tiles past the batch's real count return at once
template <bool DEV = false>
__global__ __launch_bounds__(256) void xhc_mark_kernel(const uint8_t* __restrict__ d_in, BatchTables bt, const u64* __restrict__ cand_prefix, XhcBufs xb)
{
	__shared__ uint8_t s_b[XHC_TILE + 256u + 16u];
	__shared__ uint32_t s_k[256];
	const uint32_t tile = blockIdx.x, tid = threadIdx.x;
	if (DEV && tile >= bt.chunk_prefix[bt.n_units]) { return; }
	const uint32_t u = unit_of_chunk(bt.chunk_prefix, bt.n_units, tile), t = tile - bt.chunk_prefix[u];
	const uint32_t n = (uint32_t)bt.in_len[u];
	const uint8_t* __restrict__ src = d_in + bt.in_off[u];
	const uint32_t room = (uint32_t)(cand_prefix[u + 1] - cand_prefix[u]);
	uint32_t* __restrict__ my = xb.cand_pos + cand_prefix[u];
	const u64 T0 = (u64)t * XHC_TILE;
	if (t == 0 && tid == 0) { const uint32_t i = atomicAdd(&xb.cand_cnt[u], 1u); if (i < room) { my[i] = 0; } }   // chunk 0 starts at offset 0
	if (T0 >= n) { return; }
	const uint32_t avail = n - T0 < XHC_TILE + 255u ? (uint32_t)(n - T0) : XHC_TILE + 255u;
	for (uint32_t i = tid; i < avail; i += 256u) { s_b[i] = src[T0 + i]; }
	{ const uint32_t lo = tid & 15u, hi = tid >> 4; s_k[tid] = (lo ? 1u << (15u - lo) : 0u) + (hi ? 1u << (15u - hi) : 0u); }
	__syncthreads();
	const uint32_t base = tid * 64u;                                     // this thread: offsets T0 + base .. + 63
	uint32_t sum = 0;
	for (uint32_t i = 0; i < 64u; ++i) {
		const u64 p = T0 + base + i;
		if (p + 260u > n) { break; }                                     // a chunk is a table and at least 4 bytes (:140)
		if (i == 0) { for (uint32_t j = 0; j < 256u; ++j) { sum += s_k[s_b[base + j]]; } }
		else { sum += s_k[s_b[base + i + 255u]] - s_k[s_b[base + i - 1u]]; }
		if (sum == 32768u && p != 0) { const uint32_t k = atomicAdd(&xb.cand_cnt[u], 1u); if (k < room) { my[k] = (uint32_t)p; } }
	}
}

// ONE chunk per wave, wherever a candidate says a chunk starts (speculative: see xhc_mark_kernel / xhc_chain_kernel). PASS 1: every candidate
// is measured (where the next chunk would start, bytes produced, how far its matches reach in front of the chunk, tokens; 2 = not a chunk);
// the candidate at offset 0 is chunk 0 for sure and writes its tokens at once. PASS 2: the chunks the chain check accepted write their
// tokens at their place in the unit's token stream. PASS 3 (the size query): PASS 1 without any token written, chunk 0 included.
#ifdef XHC_PROFILE   // make EXTRA=-DXHC_PROFILE: steps / symbols per step / symbols one at a time, summed and the maximum per chunk (tools/dev/gpu_xhcprof.py)
__device__ unsigned long long g_xhc_prof[8];
extern "C" void mscomp_amd_debug_xhc_prof(unsigned long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_xhc_prof), 64); unsigned long long z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_xhc_prof), z, 64); }
#define XHC_CN(i, v) { if (lane == 0) { atomicAdd(&g_xhc_prof[i], (unsigned long long)(v)); } }
#define XHC_LOC(i) { ++xhc_loc[i]; }
#define XHC_END() { if (lane == 0) { atomicMax(&g_xhc_prof[4], (unsigned long long)xhc_loc[0]); atomicMax(&g_xhc_prof[5], (unsigned long long)xhc_loc[1]); atomicMax(&g_xhc_prof[6], (unsigned long long)(xhc_loc[0] * 3u + xhc_loc[1])); atomicAdd(&g_xhc_prof[7], 1ull); } }
#else
#define XHC_CN(i, v)
#define XHC_LOC(i)
#define XHC_END()
#endif
template <int PASS>
__global__ __launch_bounds__(64) void xhc_parse_kernel(const uint8_t* __restrict__ d_in, BatchTables bt, const u64* __restrict__ tok_prefix,
                                                      const u64* __restrict__ cand_prefix, XhcBufs xb, uint32_t* __restrict__ tok)
{
	__shared__ XhdLds S;
	const uint32_t lane = threadIdx.x, slot = blockIdx.x;
	const uint32_t u = seg_of_flat(cand_prefix, bt.n_units, slot);
	const uint32_t idx = slot - (uint32_t)cand_prefix[u];
	const uint32_t have = xb.cand_cnt[u], room = (uint32_t)(cand_prefix[u + 1] - cand_prefix[u]);
	if (idx >= (have < room ? have : room)) { return; }
	// a buffer of several chunks may have token scratch: its candidates keep their tokens there in PASS 1 (xhc_gather_kernel moves those of the
	// accepted chunks to their place), and PASS 2 is left with the chunks whose tokens did not fit (state bit 4)
	const bool has_scr = xb.scr_prefix != nullptr && xb.scr_prefix[u + 1] > xb.scr_prefix[u];
	if (PASS == 2 && (xb.mode[u] != XHC_SPEC || xb.tok_off[slot] == ~(u64)0 || xb.cand_pos[slot] == 0 || (has_scr && !(xb.res_state[slot] & 4u)))) { return; }
	const bool writing = PASS == 2 || xb.cand_pos[slot] == 0;           // (in PASS 3: walks on as chunk 0 does, without storing)
	const bool scr = PASS == 1 && !writing && has_scr;
	bool scr_ok = true;
	const uint32_t at = xb.cand_pos[slot];
	const uint32_t n = (uint32_t)bt.in_len[u];
	const uint8_t* src = d_in + bt.in_off[u];
	const u64 tok_at = PASS == 2 ? xb.tok_off[slot] : (u64)0;
	uint32_t* __restrict__ mytok = PASS == 3 ? nullptr : scr ? xb.scr_tok + (xb.scr_prefix[u] + idx) * (u64)XHC_SCR : tok + tok_prefix[u] + tok_at;
	const u64 tokcap = PASS == 3 ? 0 : scr ? (u64)XHC_SCR : tok_prefix[u + 1] - tok_prefix[u] - tok_at;   // chunk 0 writes before the capacity is judged: never beyond the unit's slots
	const bool storing = PASS != 3 && (writing || scr);
#ifdef XHC_PROFILE
	uint32_t xhc_loc[2] = {0, 0};
#endif
	u64 reach = 0;
	u64 nt = 0;                                                          // tokens so far
	#define XHD_EMIT(w) { if (storing && lane == 0 && nt < tokcap) { mytok[nt] = (w); } ++nt; }
	int32_t status = 1; u64 op = 0;                                      // 1 = running
	// ---- input ring (see xpd_kernel) ----
	const uint32_t a0 = (uint32_t)((uintptr_t)src & 15u);
	const uint8_t* ab = src - a0;
	const uint32_t endq = a0 + n;                                        // units are below 4 GiB - 4096
	uint32_t loaded = 0;                                                 // blocks of XHD_INB input bytes brought to LDS so far (the last two are resident)
	// a block is loaded when the walk gets there (one HBM round trip per KiB of input: nothing next to ~2500 symbols); values that
	// live across the walk in registers (a prefetched block) made the compiler wait for memory and shuffle them on every symbol
	#define XHD_BLOCK() { uint8_t* b_ = S.in + (loaded & 1u) * XHD_INB; __syncthreads(); \
		_Pragma("unroll") for (int i_ = 0; i_ < (int)(XHD_INB / 1024u); ++i_) { const u64 q_ = (u64)loaded * XHD_INB + ((uint32_t)i_ * 64u + lane) * 16u; \
			*reinterpret_cast<uint4*>(b_ + ((uint32_t)i_ * 64u + lane) * 16u) = q_ < endq ? *reinterpret_cast<const uint4*>(ab + q_) : make_uint4(0, 0, 0, 0); } \
		++loaded; __syncthreads(); }
	// loaded * XHD_INB never lies behind the walk, so the distance to it is a plain 32-bit difference (units end below 4 GiB - 4096)
	#define XHD_NEED(q, margin) while (loaded * XHD_INB - (q) < (margin) && loaded * XHD_INB < endq) { XHD_BLOCK() }
	loaded = (a0 + at) / XHD_INB;
	XHD_BLOCK() XHD_BLOCK()
	auto rb = [&](uint32_t q) -> uint32_t { return S.in[q & (2u * XHD_INB - 1u)]; };
	uint32_t ip = a0 + at;
	uint32_t state = 2, next_at = 0;                                      // 0 chunk done, 1 the stream ends with it, 2 not a chunk
	while (status == 1) {
		// ---- a chunk: 256 bytes of code lengths, then its bit stream (:137-152) ----
		if (endq - ip < 260u) { if (ip == endq && at == 0) { state = 1; next_at = 0; } break; }   // an empty buffer is an empty stream (:140-144)
		XHD_NEED(ip, 320u)
		uint32_t cl[8];
		{
			const uint32_t w = rb(ip + 4u * lane) | (rb(ip + 4u * lane + 1u) << 8) | (rb(ip + 4u * lane + 2u) << 16) | (rb(ip + 4u * lane + 3u) << 24);
			#pragma unroll
			for (int k = 0; k < 8; ++k) { cl[k] = (w >> (4 * k)) & 0xFu; }   // symbols 8 lane .. 8 lane + 7
		}
		ip += 256u;
		__syncthreads();
		// SetCodeLengths (HuffmanDecoder.h:42-90): counts, limits, positions, canonical order
		uint32_t last = 0, pos_acc = 0, prevcnt = 0; bool bad = false;
		for (uint32_t i = lane; i < 512u; i += 64u) { S.syms[i] = 0xFFFFu; }
		if (lane == 0) { S.lims[0] = 0; S.poss[0] = 0; }
		for (uint32_t L = 1; L <= 15u; ++L) {
			u64 m[8]; uint32_t cnt = 0, before = 0;
			#pragma unroll
			for (int k = 0; k < 8; ++k) { m[k] = __ballot(cl[k] == L); cnt += (uint32_t)__builtin_popcountll(m[k]); before += popc_below(m[k]); }
			pos_acc += prevcnt; prevcnt = cnt;                           // poss[L] = poss[L-1] + cnts[L-1], cnts[0] = 0
			if (L < 15u) { const uint32_t inc = cnt << (15u - L); if (last + inc > 32768u) { bad = true; } last += inc; }
			else if (last + cnt > 32768u) { bad = true; }
			if (lane == 0) { S.lims[L] = L < 15u ? last : 32768u; S.poss[L] = pos_acc; }
			uint32_t mine = 0;
			#pragma unroll
			for (int k = 0; k < 8; ++k) { if (cl[k] == L) { const uint32_t at = pos_acc + before + mine; if (at < 512u) { S.syms[at] = (uint16_t)(lane * 8u + k); } ++mine; } }
		}
		if (bad) { status = -3; break; }                                 // :149
		__syncthreads();
		const uint32_t lims9 = S.lims[9];
		const uint32_t lim10 = S.lims[10], lim11 = S.lims[11], lim12 = S.lims[12], lim13 = S.lims[13], lim14 = S.lims[14];   // (for the many-symbols step)
		for (uint32_t i = lane; i < 512u; i += 64u) {
			uint32_t e = 0;
			const uint32_t x = i << 6;
			if (x < lims9) {
				uint32_t L = 1;
				while (x >= S.lims[L]) { ++L; }
				const uint32_t sidx = S.poss[L] + ((x - S.lims[L - 1u]) >> (15u - L));
				const uint32_t sym = sidx < 512u ? S.syms[sidx] : 0xFFFFu;
				e = sym == 0xFFFFu ? 0u : ((sym << 4) | L);
			}
			S.fast[i] = (uint16_t)e;
		}
		__syncthreads();
		// ---- the chunk's symbols (:87-127) ----
		XHD_NEED(ip, 320u)
		uint32_t mask = (rb(ip) << 16) | (rb(ip + 1) << 24) | rb(ip + 2) | (rb(ip + 3) << 8);   // Bitstream.h:44
		uint32_t bits = 32; ip += 4u;
		uint32_t prod = 0;                                               // bytes of this chunk so far, saturating
		bool stream_end = false, skip_wide = false;
		#define XHD_SKIP(k) { mask <<= (k); bits -= (k); if (bits < 16u && ip + 2u <= endq) { XHD_NEED(ip, 2u) mask |= (rb(ip) | (rb(ip + 1) << 8)) << (16u - bits); bits |= 16u; ip += 2u; } }
		#define XHD_MASK_ZERO() (bits == 0 || (mask >> (32u - bits)) == 0)
		#define XHD_DECODE(sym) { const uint32_t r_ = bits; const uint32_t x_ = r_ < 15u ? (((mask >> 16) >> (16u - r_)) << (15u - r_)) : (mask >> 17); \
			const uint32_t f_ = S.fast[x_ >> 6]; uint32_t n_; \
			if (f_) { n_ = f_ & 0xFu; sym = f_ >> 4; if (n_ > r_) { sym = 0xFFFFu; } else { XHD_SKIP(n_) } } \
			else { n_ = x_ >= lims9 ? 10u : 1u; while (x_ >= S.lims[n_]) { ++n_; } \
				if (n_ > r_) { sym = 0xFFFFu; } else { XHD_SKIP(n_) const uint32_t s_ = S.poss[n_] + ((x_ - S.lims[n_ - 1u]) >> (15u - n_)); sym = s_ >= 512u ? 0xFFFFu : S.syms[s_]; } } }
		while (prod < 65536u || !XHD_MASK_ZERO()) {
			// a chunk of an encoder ends with its 65536th byte and an empty bit buffer; what still has bits then runs on in the reference
			// (:87) -- possibly to the end of the buffer. A candidate is not followed there: it counts as "not a chunk", and a buffer
			// whose chain does not close without it goes to the serial walk, which follows the reference to the letter.
			if (!writing && prod >= 65536u) { status = -3; break; }
			if (!skip_wide && prod < 65536u && bits >= 16u && endq - ip >= 24u) {
				// ---- many symbols per step: lane b decodes the symbols that would start b and 64 + b bits from here (the code through the same
				// tables, a match's offset bits behind it); the symbols that really follow each other are then a walk b -> b + bits taken from
				// bit 0, by readlane: ~6 (matches) to 16 (8-bit literals) of them. Stops in front of a match with length bytes (they sit in the byte
				// stream, where the next 16 bits would be pulled from: the symbol-at-a-time code below takes that one) and in front of anything
				// invalid; the bit buffer is rebuilt as Bitstream.h would hold it. (One window of 64 bit offsets per step: 8 191 steps for a chunk of
				// literals, 7.9 ms for the slowest chunk of the bench; with two windows half the steps.)
				XHD_NEED(ip, 24u)
				uint32_t dw[5];                                            // bytes ip .. ip + 19: ten 16-bit words, each the next 16 bits of the stream
				{
					const uint32_t* in32 = reinterpret_cast<const uint32_t*>(S.in);
					const uint32_t i_ = (ip >> 2) & (2u * XHD_INB / 4u - 1u), sh_ = ip & 3u, M_ = 2u * XHD_INB / 4u - 1u;
					uint32_t r_[6];
					#pragma unroll
					for (uint32_t k_ = 0; k_ < 6u; ++k_) { r_[k_] = in32[(i_ + k_) & M_]; }
					#pragma unroll
					for (uint32_t k_ = 0; k_ < 5u; ++k_) { dw[k_] = __builtin_amdgcn_alignbyte(r_[k_ + 1u], r_[k_], sh_); }
				}
				#define XHD_SWAP16(x) (((x) << 16) | ((x) >> 16))              /* word k of the stream first: (w0 << 16) | w1 */
				const u64 t0 = ((u64)XHD_SWAP16(dw[0]) << 32) | XHD_SWAP16(dw[1]), t1 = ((u64)XHD_SWAP16(dw[2]) << 32) | XHD_SWAP16(dw[3]), t2 = (u64)XHD_SWAP16(dw[4]) << 32;
				#undef XHD_SWAP16
				const u64 sq0 = ((u64)mask << 32) | (t0 >> bits), sq1 = (t0 << (64u - bits)) | (t1 >> bits), sq2 = (t1 << (64u - bits)) | (t2 >> bits);   // the next 192 bits (bits + 160 real)
				uint32_t vw[2];
				vw[0] = (uint32_t)((lane ? (sq0 << lane) | (sq1 >> (64u - lane)) : sq0) >> 32);
				vw[1] = (uint32_t)((lane ? (sq1 << lane) | (sq2 >> (64u - lane)) : sq1) >> 32);
				uint32_t stp[2], tokw[2], mln[2], mof[2]; bool ism[2]; u64 evm[2];
				#pragma unroll
				for (uint32_t h_ = 0; h_ < 2u; ++h_) {
					const uint32_t view = vw[h_];
					const uint32_t x15 = view >> 17;
					const uint32_t f = S.fast[x15 >> 6];
					uint32_t n, sy;
					if (f) { n = f & 0xFu; sy = f >> 4; }
					else if (x15 < lims9) { n = 1; sy = 0xFFFFu; }           // a short code that no symbol has (the table says 0 for it too)
					else {                                                   // a code of 10 to 15 bits: its length from the limits (wave-uniform, in registers), no loop
						n = 10u + (x15 >= lim10 ? 1u : 0u) + (x15 >= lim11 ? 1u : 0u) + (x15 >= lim12 ? 1u : 0u) + (x15 >= lim13 ? 1u : 0u) + (x15 >= lim14 ? 1u : 0u);
						const uint32_t s_ = S.poss[n] + ((x15 - S.lims[n - 1u]) >> (15u - n)); sy = s_ >= 512u ? 0xFFFFu : S.syms[s_];
					}
					const bool lit = sy < 0x100u, mat = !lit && sy != 0xFFFFu;
					const uint32_t ob = (sy >> 4) & 0xFu;
					const uint32_t moff = ob ? ((view << n) >> (32u - ob)) + (1u << ob) : 1u;
					const uint32_t mlen = lit ? 1u : (sy & 0xFu) + 3u;
					const bool evl = !lit && (!mat || (sy & 0xFu) == 0xFu);
					evm[h_] = __ballot(evl);
					stp[h_] = evl ? 128u : n + (mat ? ob : 0u);              // (the walk ends on a symbol it must not take, which is then dropped again)
					tokw[h_] = lit ? (0x80000000u | sy) : (moff | (mlen << 16)); mln[h_] = mlen; mof[h_] = moff; ism[h_] = mat;
				}
				u64 mk0 = 0, mk1 = 0; uint32_t b = 0;
				while (b < 64u) { mk0 |= (u64)1 << b; b += (uint32_t)__builtin_amdgcn_readlane((int)stp[0], (int)b); }
				if (mk0 & evm[0]) { b = ctz64(mk0 & evm[0]); mk0 &= ~evm[0]; skip_wide = true; }
				else {
					while (b < 128u) { mk1 |= (u64)1 << (b - 64u); b += (uint32_t)__builtin_amdgcn_readlane((int)stp[1], (int)(b - 64u)); }
					if (mk1 & evm[1]) { b = 64u + ctz64(mk1 & evm[1]); mk1 &= ~evm[1]; skip_wide = true; }
				}
				bool on0 = (mk0 >> lane) & 1u, on1 = (mk1 >> lane) & 1u;
				const uint32_t l0 = on0 ? mln[0] : 0u, in0 = wave_incl_scan_add_u32(l0), tot0 = (uint32_t)__builtin_amdgcn_readlane((int)in0, 63);
				const uint32_t l1 = on1 ? mln[1] : 0u, in1 = tot0 + wave_incl_scan_add_u32(l1);
				const uint32_t bf0 = in0 - l0, bf1 = in1 - l1;
				{	// the chunk is full in front of a symbol: the loop condition decides there
					const u64 ov0 = __ballot(on0 && prod + bf0 >= 65536u), ov1 = __ballot(on1 && prod + bf1 >= 65536u);
					if (ov0) { const uint32_t sl = ctz64(ov0); mk0 &= ((u64)1 << sl) - 1u; mk1 = 0; b = sl; skip_wide = false; }
					else if (ov1) { const uint32_t sl = ctz64(ov1); mk1 &= ((u64)1 << sl) - 1u; b = 64u + sl; skip_wide = false; }
					on0 = (mk0 >> lane) & 1u; on1 = (mk1 >> lane) & 1u;
				}
				if (mk0) {
					const uint32_t adv = mk1 ? (uint32_t)__builtin_amdgcn_readlane((int)in1, (int)(63u - (uint32_t)__builtin_clzll(mk1)))
					                         : (uint32_t)__builtin_amdgcn_readlane((int)in0, (int)(63u - (uint32_t)__builtin_clzll(mk0)));
					const u64 op0 = op + bf0, op1 = op + bf1;
					const uint32_t rc0 = (on0 && ism[0] && (u64)mof[0] > op0) ? (uint32_t)((u64)mof[0] - op0) : 0u;   // how far a match reaches in front of the chunk (offsets are below 65536 + 32768)
					const uint32_t rc1 = (on1 && ism[1] && (u64)mof[1] > op1) ? (uint32_t)((u64)mof[1] - op1) : 0u;
					if (__ballot((rc0 | rc1) != 0)) { const uint32_t rmax = wave_max_u32(rc0 > rc1 ? rc0 : rc1); if (rmax > reach) { reach = rmax; } }
					const uint32_t c0 = (uint32_t)__builtin_popcountll(mk0), c1 = (uint32_t)__builtin_popcountll(mk1);
					const u64 ti0 = nt + popc_below(mk0), ti1 = nt + c0 + popc_below(mk1);
					if (storing && on0 && ti0 < tokcap) { mytok[ti0] = tokw[0]; }
					if (storing && on1 && ti1 < tokcap) { mytok[ti1] = tokw[1]; }
					nt += c0 + c1;
					XHC_CN(0, 1) XHC_CN(1, c0 + c1) XHC_LOC(0)
					op += adv; prod += adv;
					// Bitstream.h:61-75: a word is pulled whenever fewer than 16 bits are left
					const int32_t avail = (int32_t)bits - (int32_t)b;
					const uint32_t pulls = avail < 16 ? (uint32_t)(16 - avail + 15) >> 4 : 0u;
					const uint32_t nb = (uint32_t)(avail + 16 * (int32_t)pulls);
					u64 x64;
					if (b < 64u) { x64 = b ? (sq0 << b) | (sq1 >> (64u - b)) : sq0; }
					else if (b < 128u) { const uint32_t c_ = b - 64u; x64 = c_ ? (sq1 << c_) | (sq2 >> (64u - c_)) : sq1; }
					else { x64 = sq2 << (b - 128u); }
					mask = (uint32_t)(x64 >> 32) & (nb >= 32u ? 0xFFFFFFFFu : ~(0xFFFFFFFFu >> nb));
					bits = nb; ip += 2u * pulls;
					continue;
				}
			}
			skip_wide = false;
			XHC_CN(2, 1) XHC_LOC(1)
			uint32_t sym;
			XHD_DECODE(sym)
			if (sym < 0x100u) {
				XHD_EMIT(0x80000000u | sym)
				++op; ++prod;
			} else {
				if (sym == 0xFFFFu) { status = -3; break; }
				if (sym == 0x100u && ip == endq && XHD_MASK_ZERO()) { stream_end = true; break; }   // :91
				uint32_t len = sym & 0xFu;
				if (len == 0xFu) {
					XHD_NEED(ip, 8u)
					if (endq - ip < 1u) { status = -3; break; }
					len = rb(ip); ip += 1u;
					if (len == 0xFFu) {
						if (endq - ip < 2u) { status = -3; break; }
						len = rb(ip) | (rb(ip + 1) << 8); ip += 2u;
						if (len == 0) {
							if (endq - ip < 4u) { status = -3; break; }
							len = rb(ip) | (rb(ip + 1) << 8) | (rb(ip + 2) << 16) | (rb(ip + 3) << 24); ip += 4u;
						}
						if (len < 0xFu) { status = -3; break; }
						len -= 0xFu;
					}
					len += 0xFu;
				}
				len += 3u;
				const uint32_t ob = (sym >> 4) & 0xFu;
				if (ob > bits) { status = -3; break; }                   // :117
				const uint32_t off = ((mask >> 16) >> (16u - ob)) + (1u << ob);
				XHD_SKIP(ob)
				if (off > op && off - op > reach) { reach = off - op; }   // :120 is judged when the chunk's place in the output is known
				op += len; prod = prod + len < prod ? 0xFFFFFFFFu : prod + len;
				if (PASS != 3 && (writing || (scr && len <= 4u * LZT_MAXLEN))) { while (len > LZT_MAXLEN) { XHD_EMIT(off | (LZT_MAXLEN << 16)) len -= LZT_MAXLEN; } }
				else if (len > LZT_MAXLEN) { nt += (len - 1u) / LZT_MAXLEN; len = LZT_MAXLEN; scr_ok = false; }   // only counted: a candidate that is no chunk may "hold" gigabyte matches
				XHD_EMIT(off | (len << 16))
			}
		}
		if (status != 1) { break; }
		if (!stream_end) {                                               // :128-134: is the next symbol the end of the stream?
			const uint32_t ip_keep = ip;
			uint32_t sym;
			XHD_DECODE(sym)
			if (sym == 0x100u && ip == endq && XHD_MASK_ZERO()) { stream_end = true; } else { ip = ip_keep; }
		}
		state = stream_end ? 1u : 0u; next_at = ip - a0;
		break;                                                           // one chunk
	}
	#undef XHD_BLOCK
	#undef XHD_NEED
	#undef XHD_SKIP
	#undef XHD_MASK_ZERO
	#undef XHD_DECODE
	#undef XHD_EMIT
	XHC_END()
	if (PASS != 2 && lane == 0) {
		xb.res_state[slot] = (status == 1 ? state : 2u) | ((scr && (!scr_ok || nt > XHC_SCR)) ? 4u : 0u); xb.res_end[slot] = next_at; xb.res_prod[slot] = op; xb.res_ntok[slot] = nt;
		xb.res_reach[slot] = reach > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)reach;
	}
}

// one wave per buffer: the chain of chunks from offset 0 through the measured candidates
__global__ __launch_bounds__(64) void xhc_chain_kernel(BatchTables bt, const u64* __restrict__ cand_prefix, XhcBufs xb, u64* __restrict__ ntok,
                                                      u64* __restrict__ d_out_len, int32_t* __restrict__ d_status)
{
	__shared__ uint32_t s_pos[XHC_MAXC];
	const uint32_t lane = threadIdx.x, u = blockIdx.x;
	const uint32_t n = (uint32_t)bt.in_len[u];
	const u64 cap = bt.out_cap[u], base = cand_prefix[u];
	const uint32_t room = (uint32_t)(cand_prefix[u + 1] - base), have = xb.cand_cnt[u];
	bool ok = have >= 1u && have <= room && have <= XHC_MAXC;
	const uint32_t cnt = ok ? have : 0u;
	for (uint32_t i = lane; i < cnt; i += 64u) { s_pos[i] = xb.cand_pos[base + i]; xb.tok_off[base + i] = ~(u64)0; }
	__syncthreads();
	uint32_t pos = 0, steps = 0; u64 out = 0, nt = 0; bool success = false;
	while (ok) {
		uint32_t found = 0xFFFFFFFFu;
		for (uint32_t i0 = 0; i0 < cnt; i0 += 64u) {
			const u64 m = __ballot(i0 + lane < cnt && s_pos[i0 + lane] == pos);
			if (m) { found = i0 + ctz64(m); break; }
		}
		if (found == 0xFFFFFFFFu) { break; }
		const u64 sl = base + found;
		const uint32_t st = xb.res_state[sl] & 3u, reach = xb.res_reach[sl], end = xb.res_end[sl];
		if (st == 2u || reach == 0xFFFFFFFFu || (u64)reach > out) { break; }     // not a chunk, or a match reaches in front of the buffer (:120)
		if (lane == 0) { xb.tok_off[sl] = nt; }
		out += xb.res_prod[sl]; nt += xb.res_ntok[sl];
		if (st == 1u) { success = end == n; break; }
		if (end <= pos || ++steps > cnt) { break; }
		pos = end;
	}
	success = success && out <= cap;                                     // beyond the capacity: the serial walk says where and how
	if (lane == 0) {
		xb.mode[u] = success ? XHC_SPEC : XHC_SERIAL;
		if (success) { d_status[u] = 0; d_out_len[u] = out; ntok[u] = nt; }
	}
}

// the tokens of the accepted chunks of a buffer with token scratch: from where PASS 1 left them to their place in the buffer's token stream
__global__ __launch_bounds__(256) void xhc_gather_kernel(BatchTables bt, const u64* __restrict__ tok_prefix, const u64* __restrict__ cand_prefix, XhcBufs xb, uint32_t* __restrict__ tok)
{
	const uint32_t slot = blockIdx.x;
	const uint32_t u = seg_of_flat(cand_prefix, bt.n_units, slot);
	const uint32_t idx = slot - (uint32_t)cand_prefix[u];
	const uint32_t have = xb.cand_cnt[u], room = (uint32_t)(cand_prefix[u + 1] - cand_prefix[u]);
	if (idx >= (have < room ? have : room)) { return; }
	if (xb.scr_prefix == nullptr || xb.scr_prefix[u + 1] <= xb.scr_prefix[u]) { return; }
	if (xb.mode[u] != XHC_SPEC || xb.tok_off[slot] == ~(u64)0 || xb.cand_pos[slot] == 0 || (xb.res_state[slot] & 4u)) { return; }
	const uint32_t* __restrict__ from = xb.scr_tok + (xb.scr_prefix[u] + idx) * (u64)XHC_SCR;
	uint32_t* __restrict__ to = tok + tok_prefix[u] + xb.tok_off[slot];
	const uint32_t cnt = (uint32_t)xb.res_ntok[slot];
	for (uint32_t i = threadIdx.x; i < cnt; i += 256u) { to[i] = from[i]; }
}

// ---- launchers: one per stage, in the order they run (launch.hip decode_launch / size_launch) ---------------------------------------------
void launch_xhc_mark(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const u64* cand_prefix, const XhcBufs& xb, bool dev)
{
	if (bt.n_units == 0) { return; }
	if (dev) {                                                           // (a kernel, not a memset: kernels.h launch_dev_zero)
		launch_dev_zero(st, xb.cand_cnt, bt.n_units + 1u);
		hipLaunchKernelGGL(xhc_mark_kernel<true>, dim3(bt.n_chunks), dim3(256), 0, st, d_in, bt, cand_prefix, xb);
	} else {
		(void)hipMemsetAsync(xb.cand_cnt, 0, ((size_t)bt.n_units + 1) * sizeof(uint32_t), st);
		hipLaunchKernelGGL(xhc_mark_kernel<false>, dim3(bt.n_chunks), dim3(256), 0, st, d_in, bt, cand_prefix, xb);
	}
}
void launch_xhc_candidates(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const u64* tok_prefix, const u64* cand_prefix, uint32_t n_slots, const XhcBufs& xb, uint32_t* tok)
{
	if (bt.n_units) { hipLaunchKernelGGL(xhc_parse_kernel<1>, dim3(n_slots), dim3(64), 0, st, d_in, bt, tok_prefix, cand_prefix, xb, tok); }
}
void launch_xhc_candidates_size(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const u64* cand_prefix, uint32_t n_slots, const XhcBufs& xb)
{
	if (bt.n_units) { hipLaunchKernelGGL(xhc_parse_kernel<3>, dim3(n_slots), dim3(64), 0, st, d_in, bt, (const u64*)nullptr, cand_prefix, xb, (uint32_t*)nullptr); }
}
void launch_xhc_chain(hipStream_t st, const BatchTables& bt, const u64* cand_prefix, const XhcBufs& xb, u64* ntok, u64* d_out_len, int32_t* d_status)
{
	if (bt.n_units) { hipLaunchKernelGGL(xhc_chain_kernel, dim3(bt.n_units), dim3(64), 0, st, bt, cand_prefix, xb, ntok, d_out_len, d_status); }
}
void launch_xhc_tokens(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const u64* tok_prefix, const u64* cand_prefix, uint32_t n_slots, const XhcBufs& xb, uint32_t* tok)
{
	if (bt.n_units == 0) { return; }
	if (xb.scr_prefix) { hipLaunchKernelGGL(xhc_gather_kernel, dim3(n_slots), dim3(256), 0, st, bt, tok_prefix, cand_prefix, xb, tok); }
	hipLaunchKernelGGL(xhc_parse_kernel<2>, dim3(n_slots), dim3(64), 0, st, d_in, bt, tok_prefix, cand_prefix, xb, tok);
}
void launch_xhd_parse(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const u64* tok_prefix, uint32_t* tok, u64* ntok, u64* d_out_len, int32_t* d_status, const uint32_t* mode)
{
	if (bt.n_units) { hipLaunchKernelGGL(xhd_parse_kernel<true>, dim3(bt.n_units), dim3(64), 0, st, d_in, bt, tok_prefix, tok, ntok, d_out_len, d_status, mode); }
}
void launch_xhd_size(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, u64* ntok, u64* d_out_len, int32_t* d_status, const uint32_t* mode)
{
	if (bt.n_units) { hipLaunchKernelGGL(xhd_parse_kernel<false>, dim3(bt.n_units), dim3(64), 0, st, d_in, bt, (const u64*)nullptr, (uint32_t*)nullptr, ntok, d_out_len, d_status, mode); }
}

} // namespace msc
