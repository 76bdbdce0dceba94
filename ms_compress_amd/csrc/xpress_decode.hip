// xpress_decode.hip -- gfx950 Xpress decompressor, batch form: n independent units resident in HBM.
//   xpd_kernel         one wave walks and copies one stream (8 KiB window in an LDS ring)                         [comment at the kernel]
//   xpt_parse_kernel   one wave walks one stream a flag word at a time and writes 32-bit tokens; the large streams are walked by
//                      segments first (xps_*); the bytes follow from the tokens (lz_copy.hip, lzglobal.hip)       [comments at the kernels]
// Size query (mscomp_amd_plan_create_size): the same walks with every test, no byte stage or token store -- xpt_parse_kernel<false> / xps_emit_kernel<false>.
// Status and length per unit are those of the reference's one-shot call (lznt1_decode.hip says how that is checked).
#include "kernels.h"

namespace msc {

// xpress_decompress (/root/reference/src/xpress_decompress.cpp:405-462, READ_SYMBOL :62-107): a stream is one chain of tokens - where
// a token starts depends on every token before it (32-bit flag words, 1 / 2 / 3 / 4 / 6 / 10-byte tokens, a length nibble shared
// by two matches) - so a stream is decoded by one wave, streams in parallel. All lanes run the token walk (it is uniform).
// The input is staged through a 2 KiB LDS ring (1 KiB blocks, loaded when the walk gets there), the output through a 10 KiB ring
// from which matches are copied (offsets reach 8192 bytes back) and which goes to HBM in 2 KiB pieces: 12.3 KiB of LDS, 13
// streams per CU. A literal run and a match are moved by the lanes together. The 8 bytes at the next token are fetched (3
// aligned dword reads) before the current token's bytes are moved, so a token costs about one LDS round trip.
#define XPD_INB  1024u
#define XPD_RING 10240u
#define XPD_PIECE 2048u
struct XpdLds { __attribute__((aligned(16))) uint8_t in[2u * XPD_INB]; __attribute__((aligned(16))) uint8_t out[XPD_RING]; };

__global__ __launch_bounds__(64) void xpd_kernel(const uint8_t* __restrict__ d_in, BatchTables bt, uint8_t* __restrict__ d_out,
                                                u64* __restrict__ d_out_len, int32_t* __restrict__ d_status)
{
	__shared__ XpdLds S;
	const uint32_t lane = threadIdx.x, u = blockIdx.x;
	const uint32_t n = (uint32_t)bt.in_len[u];
	const u64 cap = bt.out_cap[u];
	const uint8_t* src = d_in + bt.in_off[u];
	uint8_t* dst = d_out + bt.out_off[u];
	int32_t status = -3; u64 op = 0;
	if (n < 5u) {                                                        // :414-418
		bool ok = n == 0;
		if (n == 4u) { ok = ((uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | ((uint32_t)src[3] << 24)) != 0xFFFFFFFFu; }
		if (lane == 0) { d_status[u] = ok ? 0 : -3; d_out_len[u] = 0; }
		return;
	}
	// ---- input ring: q = offset from the 16-byte aligned base (32 bits: units are below 4 GiB - 4096); block b = q in [1024 b, 1024 (b+1)) ----
	const uint32_t a0 = (uint32_t)((uintptr_t)src & 15u);
	const uint8_t* ab = src - a0;
	const uint32_t endq = a0 + n;
	uint32_t loaded = 0;                                                 // blocks of 1024 input bytes brought to LDS so far (the last two are resident)
	#define XPD_BLOCK() { __syncthreads(); { const u64 q_ = (u64)loaded * XPD_INB + lane * 16u; \
			*reinterpret_cast<uint4*>(S.in + (loaded & 1u) * XPD_INB + lane * 16u) = q_ < endq ? *reinterpret_cast<const uint4*>(ab + q_) : make_uint4(0, 0, 0, 0); } \
		++loaded; __syncthreads(); }
	XPD_BLOCK() XPD_BLOCK()
	auto rb = [&](uint32_t q) -> uint32_t { return S.in[q & (2u * XPD_INB - 1u)]; };
	const uint32_t* in32 = reinterpret_cast<const uint32_t*>(S.in);
	// bytes q .. q+7 as two dwords
	#define XPD_FETCH8(q, lo, hi) { const uint32_t i_ = ((q) >> 2) & (2u * XPD_INB / 4u - 1u), sh_ = (q) & 3u; \
		const uint32_t w0_ = in32[i_], w1_ = in32[(i_ + 1u) & (2u * XPD_INB / 4u - 1u)], w2_ = in32[(i_ + 2u) & (2u * XPD_INB / 4u - 1u)]; \
		lo = __builtin_amdgcn_alignbyte(w1_, w0_, sh_); hi = __builtin_amdgcn_alignbyte(w2_, w1_, sh_); }
	// ---- output ring: coordinate r = output offset + d0 (d0 = alignment of the destination): pieces of 2048 are 16-byte aligned in HBM ----
	const uint32_t d0 = (uint32_t)((uintptr_t)dst & 15u);
	uint8_t* db = dst - d0;
	u64 flushed = 0;                                                     // ring coordinate up to which the output is in HBM (multiple of XPD_PIECE)
	uint32_t fi = 0;                                                     // flushed mod XPD_RING
	#define XPD_FLUSH() { _Pragma("unroll") for (uint32_t i_ = 0; i_ < 2u; ++i_) { const uint32_t o_ = (i_ * 64u + lane) * 16u; const u64 r_ = flushed + o_; \
			if (r_ >= d0) { *reinterpret_cast<uint4*>(db + r_) = *reinterpret_cast<const uint4*>(S.out + fi + o_); } \
			else { for (uint32_t k_ = d0; k_ < 16u; ++k_) { db[r_ + k_] = S.out[fi + o_ + k_]; } } } \
		flushed += XPD_PIECE; fi += XPD_PIECE; if (fi == XPD_RING) { fi = 0; } }
	auto wrap = [](uint32_t x) -> uint32_t { return x >= XPD_RING ? x - XPD_RING : x; };
	uint32_t wi = d0;                                                    // ring index of output offset op
	u64 nextflush = XPD_PIECE - d0;                                      // output offset at which the next piece is complete
	uint32_t ip = a0;
	uint32_t half = 0; bool have_half = false;
	bool done = false;
	uint32_t lo = 0, hi = 0;
	XPD_FETCH8(ip, lo, hi)
	while (!done) {
		if (ip + 4u > endq) { status = -3; break; }                     // :461 the input ended at a flag word
		while ((u64)loaded * XPD_INB < (u64)ip + 352u && (u64)loaded * XPD_INB < endq) {   // a flag word and its 32 tokens take at most 4 + 32 * 10 bytes
			XPD_BLOCK()
			XPD_FETCH8(ip, lo, hi)
		}
		uint32_t flags = lo;
		uint32_t flagged = flags >> 31;
		flags = (flags << 1) | 1u; ip += 4u;
		lo = hi; XPD_FETCH8(ip, lo, hi)
		do {
			if (ip == endq) {                                            // :433-438
				const uint32_t x = ~flags;
				status = (flagged && !((x + 1u) & x)) ? 0 : -3; done = true; break;
			}
			if (flagged) {
				if (ip + 2u > endq) { status = -3; done = true; break; }
				const uint32_t sym = lo & 0xFFFFu;
				uint32_t used = 2u;                                      // bytes of this token; byte k of the token is (k < 4 ? lo : hi) >> 8 (k & 3)
				const uint32_t off = (sym >> 3) + 1u; uint32_t len = sym & 7u;
				if (len == 7u) {
					if (have_half) { len = half >> 4; have_half = false; }
					else if (ip + used == endq) { status = -3; done = true; break; }
					else { half = (lo >> 16) & 0xFFu; used = 3u; have_half = true; len = half & 0xFu; }
					if (len == 0xFu) {
						if (ip + used == endq) { status = -3; done = true; break; }
						len = used == 2u ? (lo >> 16) & 0xFFu : lo >> 24; ++used;
						if (len == 0xFFu) {
							if (ip + used + 2u > endq) { status = -3; done = true; break; }
							len = used == 3u ? ((lo >> 24) | ((hi & 0xFFu) << 8)) : (hi & 0xFFFFu); used += 2u;
							if (len == 0) {
								if (ip + used + 4u > endq) { status = -3; done = true; break; }
								const uint32_t q4 = ip + used;
								len = rb(q4) | (rb(q4 + 1u) << 8) | (rb(q4 + 2u) << 16) | (rb(q4 + 3u) << 24); used += 4u;
							}
							if (len < 0xFu + 0x7u) { status = -3; done = true; break; }
							len -= 0xFu + 0x7u;
						}
						len += 0xFu;
					}
					len += 0x7u;
				}
				len += 0x3u;
				ip += used;
				XPD_FETCH8(ip, lo, hi)                                  // the next token's bytes travel while this one is copied
				if (off > op) { status = -3; done = true; break; }       // :442
				if (len > cap - op) { status = -5; done = true; break; } // :443
				uint32_t left = len;
				if (off >= 64u) {
					uint32_t si = wi >= off ? wi - off : wi + XPD_RING - off;
					while (left) {
						const uint32_t step = left < 64u ? left : 64u;
						if (lane < step) { S.out[wrap(wi + lane)] = S.out[wrap(si + lane)]; }
						wi = wrap(wi + step); si = wrap(si + step); op += step; left -= step;
						if (op >= nextflush) { __syncthreads(); XPD_FLUSH() nextflush += XPD_PIECE; }
					}
				} else {
					const float ro = __builtin_amdgcn_rcpf((float)off);  // off < 64: (x + 0.5) / off is never within 1e-3 of an integer
					const uint32_t span = (uint32_t)(64.5f * ro) * off;  // whole periods per step
					const uint32_t lm = lane - (uint32_t)(((float)lane + 0.5f) * ro) * off;
					const uint32_t s0 = wi >= off ? wi - off : wi + XPD_RING - off;
					const uint32_t v = S.out[wrap(s0 + lm)];
					while (left) {
						const uint32_t step = left < span ? left : span;
						if (lane < step) { S.out[wrap(wi + lane)] = (uint8_t)v; }
						wi = wrap(wi + step); op += step; left -= step;
						if (op >= nextflush) { __syncthreads(); XPD_FLUSH() nextflush += XPD_PIECE; }
					}
				}
				flagged = flags >> 31; flags <<= 1;
			} else {
				// a run of literals: this token and the zero flags behind it, as far as input and room reach
				uint32_t run = (uint32_t)__builtin_clz(flags) + 1u;
				if (op == cap) { status = -5; done = true; break; }      // :455
				if (run > endq - ip) { run = endq - ip; }
				if ((u64)run > cap - op) { run = (uint32_t)(cap - op); }
				if (lane < run) { S.out[wrap(wi + lane)] = (uint8_t)rb(ip + lane); }
				op += run; ip += run; wi = wrap(wi + run);
				XPD_FETCH8(ip, lo, hi)
				if (op >= nextflush) { __syncthreads(); XPD_FLUSH() nextflush += XPD_PIECE; }
				flagged = (uint32_t)(((u64)flags << (run - 1u)) >> 31) & 1u;
				flags = (uint32_t)((u64)flags << run);
			}
		} while (flags);
	}
	#undef XPD_BLOCK
	#undef XPD_FETCH8
	// the rest of the ring
	__syncthreads();
	if (status == 0) {
		const u64 rend = op + d0;
		for (u64 r = flushed + lane; r < rend; r += 64u) { if (r >= d0) { db[r] = S.out[wrap(fi + (uint32_t)(r - flushed))]; } }
	}
	#undef XPD_FLUSH
	if (lane == 0) { d_status[u] = status; d_out_len[u] = status == 0 ? op : 0; }
}

void launch_xpress_decompress(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, uint8_t* d_out, u64* d_out_len, int32_t* d_status)
{
	if (bt.n_units == 0) { return; }
	hipLaunchKernelGGL(xpd_kernel, dim3(bt.n_units), dim3(64), 0, st, d_in, bt, d_out, d_out_len, d_status);
}

// ---- the same stream as TOKENS, a flag word at a time ---------------------------------------------------------------------------------
// xpd_kernel above takes one token per step (and moves its bytes): 450 cycles per token, 3.7 s for one 51 MB stream. But where the 32 tokens
// of a flag word start is known at once unless a match carries extra length bytes: a literal takes 1 byte, a match 2, so token r starts
// r + (matches before r) bytes behind the flag word, and only a match whose 3-bit length field is 7 (a match of 10 bytes or more) takes more.
// So lane r reads token r. Such a match takes its length from a nibble, two nibbles to a byte that the first of the two brings along: the
// tokens behind it move by one, and by one more behind a nibble of 15 with its length byte -- found by a short iteration (below). Only the
// longer forms (a match of 280 bytes or more) stop the lanes: the tokens before it are decoded, checked (READ_SYMBOL's and the copy's tests, :62-107 / :442-455, with the
// output offset from a wave scan of the lengths) and written as 32-bit tokens together, that match is decoded by all lanes as one, and
// the rest of the flag word goes the same way from behind it.
// The bytes are produced afterwards by lz_copy_kernel / lz_copy_block_kernel, as for Xpress+Huffman. Status and length are those of the
// serial walk: the first token, in order, that fails decides.
#define XPT_INB 1024u
#define XPS_DONE 0x5EC0D0E5u
// The walk of one wave from a flag word on: state in / state out. EMIT: tokens are written at mytok[tc ...] and the copy's tests (:442-443, :455)
// are made against the output offset `op` and the capacity; without it the walk only counts (tokens, bytes) -- for a stretch of a stream whose
// place in the output is not known yet (xps_* below). It ends in front of the first flag word at or behind `limit` (running = true) or where
// the reference's loop ends (status). Offsets are relative to the 16-byte aligned base `ab`, as in xpd_kernel.
// CHECK (defaults to EMIT): the offset test of :442 against the absolute `op`. CHECK without EMIT is the size query's walk: every test, no store.
struct XptWalk { uint32_t ip; u64 op, tc; uint32_t half, hp; bool have_half; int32_t status; bool running; };
#define XPT_BLOCK() { __syncthreads(); *reinterpret_cast<uint4*>(s_in + (loaded & 1u) * XPT_INB + lane * 16u) = nxt; ++loaded; \
	{ const u64 q_ = (u64)loaded * XPT_INB + lane * 16u; nxt = q_ < endq ? *reinterpret_cast<const uint4*>(ab + q_) : make_uint4(0, 0, 0, 0); } __syncthreads(); }
template <bool EMIT, bool CHECK = EMIT>
__device__ __forceinline__ void xpt_walk(uint8_t* s_in, const uint8_t* __restrict__ ab, const uint32_t endq, uint32_t& loaded, uint4& nxt, XptWalk& W,
                                         const uint32_t limit, const u64 cap, uint32_t* __restrict__ mytok, const uint32_t lane)
{
	auto rb = [&](uint32_t q) -> uint32_t { return s_in[q & (2u * XPT_INB - 1u)]; };
	const uint32_t* in32 = reinterpret_cast<const uint32_t*>(s_in);
	uint32_t ip = W.ip, half = W.half, hp = W.hp;
	u64 op = W.op, tc = W.tc;
	bool have_half = W.have_half, done = false, running = false;
	int32_t status = -3;
	while (!done) {
		if (ip >= limit) { running = true; break; }                     // a flag word at or behind the limit: the walk stops in front of it
		if (ip + 4u > endq) { status = -3; break; }                     // :461 the input ended at a flag word
		while ((u64)loaded * XPT_INB < (u64)ip + 352u && (u64)loaded * XPT_INB < endq) { XPT_BLOCK() }   // a flag word and its 32 tokens take at most 4 + 32 * 10 bytes
		uint32_t m;                                                      // bit i: token i is a match
		{ const uint32_t i_ = (ip >> 2) & (2u * XPT_INB / 4u - 1u); m = __builtin_bitreverse32(__builtin_amdgcn_alignbyte(in32[(i_ + 1u) & (2u * XPT_INB / 4u - 1u)], in32[i_], ip & 3u)); }
		ip += 4u;
		uint32_t j0 = 0;                                                 // first token of the flag word not taken yet
		while (j0 < 32u) {
			const uint32_t mm = m >> j0, cntl = 32u - j0, r = lane & 31u;
			const bool act = lane < cntl;
			const bool is_m = (mm >> r) & 1u;
			// Matches with length field 7 ("long") take their length from a nibble: every other one brings a byte for two of them (the
			// first, if none is pending, :88-95), which moves the tokens behind it by one. Which matches are long depends on where they
			// are, and that on the long ones before them: solved by iteration -- positions from the current set, the set from the symbols at
			// those positions, until it stands. A nibble of 15 is followed by a length byte (:96-99; 255 there: longer forms, not taken here), one
			// more byte to move by: a second set, iterated along. The sets are right up to one token further every round at least (token 0 is
			// always right) and the true sets are a fixed point, the only one; typically 1 + the number of shifting matches rounds.
			const uint32_t below = (1u << r) - 1u, mbefore = (uint32_t)__builtin_popcount(mm & below);
			const uint32_t hsel = have_half ? 1u : 0u;                   // which long matches bring the nibble byte: every other one, the first unless a nibble is pending
			uint32_t longs = 0, ext1 = 0, q, w, hbn, nib, extb;
			bool lng, brings, e1;
			for (;;) {
				const uint32_t kb = (uint32_t)__builtin_popcount(longs & below);
				q = ip + r + mbefore + ((kb + 1u - hsel) >> 1) + (uint32_t)__builtin_popcount(ext1 & below);
				{ const uint32_t i_ = (q >> 2) & (2u * XPT_INB / 4u - 1u); w = __builtin_amdgcn_alignbyte(in32[(i_ + 1u) & (2u * XPT_INB / 4u - 1u)], in32[i_], q & 3u); }   // bytes q .. q+3
				lng = act && is_m && (w & 7u) == 7u;
				const uint32_t now = (uint32_t)__ballot(lng);
				hbn = (w >> 16) & 0xFFu;
				if (now == 0) { brings = false; e1 = false; nib = 0; extb = 0; if (longs == 0 && ext1 == 0) { break; } longs = 0; ext1 = 0; continue; }   // no long match at all: most flag words of text
				const uint32_t kn = (uint32_t)__builtin_popcount(now & below);
				brings = lng && ((kn & 1u) == hsel);
				const uint32_t pv = now & below;
				const uint32_t hprev = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((31u - (uint32_t)__builtin_clz(pv ? pv : 1u)) << 2), (int)hbn);
				nib = brings ? (hbn & 0xFu) : ((kn ? hprev : half) >> 4);
				extb = brings ? w >> 24 : hbn;                          // the length byte behind a nibble of 15
				e1 = lng && nib == 0xFu && extb != 0xFFu;
				const uint32_t now1 = (uint32_t)__ballot(e1);
				if (now == longs && now1 == ext1) { break; }
				longs = now; ext1 = now1;
			}
			const uint32_t b0 = w & 0xFFu, sym = w & 0xFFFFu;
			const bool gone = q >= endq;
			const bool cut = is_m && (q + 2u > endq || (brings && q + 2u == endq) || (lng && nib == 0xFu && q + 2u + (brings ? 1u : 0u) >= endq));   // :64 / :92 / :97
			const u64 ev = __ballot(act && (gone || cut || (lng && nib == 0xFu && !e1)));
			const uint32_t first = ev ? ctz64(ev) : cntl;                // tokens j0 .. j0 + first - 1 are plain: literals and matches of up to 279 bytes
			const bool plain = lane < first;
			const uint32_t len = is_m ? (lng ? (e1 ? extb + 25u : nib + 10u) : (sym & 7u) + 3u) : 1u, off = (sym >> 3) + 1u;
			const uint32_t l = plain ? len : 0u, incl = wave_incl_scan_add_u32(l);
			const u64 opi = op + (incl - l);
			const bool bad_off = CHECK && plain && is_m && (u64)off > opi;                                   // :442
			const bool bad_cap = plain && (is_m ? (u64)len > cap - opi : opi >= cap);               // :443 / :455
			const u64 eb = __ballot(bad_off || bad_cap);
			if (eb) {
				const uint32_t e = ctz64(eb);
				status = ((__ballot(bad_off) >> e) & 1u) ? -3 : -5; done = true; break;
			}
			if (EMIT && plain) { mytok[tc + lane] = is_m ? ((len << 16) | off) : (0x80000000u | b0); }
			tc += first;
			op += first ? (uint32_t)__builtin_amdgcn_readlane((int)incl, (int)(first - 1u)) : 0u;
			{	// the nibble state behind the plain tokens
				const uint32_t pl = longs & (first < 32u ? (1u << first) - 1u : 0xFFFFFFFFu);
				if (pl) {
					const bool pend = have_half ^ (((uint32_t)__builtin_popcount(pl) & 1u) != 0);
					if (pend) { const uint32_t ll_ = 31u - (uint32_t)__builtin_clz(pl); half = (uint32_t)__builtin_amdgcn_readlane((int)hbn, (int)ll_); hp = (uint32_t)__builtin_amdgcn_readlane((int)q, (int)ll_) + 2u; }   // (the last long one brought it)
					have_half = pend;
				}
			}
			if (first == cntl) { ip = (uint32_t)__builtin_amdgcn_readlane((int)(q + (is_m ? 2u : 1u) + (brings ? 1u : 0u) + (e1 ? 1u : 0u)), (int)(cntl - 1u)); break; }
			ip = (uint32_t)__builtin_amdgcn_readlane((int)q, (int)first);
			if ((__ballot(gone) >> first) & 1u) {                        // :433-438: the input ends here: this flag and all behind it must be set
				const uint32_t k = j0 + first;
				status = (m >> k) == (0xFFFFFFFFu >> k) ? 0 : -3; done = true; break;
			}
			if ((__ballot(cut) >> first) & 1u) { status = -3; done = true; break; }
			// a match with extra length bytes, by all lanes as one (READ_SYMBOL :62-107)
			const uint32_t sy = (uint32_t)__builtin_amdgcn_readlane((int)sym, (int)first);
			const uint32_t loff = (sy >> 3) + 1u;
			uint32_t used = 2u, ll;
			if (have_half) { ll = half >> 4; have_half = false; }
			else if (ip + used == endq) { status = -3; done = true; break; }
			else { half = rb(ip + 2u); hp = ip + 2u; used = 3u; have_half = true; ll = half & 0xFu; }
			if (ll == 0xFu) {
				if (ip + used == endq) { status = -3; done = true; break; }
				ll = rb(ip + used); ++used;
				if (ll == 0xFFu) {
					if (ip + used + 2u > endq) { status = -3; done = true; break; }
					ll = rb(ip + used) | (rb(ip + used + 1u) << 8); used += 2u;
					if (ll == 0) {
						if (ip + used + 4u > endq) { status = -3; done = true; break; }
						ll = rb(ip + used) | (rb(ip + used + 1u) << 8) | (rb(ip + used + 2u) << 16) | (rb(ip + used + 3u) << 24); used += 4u;
					}
					if (ll < 0xFu + 0x7u) { status = -3; done = true; break; }
					ll -= 0xFu + 0x7u;
				}
				ll += 0xFu;
			}
			ll += 0x7u + 0x3u;
			if (CHECK && (u64)loff > op) { status = -3; done = true; break; }    // :442
			if ((u64)ll > cap - op) { status = -5; done = true; break; } // :443
			const uint32_t np = ll / LZT_MAXLEN + (ll % LZT_MAXLEN ? 1u : 0u);    // pieces with the same offset copy the same bytes
			for (uint32_t k = lane; EMIT && k < np; k += 64u) { mytok[tc + k] = ((k + 1u == np ? ll - (np - 1u) * LZT_MAXLEN : LZT_MAXLEN) << 16) | loff; }
			tc += np; op += ll; ip += used;
			j0 += first + 1u;
		}
	}
	W.ip = ip; W.op = op; W.tc = tc; W.half = half; W.hp = hp; W.have_half = have_half; W.status = status; W.running = running;
}

// ring start for a walk that begins at offset ip0 (from the aligned base): blocks ip0 / 1024 and the next one resident, the third on its way
#define XPT_RING_START(ip0) { loaded = (ip0) / XPT_INB; { const u64 q_ = (u64)loaded * XPT_INB + lane * 16u; nxt = q_ < endq ? *reinterpret_cast<const uint4*>(ab + q_) : make_uint4(0, 0, 0, 0); } XPT_BLOCK() XPT_BLOCK() }

// EMIT = false: the size query (tok / tok_prefix unused)
template <bool EMIT = true>
__global__ __launch_bounds__(64) void xpt_parse_kernel(const uint8_t* __restrict__ d_in, BatchTables bt, const u64* __restrict__ tok_prefix, uint32_t* __restrict__ tok,
                                                      u64* __restrict__ ntok, u64* __restrict__ d_out_len, int32_t* __restrict__ d_status, const uint32_t* __restrict__ spec_done)
{
	__shared__ __attribute__((aligned(16))) uint8_t s_in[2u * XPT_INB];
	const uint32_t lane = threadIdx.x, u = blockIdx.x;
	if (spec_done && spec_done[u] == XPS_DONE) { return; }              // the segment-parallel walk has done this stream (xps_* below)
	const uint32_t n = (uint32_t)bt.in_len[u];
	const u64 cap = bt.out_cap[u];
	const uint8_t* src = d_in + bt.in_off[u];
	uint32_t* __restrict__ mytok = EMIT ? tok + tok_prefix[u] : nullptr;
	if (n < 5u) {                                                        // :414-418
		bool ok = n == 0;
		if (n == 4u) { ok = ((uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | ((uint32_t)src[3] << 24)) != 0xFFFFFFFFu; }
		if (lane == 0) { d_status[u] = ok ? 0 : -3; d_out_len[u] = 0; ntok[u] = 0; }
		return;
	}
	// input ring as in xpd_kernel (two blocks of 1024 bytes); the block after the newest one is already on its way from HBM, in registers
	const uint32_t a0 = (uint32_t)((uintptr_t)src & 15u);
	const uint8_t* ab = src - a0;
	const uint32_t endq = a0 + n;
	uint32_t loaded; uint4 nxt;
	XPT_RING_START(a0)
	XptWalk W = { a0, 0, 0, 0, 0, false, -3, false };
	xpt_walk<EMIT, true>(s_in, ab, endq, loaded, nxt, W, 0xFFFFFFFFu, cap, mytok, lane);
	if (lane == 0) { d_status[u] = W.status; d_out_len[u] = W.status == 0 ? W.op : 0; ntok[u] = W.status == 0 ? W.tc : 0; }
}

// ---- ONE large Xpress stream by many waves (SURVEY.md 8f-1 / 8f-2a on the decoding side) ----------------------------------------------------
// Where a flag word starts is known only to a walk that comes from the start of the stream. But a walk that starts at a WRONG place falls
// into step with the right one sooner or later (tools/xp_sync_study.py: after 2 KB in the median, 27 KB at the 90th, 137 KB at the 99th
// percentile of 4 800 starts in the corpus: whenever it reaches a flag word of the right walk in the right state, it IS the right walk).
// So the input of a stream is cut into segments of XPS_SEG bytes (16 KiB) and
//   round 0: a wave per segment starts XPS_WARM bytes before its segment as if a flag word began there (no nibble pending), notes the state
//            in which it arrives at the first flag word at or behind the segment start ("landing": offset, pending nibble and where its byte
//            is) and counts tokens and bytes from there to the first flag word at or behind the segment end ("exit"). Segment 0 starts at the start.
//   check:   segment k holds if its landing is the exit of segment k - 1 (and that one ran on); by induction from segment 0 a chain of
//            holding segments is the true parse. The FIRST of a run of segments that do not hold is walked again from the exit of the segment
//            before it -- a segment that holds, so this is the true state -- and goes on through the run until it arrives where a later
//            segment had landed: one round per run, whatever its length (there are stretches of 100 KB and more that no speculative walk
//            enters: flag words 0xAAAAAAAA / 0x55555555 in a lattice of 52-54 bytes, DESIGN_DECODERS.md). XPS_ROUNDS rounds are launched; a segment
//            behind a run may stop holding when the run's exit changes, which is what the further rounds are for.
//   emit:    with the segments' token and byte counts summed up, every segment is walked once more from its true state, writing its tokens
//            at their place and making the tests that need the output offset.
// Whatever does not fit this picture -- a segment that ends in an error, more rounds needed, a test failing, output beyond the capacity --
// sends the stream to the one-wave walk above, which gives the reference's status to the letter.
struct XpsSeg { uint32_t l_ip, l_hp, e_ip, e_hp, kind, redo; u64 ntok, nout, tbase, obase, pad_; };
static_assert(sizeof(XpsSeg) == XPS_SEG_BYTES, "XpsSeg");   // l_hp / e_hp: 0xFFFFFFFF = no nibble pending; kind: 0 ran on, 1 the stream ended well, 2 anything else
__device__ __forceinline__ XpsSeg* xps_segs(const XpsTables& x, uint32_t b) { return reinterpret_cast<XpsSeg*>(static_cast<uint8_t*>(x.seg) + x.seg_prefix[b] * XPS_SEG_BYTES); }
__device__ __forceinline__ void xps_segment_of(const XpsTables& x, uint32_t n_big, uint32_t flat, uint32_t& b, uint32_t& k)
{
	uint32_t lo = 0, hi = n_big;
	while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (x.seg_prefix[mid] <= flat) { lo = mid; } else { hi = mid; } }
	b = lo; k = flat - (uint32_t)x.seg_prefix[lo];
}
// DEV instances (a dev plan with large units): the grids are sized for the plan's bounds, the stream list and the counts of this execution
// were written by its path pass (x.cnt: streams, segments), and a block past the real count returns at once. The <false> instances are the
// kernels of host plans, which grid by the counts themselves.
template <bool DEV> __device__ __forceinline__ uint32_t xps_streams(const XpsTables& x) { return DEV ? x.cnt[0] : x.n_big; }

template <bool DEV>
__global__ void xps_init_kernel(XpsTables x) { const uint32_t b = blockIdx.x * 256u + threadIdx.x; if (b < xps_streams<DEV>(x)) { x.mode[b] = 1u; } }

// ROUND 0: every segment (speculative start); ROUND > 0: the segments the check marked, from the exit of the segment before
template <int ROUND, bool DEV>
__global__ __launch_bounds__(64) void xps_walk_kernel(const uint8_t* __restrict__ d_in, BatchTables bt, XpsTables x)
{
	__shared__ __attribute__((aligned(16))) uint8_t s_in[2u * XPT_INB];
	const uint32_t lane = threadIdx.x;
	if (DEV && blockIdx.x >= x.cnt[1]) { return; }
	uint32_t b, k;
	xps_segment_of(x, xps_streams<DEV>(x), blockIdx.x, b, k);
	const uint32_t u = x.unit[b];
	XpsSeg* __restrict__ seg = xps_segs(x, b);
	const uint32_t nseg = (uint32_t)(x.seg_prefix[b + 1] - x.seg_prefix[b]);
	if (ROUND > 0 && (x.mode[b] != 1u || !seg[k].redo || seg[k - 1u].redo)) { return; }   // (mode 1: rounds still running.) Only the FIRST of a run of
	                                                                     // segments that do not hold walks: it starts from a segment that holds, and goes on below
	const uint32_t n = (uint32_t)bt.in_len[u];
	const uint8_t* src = d_in + bt.in_off[u];
	const uint32_t a0 = (uint32_t)((uintptr_t)src & 15u);
	const uint8_t* ab = src - a0;
	const uint32_t endq = a0 + n;
	uint32_t loaded; uint4 nxt;
	XptWalk W = { a0, 0, 0, 0, 0, false, -3, false };
	if (ROUND == 0 && k > 0) {
		W.ip = a0 + k * x.seg_bytes - x.warm_bytes;
		XPT_RING_START(W.ip)
		xpt_walk<false>(s_in, ab, endq, loaded, nxt, W, a0 + k * x.seg_bytes, ~(u64)0, nullptr, lane);
		if (!W.running) {                                                  // it fell over before the segment: nothing to offer
			if (lane == 0) { seg[k].l_ip = 0xFFFFFFFFu; seg[k].l_hp = 0; seg[k].e_ip = 0; seg[k].e_hp = 0; seg[k].kind = 2u; seg[k].ntok = 0; seg[k].nout = 0; seg[k].redo = 0; }
			return;
		}
		W.op = 0; W.tc = 0;
	} else if (ROUND > 0) {
		if (seg[k - 1u].kind != 0u) { if (lane == 0) { seg[k].kind = 2u; seg[k].redo = 0; seg[k].l_ip = 0xFFFFFFFFu; } return; }   // nothing to start from
		W.ip = seg[k - 1u].e_ip;
		const uint32_t hp = seg[k - 1u].e_hp;
		W.have_half = hp != 0xFFFFFFFFu; W.hp = W.have_half ? hp : 0u; W.half = W.have_half ? ab[hp] : 0u;
		XPT_RING_START(W.ip)
	} else { XPT_RING_START(a0) }
	for (;;) {
		const uint32_t lim = k + 1u == nseg ? 0xFFFFFFFFu : a0 + (k + 1u) * x.seg_bytes;
		const uint32_t l_ip = W.ip, l_hp = W.have_half ? W.hp : 0xFFFFFFFFu;
		xpt_walk<false>(s_in, ab, endq, loaded, nxt, W, lim, ~(u64)0, nullptr, lane);
		const uint32_t e_hp = W.have_half ? W.hp : 0xFFFFFFFFu;
		if (lane == 0) {
			seg[k].l_ip = l_ip; seg[k].l_hp = l_hp; seg[k].e_ip = W.ip; seg[k].e_hp = e_hp;
			seg[k].kind = W.running ? 0u : (W.status == 0 ? 1u : 2u); seg[k].ntok = W.tc; seg[k].nout = W.op; seg[k].redo = 0;
		}
		// a walk that comes from a segment that holds goes on through the segments behind it until it arrives where one of them had landed:
		// a stretch that no speculative walk entered costs one round, however many segments it spans
		if (ROUND == 0 || !W.running || k + 1u == nseg) { break; }
		if (seg[k + 1u].l_ip == W.ip && seg[k + 1u].l_hp == e_hp) { break; }
		++k; W.op = 0; W.tc = 0;
	}
}

// which segments hold; LAST: sums, verdict (mode 2 = done by segments, 0 = the one-wave walk takes the stream) and the caller's results
template <bool LAST, bool DEV>
__global__ __launch_bounds__(256) void xps_check_kernel(BatchTables bt, XpsTables x, u64* __restrict__ ntok, u64* __restrict__ d_out_len, int32_t* __restrict__ d_status)
{
	__shared__ uint32_t s_bad;
	__shared__ u64 s_t[4], s_o[4];
	if (DEV && blockIdx.x >= x.cnt[0]) { return; }
	const uint32_t tid = threadIdx.x, b = blockIdx.x, u = x.unit[b];
	XpsSeg* __restrict__ seg = xps_segs(x, b);
	const uint32_t nseg = (uint32_t)(x.seg_prefix[b + 1] - x.seg_prefix[b]);
	if (x.mode[b] != 1u) { return; }
	if (tid == 0) { s_bad = 0; }
	__syncthreads();
	uint32_t bad = 0;                                                    // 1: some segment has to be walked again; 2: no use
	for (uint32_t k = tid; k < nseg; k += 256u) {
		bool redo = false;
		if (k > 0) {
			const XpsSeg p = seg[k - 1u];
			if (p.kind != 0u) { bad |= 2u; }                               // the stream ends (well or not) before its last segment: not our case
			else if (seg[k].l_ip != p.e_ip || seg[k].l_hp != p.e_hp) { redo = true; bad |= 1u; }
		}
		if (k + 1u == nseg && seg[k].kind != 1u && !redo) { bad |= seg[k].kind == 2u ? 2u : 2u; }   // the last segment must end the stream, and well
		seg[k].redo = redo ? 1u : 0u;
	}
	if (bad) { atomicOr(&s_bad, bad); }
	__syncthreads();
	const uint32_t verdict = s_bad;
	if (!LAST) {
		if (tid == 0 && (verdict & 2u) && !(verdict & 1u)) { x.mode[b] = 0u; }   // (while segments are still being redone, a bad kind may be that of a wrong walk)
		return;
	}
	if (verdict) { if (tid == 0) { x.mode[b] = 0u; } return; }
	// all segments hold: where their tokens and bytes go
	u64 tcar = 0, ocar = 0;
	for (uint32_t k0 = 0; k0 < nseg; k0 += 256u) {
		const uint32_t k = k0 + tid;
		const u64 t = k < nseg ? seg[k].ntok : 0, o = k < nseg ? seg[k].nout : 0;
		u64 ti = t, oi = o;
		#pragma unroll
		for (uint32_t d = 1; d < 64u; d <<= 1) { const u64 a = __shfl_up(ti, d, 64), c = __shfl_up(oi, d, 64); if ((tid & 63u) >= d) { ti += a; oi += c; } }
		if ((tid & 63u) == 63u) { s_t[tid >> 6] = ti; s_o[tid >> 6] = oi; }
		__syncthreads();
		u64 tb = tcar, ob = ocar, tt = 0, ot = 0;
		for (uint32_t w = 0; w < 4u; ++w) { if (w < (tid >> 6)) { tb += s_t[w]; ob += s_o[w]; } tt += s_t[w]; ot += s_o[w]; }
		if (k < nseg) { seg[k].tbase = tb + ti - t; seg[k].obase = ob + oi - o; }
		tcar += tt; ocar += ot;
		__syncthreads();
	}
	if (tid == 0) {
		const bool fits = ocar <= bt.out_cap[u];                           // beyond the capacity: the one-wave walk says where and how
		x.mode[b] = fits ? 2u : 0u;
		if (fits) { d_status[u] = 0; d_out_len[u] = ocar; ntok[u] = tcar; x.done[u] = XPS_DONE; }
	}
}

// EMIT = false: the size query -- the same walk and tests, no token written (tok / tok_prefix unused)
template <bool EMIT, bool DEV>
__global__ __launch_bounds__(64) void xps_emit_kernel(const uint8_t* __restrict__ d_in, BatchTables bt, XpsTables x, const u64* __restrict__ tok_prefix, uint32_t* __restrict__ tok)
{
	__shared__ __attribute__((aligned(16))) uint8_t s_in[2u * XPT_INB];
	const uint32_t lane = threadIdx.x;
	if (DEV && blockIdx.x >= x.cnt[1]) { return; }
	uint32_t b, k;
	xps_segment_of(x, xps_streams<DEV>(x), blockIdx.x, b, k);
	if (x.mode[b] != 2u) { return; }
	const uint32_t u = x.unit[b];
	const XpsSeg* __restrict__ seg = xps_segs(x, b);
	const uint32_t nseg = (uint32_t)(x.seg_prefix[b + 1] - x.seg_prefix[b]);
	const uint32_t n = (uint32_t)bt.in_len[u];
	const uint8_t* src = d_in + bt.in_off[u];
	const uint32_t a0 = (uint32_t)((uintptr_t)src & 15u);
	const uint8_t* ab = src - a0;
	const uint32_t endq = a0 + n;
	const uint32_t lim = k + 1u == nseg ? 0xFFFFFFFFu : a0 + (k + 1u) * x.seg_bytes;
	uint32_t loaded; uint4 nxt;
	XptWalk W = { seg[k].l_ip, seg[k].obase, seg[k].tbase, 0, 0, false, -3, false };
	if (seg[k].l_hp != 0xFFFFFFFFu) { W.have_half = true; W.hp = seg[k].l_hp; W.half = ab[W.hp]; }
	XPT_RING_START(W.ip)
	xpt_walk<EMIT, true>(s_in, ab, endq, loaded, nxt, W, lim, bt.out_cap[u], EMIT ? tok + tok_prefix[u] : nullptr, lane);
	// the same walk as the one that was counted, now with the tests that need the output offset: anything else than the counted end is a failed test
	// (... including the pending length nibble the walk leaves with: it seeds the next segment's walk, and a record rewritten by a later round while
	// this segment was read could agree on everything else)
	const uint32_t e_hp = W.have_half ? W.hp : 0xFFFFFFFFu;
	const bool same = W.ip == seg[k].e_ip && W.tc == seg[k].tbase + seg[k].ntok && W.op == seg[k].obase + seg[k].nout && (W.running ? (seg[k].kind == 0u && e_hp == seg[k].e_hp) : (seg[k].kind == 1u && W.status == 0));
	if (!same && lane == 0) { x.done[u] = 0; }                            // the one-wave walk takes the stream after all
}

// ---- launchers of the token walks -------------------------------------------------------------------------------------------------------
void launch_xpt_parse(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const u64* tok_prefix, uint32_t* tok, u64* ntok, u64* d_out_len, int32_t* d_status, const XpsTables& x)
{
	if (bt.n_units) { hipLaunchKernelGGL(xpt_parse_kernel<true>, dim3(bt.n_units), dim3(64), 0, st, d_in, bt, tok_prefix, tok, ntok, d_out_len, d_status, (const uint32_t*)(x.n_big ? x.done : nullptr)); }
}
void launch_xpt_size(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, u64* ntok, u64* d_out_len, int32_t* d_status, const XpsTables& x)
{
	if (bt.n_units) { hipLaunchKernelGGL(xpt_parse_kernel<false>, dim3(bt.n_units), dim3(64), 0, st, d_in, bt, (const u64*)nullptr, (uint32_t*)nullptr, ntok, d_out_len, d_status, (const uint32_t*)(x.n_big ? x.done : nullptr)); }
}

// the segment kernels, when the plan has large streams (DEV: kernels.h XpsTables::cnt): speculative walks, one round of check + walk again, verdict + the emit walk
template <bool DEV>
static void xps_walk(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const XpsTables& x)
{
	if (DEV) { launch_dev_zero(st, x.done, bt.n_units); }             // (a kernel, not a memset: kernels.h launch_dev_zero)
	else { (void)hipMemsetAsync(x.done, 0, (size_t)bt.n_units * 4u, st); }
	hipLaunchKernelGGL(xps_init_kernel<DEV>, dim3((x.n_big + 255u) / 256u), dim3(256), 0, st, x);
	hipLaunchKernelGGL((xps_walk_kernel<0, DEV>), dim3(x.n_seg), dim3(64), 0, st, d_in, bt, x);
}
template <bool DEV>
static void xps_redo(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const XpsTables& x, u64* ntok, u64* d_out_len, int32_t* d_status)
{
	hipLaunchKernelGGL((xps_check_kernel<false, DEV>), dim3(x.n_big), dim3(256), 0, st, bt, x, ntok, d_out_len, d_status);
	hipLaunchKernelGGL((xps_walk_kernel<1, DEV>), dim3(x.n_seg), dim3(64), 0, st, d_in, bt, x);
}
template <bool DEV, bool EMIT>
static void xps_verdict(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const XpsTables& x, const u64* tok_prefix, uint32_t* tok, u64* ntok, u64* d_out_len, int32_t* d_status)
{
	hipLaunchKernelGGL((xps_check_kernel<true, DEV>), dim3(x.n_big), dim3(256), 0, st, bt, x, ntok, d_out_len, d_status);
	hipLaunchKernelGGL((xps_emit_kernel<EMIT, DEV>), dim3(x.n_seg), dim3(64), 0, st, d_in, bt, x, tok_prefix, tok);
}
void launch_xps_walk(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const XpsTables& x)
{
	if (bt.n_units && x.n_big) { (x.cnt ? xps_walk<true> : xps_walk<false>)(st, d_in, bt, x); }
}
void launch_xps_redo(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const XpsTables& x, u64* ntok, u64* d_out_len, int32_t* d_status)
{
	if (bt.n_units && x.n_big) { (x.cnt ? xps_redo<true> : xps_redo<false>)(st, d_in, bt, x, ntok, d_out_len, d_status); }
}
void launch_xps_emit(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const XpsTables& x, const u64* tok_prefix, uint32_t* tok, u64* ntok, u64* d_out_len, int32_t* d_status)
{
	if (bt.n_units && x.n_big) { (x.cnt ? xps_verdict<true, true> : xps_verdict<false, true>)(st, d_in, bt, x, tok_prefix, tok, ntok, d_out_len, d_status); }
}
void launch_xps_size(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const XpsTables& x, u64* ntok, u64* d_out_len, int32_t* d_status)
{
	if (bt.n_units && x.n_big) { (x.cnt ? xps_verdict<true, false> : xps_verdict<false, false>)(st, d_in, bt, x, nullptr, nullptr, ntok, d_out_len, d_status); }
}

} // namespace msc
