// lznt1.hip -- LZNT1 one-shot compression for gfx950 (MI355X), bit-exact with the reference CPU encoder.
//
// Replaces: lznt1_compress / lznt1_compress_chunk (/root/reference/src/lznt1_compress.cpp:233-273, :49-94) and
// LZNT1Dictionary::Fill/Find (/root/reference/include/mscomp/LZNT1Dictionary.h:93-106, :114-143).
//
// One wavefront (64-thread block) = one 4 KiB chunk, everything staged in LDS (20.2 KiB -> 7 chunks in flight per CU):
//   A. coalesced 16 B/lane load of the chunk into LDS;
//   B. dictionary = the reference's per-key position arrays as ONE position-sorted bucket array in LDS, built by a stable
//      counting sort on a 12-bit hash of the 3-byte key: histogram by LDS atomics, exclusive scan of the counts (DPP),
//      then an ORDERED scatter in 64 ascending batches (one LDS gather + scatter of the bucket cursors per batch,
//      intra-batch conflicts resolved with ballots). Afterwards cursor[h] = end of bucket h, so the candidates of a
//      position are simply the entries of its bucket that are smaller than the position itself;
//   C. window by window (64 positions, lane = position), LAZILY like the reference (Find runs only where the greedy parse
//      can start a token):
//        1. every lane at or after the parse position scans the 4 OLDEST candidates of its position itself (unconditional
//           loads in flight together, strictly-longer wins). Which bucket entries are candidates needs no count: the position is itself
//           an entry of its bucket, behind its older same-hash positions, so the candidates are the entries in front of the first one
//           that is not smaller than the position (a prefix-AND of ballots). The compares have two stages: the first 8 bytes always,
//           bytes 8..15 only if a candidate of some lane of the wave agreed on all 8 and max_len allows more;
//        2. the greedy walk runs on the scalar unit over ballot masks (s_ff1 over literal runs). When it lands on a
//           position with a candidate that matched 16 bytes (and max_len > 16), the whole wave extends those candidates,
//           256 bytes per step; when it lands on a position that still has unexamined candidates, the whole wave finishes
//           that ONE position: 64 candidates per step (the lanes in front of the position's own entry; the step that holds it is the
//           last), the same two stages. A step's candidates are younger than the best so far, and the older one wins on equal length, so
//           only the lanes whose candidate is strictly longer than the best (and at least 3 bytes long) can change it: one compare and a
//           ballot find them, and only a step that has such a lane reduces them, DPP max of (len, -position) = longest, oldest on ties
//           (three steps of four have none). Stop when max_len is reached. Positions covered by a match are never extended or finished;
//        3. tokens go straight to the chunk's scratch slot, placed by the closed form
//           pos(t) = (t div 8 + 1) + sum size(u<t)   (mbcnt prefix popcounts); flag bits collect in a 16-entry LDS ring;
//   D. header (0xB000|size-1), or the raw chunk (0x3000|n-1) when the running size reaches n; util.hip concatenates slots.
#include "common.h"
#include "kernels.h"
#include "host.h"

namespace msc {

#ifdef LZ_PROFILE   // dev-only phase timers (s_memtime cycles summed over blocks); not in the production build
__device__ unsigned long long g_lz_prof[16];
#define LZ_T(i) { const unsigned long long t_ = __builtin_readcyclecounter(); t_acc[i] += t_ - t_prev; t_prev = t_; }
#define LZ_T0   unsigned long long t_prev = __builtin_readcyclecounter(); unsigned long long t_acc[16] = {0};
#define LZ_CNT(i, v) { t_acc[i] += (unsigned long long)(v); }
#define LZ_TEND if (lane == 0) { for (int i_ = 0; i_ < 16; ++i_) { atomicAdd(&g_lz_prof[i_], t_acc[i_]); } }
#else
#define LZ_T(i)
#define LZ_T0
#define LZ_CNT(i, v)
#define LZ_TEND
#endif

#ifdef LZ4_PROFILE_EVENTS   // (the event counters below; they imply the phase timers)
#define LZ4_PROFILE
#endif
#ifdef LZ4_PROFILE   // dev-only: the four-wave kernel's phase cycles, per WAVE: slot [LZ4_NSLOT wv + i] is wave wv's time in phase i, kept in lane i of one
                     // vector register until the kernel's end (one atomic per slot and wave then). Even slots are work, the odd slot behind each is the
                     // idle time in front of the barrier that ends it: 0 load, 2 B1 rank, 4 B2 re-read + bucket sums, 6 B3 pack, 8 B4 scatter, 10 parse of the
                     // wave's segment + seam, 12 cascade check, 14 flag clear + scans, 16 token staging + emit loop, 18 flag bytes, header, size.
                     // With LZ4_PROFILE_EVENTS, summed over all windows walked, behind the phase slots: finishing steps [+0], lz_lcp_tail wave-iterations of the
                     // finishing steps [+1], long-pending stops [+2], cooperative 256-byte extension steps [+3].
                     // The event counters are same-address global atomics from inside the parse, some 300 per chunk: they hold up every global
                     // access of the kernel and inflate the phase cycles of load, parse and emit many times over, so the two are read in separate builds.
#define LZ4_NSLOT 20
#define LZ4_NEV   (4 * LZ4_NSLOT)
#define LZ4_NPROF (LZ4_NEV + 4)
__device__ unsigned long long g_lz4_prof[LZ4_NPROF];
#endif

#ifndef LZ_TBL_BITS
#define LZ_TBL_BITS 12   // bucket ends stay below 4096: twelve bits each (the four-wave kernel packs them after its sort)
#endif
#define LZ_TBL      (1u << LZ_TBL_BITS)
#ifndef LZ_SELF
#define LZ_SELF     4u       // candidates each lane scans by itself before the wave cooperates
#endif

// (never 0: bucket 0 stays empty, so "the end of the bucket before mine" is always cnt[h - 1] -- no special case in the parse.
// Keys that hash to 0 share bucket 1: a bucket may hold several keys anyway, the 3-byte compare sorts them out.)
__device__ __forceinline__ uint32_t lz_hash(uint32_t key24) { const uint32_t h = (key24 * 0x9E3779B1u) >> (32 - LZ_TBL_BITS); return h ? h : 1u; }

// position-dependent split of the 16-bit match token (lznt1_compress.cpp:51,66) -- pure function of pos
__device__ __forceinline__ uint32_t lz_shift(uint32_t pos)
{
	// = pos <= 16 ? 12 : 12 - (bits(pos - 1) - 4), as one unsigned minimum: clz(pos - 1) - 16 is >= 12 for pos <= 16 and wraps to a huge
	// value for pos <= 1 (v_ffbh_u32 gives -1 for 0)
	uint32_t z; asm("v_ffbh_u32 %0, %1" : "=v"(z) : "v"(pos - 1u));
	return (z - 16u) < 12u ? z - 16u : 12u;
}

// racing LDS accesses between lanes of one wave: relaxed wavefront-scope atomics (plain ds_read/ds_write in the ISA;
// DS operations of a wave execute in program order) so the compiler neither forwards nor reorders them.
__device__ __forceinline__ void     wst16(uint16_t* p, uint32_t v) { __hip_atomic_store(p, (uint16_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ uint16_t wld16(uint16_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void     wst32(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ uint32_t wld32(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void     wst8(uint8_t* p, uint32_t v) { __hip_atomic_store(p, (uint8_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void     wst64(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }
__device__ __forceinline__ void     wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront", "local"); }

// A bucket entry of the window's eager scan stays 16 bits wide: the compiler selects the relaxed-atomic load (wld16) as an any-extending one and
// puts an AND behind it wherever 32 zero-extended bits are asked for, although ds_read_u16 has zero-extended already. So nothing asks: the
// entry travels as a dword whose upper half is UNDEFINED to the compiler (lz_entry32), and each of its readers takes the low bits alone -- the
// "entry < position" compare selects the low word (SDWA, named here), the dword address is an AND with 0xFFC anyway, v_alignbyte_b32 reads
// bits [1:0] of its shift (common.h alignbyte_addr) and lz_key's v_bitop3_b32 bits [11:0]. (One reader that asks for the zero-extended value
// brings the AND back for all of them.)
typedef uint16_t lz_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t lz_entry32(uint16_t e) { lz_u16x2 v; v.x = e; return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ u64 lz_entry_below(uint32_t e, uint32_t p)   // the lanes whose entry is smaller than their p (< 65 536)
{
	u64 m; asm("v_cmp_gt_u32_sdwa %0, %1, %2 src0_sel:DWORD src1_sel:WORD_0" : "=s"(m) : "v"(p), "v"(e)); return m;
}
// 16 bytes at any byte offset of the chunk in LDS (common.h: lds_ld128), the offset taken modulo 4096: the AND that aligns the dword
// address also keeps it inside the chunk, so callers need no select for candidates that do not exist (they are masked afterwards).
__device__ __forceinline__ uint4 lz_ld128(const uint8_t* base, uint32_t off)
{
	const uint32_t* a = reinterpret_cast<const uint32_t*>(base + (off & 0xFFCu));
	const uint32_t w0 = a[0], w1 = a[1], w2 = a[2], w3 = a[3], w4 = a[4];
	return make_uint4(alignbyte_addr(w1, w0, off), alignbyte_addr(w2, w1, off), alignbyte_addr(w3, w2, off), alignbyte_addr(w4, w3, off));
}
// 4 bytes the same way (common.h: lds_ld32): the sort's read of a position's key
__device__ __forceinline__ uint32_t lz_ld32(const uint8_t* base, uint32_t off)
{
	const uint32_t* a = reinterpret_cast<const uint32_t*>(base + (off & 0xFFCu));
	return alignbyte_addr(a[1], a[0], off);
}
// The same for the sort's batches, position 64 b + lane: `a4` is the aligned dword that holds it, 64 b + (lane & ~3) -- one address per round of
// batches, the batch in the read's offset field -- and the lane number is the shift operand: v_alignbyte_b32 reads bits [1:0] of it alone, so no
// instruction puts the batch's base into it (the compiler cannot know: it made a v_or_b32 per batch)
__device__ __forceinline__ uint32_t lz_ld32_lane(const uint8_t* a4, uint32_t lane)
{
	const uint32_t* a = reinterpret_cast<const uint32_t*>(a4);
	return alignbyte_addr(a[1], a[0], lane);
}
// Common prefix beyond the first 16 (equal) bytes of d[q..] and d[p..]: 16 bytes per step; the result may exceed maxlen
// (callers clamp).
__device__ __forceinline__ uint32_t lz_lcp_tail(const uint8_t* d, uint32_t q, uint32_t p, uint32_t maxlen, uint32_t& it)
{
	uint32_t l = 16u;
	for (;;) {
		++it;
		uint4 a, b;
		a = lz_ld128(d, q + l); b = lz_ld128(d, p + l);
		const uint32_t f = first_nz_byte16(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
		l += f;
		if (f < 16u || l >= maxlen) { break; }
	}
	return l;
}
// The same with the whole wave, for ONE pair (q, p, l and maxlen wave-uniform, l < maxlen): lane i compares the dword at l + 4 i, 256 bytes
// per step, from two aligned reads per side and v_alignbyte (the byte shifts are uniform: 4 i keeps the low bits); the first mismatch is the
// ballot's lowest lane plus the first differing byte of its XOR. Offsets are taken modulo 4096 like lz_ld128's: what lies at or beyond
// p + maxlen <= n is clamped away. Returns min(common prefix, maxlen).
__device__ __forceinline__ uint32_t lz_lcp_wave(const uint8_t* d, uint32_t q, uint32_t p, uint32_t l, uint32_t maxlen, uint32_t lane, uint32_t& steps)
{
	const uint32_t shq = q + l, shp = p + l;                       // (as byte addresses: alignbyte_addr)
	for (;;) {
		const uint32_t oq = q + l + 4u * lane, op = p + l + 4u * lane;
		const uint32_t* const aq = reinterpret_cast<const uint32_t*>(d + (oq & 0xFFCu));
		const uint32_t* const ap = reinterpret_cast<const uint32_t*>(d + (op & 0xFFCu));
		const uint32_t x = alignbyte_addr(aq[1], aq[0], shq) ^ alignbyte_addr(ap[1], ap[0], shp);
		const u64 ne = __builtin_amdgcn_ballot_w64(x != 0u);
		++steps;
		if (ne) {
			const uint32_t i = ctz64(ne);
			l += 4u * i + ((uint32_t)__builtin_ctz((uint32_t)__builtin_amdgcn_readlane((int)x, (int)i)) >> 3);
			break;
		}
		l += 256u;
		if (l >= maxlen) { break; }
	}
	return l < maxlen ? l : maxlen;
}
// First difference of two 16-byte blocks given their XOR, as a BIT index limited to capbits (<= 128): common.h first_nz_byte16 without
// its final shift -- the limit (8 x min(max_len, 16)) rides in the minimum that finds the difference, so the byte count needs no clamp.
__device__ __forceinline__ uint32_t lz_diff_bits16(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t capbits)
{
	const uint32_t a = ffbl_raw(x1) | 32u, b = ffbl_raw(x2) | 64u, c = ffbl_raw(x3) | 96u;
	return min3u(min3u(ffbl_raw(x0), a, b), c, capbits);
}
// The FIRST STAGE of a candidate compare: the first LZ_S1 = 8 bytes, from three aligned dwords. Most candidates differ from the position inside
// them; bytes 8..15 and what follows are a second stage that the wave runs only when one of its candidates needs it. (A first stage of 12 bytes
// runs its second stage less often and still lost: round 13 in profiles/HISTORY.md.)
#define LZ_S1 8u
struct LzS1 { uint32_t x, y; };
__device__ __forceinline__ LzS1 lz_ld_s1(const uint8_t* base, uint32_t off)
{
	const uint32_t* a = reinterpret_cast<const uint32_t*>(base + (off & 0xFFCu));
	const uint32_t w0 = a[0], w1 = a[1], w2 = a[2];
	return LzS1{ alignbyte_addr(w1, w0, off), alignbyte_addr(w2, w1, off) };
}
// first difference as a BIT index limited to capbits (<= 64), given the XOR of the two sides (lz_diff_bits16's form)
__device__ __forceinline__ uint32_t lz_diff_bits_s1(uint32_t x0, uint32_t x1, uint32_t capbits)
{
	return min3u(ffbl_raw(x0), ffbl_raw(x1) | 32u, capbits);
}
// The SECOND STAGE: bytes 8..15 (the dwords behind the first stage's: a caller that has read those pays for two more)
struct LzS2 { uint32_t z, w; };
__device__ __forceinline__ LzS2 lz_ld_s2(const uint8_t* base, uint32_t off)
{
	const uint32_t* a = reinterpret_cast<const uint32_t*>(base + (off & 0xFFCu));
	const uint32_t w2 = a[2], w3 = a[3], w4 = a[4];
	return LzS2{ alignbyte_addr(w3, w2, off), alignbyte_addr(w4, w3, off) };
}
// first difference of bytes 8..15 as a bit index of the 16 bytes, limited to capbits (<= 128), for a pair whose first 8 bytes are equal
__device__ __forceinline__ uint32_t lz_diff_bits_s2(uint32_t xz, uint32_t xw, uint32_t capbits)
{
	return min3u(ffbl_raw(xz) | 64u, ffbl_raw(xw) | 96u, capbits);
}
// The key (len << 12) | (4095 - q) of a candidate q (< 4096) that agrees on `bits` bits: with t = bits << 9 and c = 0xFFF it is "c ? ~q : t", bit
// by bit -- ONE three-input boolean behind the shift (v_bitop3_b32). The low three bits of `bits` land below bit 12 and are selected away with
// the rest, so no AND rounds them off first; and nothing of q above bit 11 is read, so a bucket entry needs no zero-extension for it.
// (Named as an instruction: written as (t & ~c) | (~q & c) the compiler rounds t off with an AND of its own first. Truth table 0x74 = src1 ? ~src2 : src0.)
__device__ __forceinline__ uint32_t lz_key(uint32_t bits, uint32_t q)
{
	uint32_t r; asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x74" : "=v"(r) : "v"(bits << 9), "s"(0xFFFu), "v"(q)); return r;
}
// Bit i (< 64) of a wave-uniform mask as 0 / 1 in a scalar register: no 64-bit `1 << i`, and the asm keeps the test after the shift a 32-bit one
__device__ __forceinline__ uint32_t lz_bit64(u64 m, uint32_t i) { u64 t; asm("s_lshr_b64 %0, %1, %2" : "=s"(t) : "s"(m), "s"(i) : "scc"); return (uint32_t)t & 1u; }
// 8 len + 8 on the scalar unit in one instruction
__device__ __forceinline__ uint32_t lz_need_bits(uint32_t len) { uint32_t r; asm("s_lshl3_add_u32 %0, %1, 8" : "=s"(r) : "s"(len) : "scc"); return r; }
// One window (64 positions, lane = position) of the lazy parse of a chunk: Find for the positions at / after the parse
// position `entry` (the 4 oldest candidates per lane, the rest on demand), greedy walk, token mask. Returns the parse
// position after the window; key = (len << 12) | (4095 - q) of this lane's match (valid where matchmask is set),
// o0 = the 4 bytes at this lane's position, shift = its token split.
// A position needs the START of its bucket, the end of the bucket in front of it, from `tbl`: u16 per bucket (packed = false), or 12-bit fields,
// bucket h at bit 12 h (packed = true: the field at bit 12 (h - 1) lies inside the two dwords from (12 (h - 1)) / 32 on -- one read2 and one
// v_alignbit, which takes its shift modulo 32). The field of bucket 4094 ends in the last dword of the table: the dword after it is read and shifted out.
// FULL: the chunk has 4096 bytes (the four-wave kernel's full-chunk body; `n` is not read). Every window then has 64 positions, so the window's
// end, its length `wn` and the range mask need no minimum and no select; only window 0 has a position without a candidate (position 0) and only
// window 63 has lanes without a key (62 and 63: positions 4094 and 4095), each one scalar test.
struct LzWin { uint32_t key, o0, shift; u64 tokmask, matchmask; };
// INNER (with FULL only): the window is one of 1 to 62 of a full chunk. No position 0 and no lanes without a key, so the active lanes are those
// from the next token start on; and every position lies below 4078, where the chunk's end never cuts max_len and max_len is at least 18: the two
// compare stages stop at the literals 64 and 128 bits, and "max_len > 8" and "max_len > 16" hold in every lane, so their ballots are not taken.
// And it is none of the windows 1, 2, 4, 8, 16 and 32: all 64 lanes have one token split, made from the window's base on the scalar unit.
// (The first stage's literal cap is not applied either: see the argument at the place.)
template <bool packed, bool FULL = false, bool INNER = false>
__device__ __forceinline__ uint32_t lz_window(const uint8_t* s_data, const void* tbl, const uint16_t* s_bucket, uint32_t n, uint32_t lane,
                                              uint32_t wbase, uint32_t entry, LzWin& r)
{
	if (FULL) { n = 4096u; }
	entry = (uint32_t)__builtin_amdgcn_readfirstlane((int)entry); wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);   // (uniform: keeps the walk's bookkeeping on the scalar unit)
	const uint32_t wend = FULL ? wbase + 64u : ((wbase + 64u < n) ? wbase + 64u : n);
	const uint32_t p = wbase + lane;
	const LzS1 own = lz_ld_s1(s_data, p);                        // (aligned dword reads: a misaligned read is replayed; bytes 8..15 are read by a second stage)
	const uint32_t o0 = own.x, o1 = own.y;
	// (INNER: the split is the window's, not the lane's. lz_shift(p) is a function of the bit length of p - 1, which inside the window 64 w .. 64 w + 63
	// changes at lane 0 alone, and only where 64 w is a power of two: LZ4_WINDOW keeps windows 1, 2, 4, 8, 16 and 32 out of this copy, and in every
	// other interior window p - 1 is as long as wbase in all 64 lanes. wbase >= 192, so the count is at most 24 and the minimum with 12 never
	// wins. shift, max_len and max_len << 12 are scalar registers then: no lane computes them, and the event below reads no lane for max_len.)
	uint32_t shift;
	if (INNER) { shift = (uint32_t)__builtin_clz(wbase) - 16u; } else { shift = lz_shift(p); }
	const uint32_t mask3 = (1u << shift) + 2u;
	// my candidates: the entries from bucket[s] on that are < p (ascending). A position is ACTIVE if entry <= p, 0 < p and p + 3 <= n: ranges of the
	// window, so the mask of active lanes comes from the scalar unit, and it is applied once, to the candidates' existence below. Every lane looks
	// its bucket up, active or not (any 3 bytes hash to a bucket of the table), and an inactive lane's max_len is never used.
	uint32_t rel;                                                // the next token start, relative to the window (entry < wend here: < 64)
	asm("s_max_u32 %0, %1, %2\n\ts_sub_u32 %0, %0, %2" : "=&s"(rel) : "s"(entry), "s"(wbase) : "scc");   // (a saturating subtract would go to the vector unit)
	u64 act;
	static_assert(FULL || !INNER, "an interior window is a window of a full chunk");
	if (INNER) {
		act = sgpr64(~(u64)0 << rel);
	} else if (FULL) {
		uint32_t lo;                                               // position 0: window 0 alone. The OR itself sets the condition (left to the compiler a compare follows it)
		asm("s_or_b32 %0, %1, %2\n\ts_cselect_b32 %0, %2, 1" : "=&s"(lo) : "s"(wbase), "s"(rel) : "scc");
		const uint32_t top = wbase == 4032u ? 0x3FFFFFFFu : 0xFFFFFFFFu;   // lanes 62 and 63 of window 63 are no keys
		const u64 m = ~(u64)0 << lo;
		act = sgpr64(((u64)((uint32_t)(m >> 32) & top) << 32) | (uint32_t)m);
	} else {
		const uint32_t lo = (wbase == 0 && rel == 0) ? 1u : rel;
		const uint32_t hi = n > wbase + 2u ? (n - wbase - 2u < 64u ? n - wbase - 2u : 64u) : 0u;                      // lanes [lo, hi)
		act = sgpr64((~(u64)0 << lo) & (hi >= 64u ? ~(u64)0 : (((u64)1 << hi) - 1u)));
	}
	const uint32_t maxlen = INNER ? mask3 : (n - p < mask3) ? n - p : mask3;
	uint32_t s;
	{
		const uint32_t h = lz_hash(o0 & 0xFFFFFFu);              // >= 1
		if (packed) {                                          // bucket h starts at end[h-1]
			const uint32_t bit = h * 12u - 12u;
			const uint32_t* const t = static_cast<const uint32_t*>(tbl) + (bit >> 5);
			s = __builtin_amdgcn_alignbit(t[1], t[0], bit) & 0xFFFu;
		} else {
			s = static_cast<const uint16_t*>(tbl)[h - 1u];
		}
	}
	// 1. the oldest LZ_SELF candidates (LZNT1Dictionary.h:124-135: in order, strictly longer wins, stop at max_len). With
	// key = (len << 12) | (4095 - q) the reference's choice is simply the MAXIMUM of the candidates' keys: longest first,
	// then oldest (the candidates come oldest first, so "strictly longer" keeps the oldest of equals), and nothing can
	// beat a candidate that reached max_len. A key below 3 << 12 (hash collision) is "no match" to everything downstream.
	uint32_t key = 0;
	// All loads are UNCONDITIONAL so that they issue back to back and are waited for once: the five bucket entries from one
	// address, the candidates' bytes with the offset taken modulo 4096.
	// Which entries are candidates needs no count (the OWN-ENTRY rule): an active position has p + 3 <= n, so it is a key of the sort
	// and itself an entry of its bucket, behind its r older same-hash positions; entries ascend, so bucket[s + j] < p holds for
	// every j < r and fails at j = r. "Candidate j exists" is the prefix-AND over j' <= j of bucket[s + j'] < p, on the ballots.
	// What is read behind the own entry -- the next buckets' entries, the unused slots of a short chunk (leftovers of the sort's
	// count words) or the first words of the table behind the array -- may be smaller than p and is cut off by the prefix.
	// An inactive lane reads five entries of whatever bucket its bytes hash to: the mask of active lanes cuts them off.
	uint32_t q[LZ_SELF + 1u];                                 // (their upper halves are undefined: lz_entry32)
	u64 ex[LZ_SELF + 1u];                                     // lanes whose candidate j exists
	#pragma unroll
	// (five 2-byte reads, kept apart by the relaxed-atomic form: merged into an 8-byte + a 2-byte read, as the compiler does with plain loads, the 8-byte
	// one is only 2-byte aligned and is replayed -- SQ_LDS_UNALIGNED_STALL 14 % of the LDS pipe's busy cycles, 54.4 against 53.3 ms on configs[4])
	for (uint32_t j = 0; j <= LZ_SELF; ++j) { q[j] = lz_entry32(wld16(const_cast<uint16_t*>(s_bucket) + s + j)); }
	#pragma unroll
	for (uint32_t j = 0; j <= LZ_SELF; ++j) { ex[j] = (j ? ex[j - 1u] : act) & lz_entry_below(q[j], p); }
	// The compares stop at min(max_len, 16) bytes, in two stages: the first 8 bytes of the four candidates always; all 16 only if some lane of
	// the wave has an existing candidate that agreed on the whole first stage while its max_len allows more (one wave-uniform test; then every
	// lane compares bytes 8..15 of its four candidates). A candidate that reached 16 bytes with
	// max_len > 16 is extended only when the walk lands on its position (step 2), by the whole wave: inside a long repeat every lane has such
	// candidates, and the walk visits one or two of them.
	const uint32_t capb = INNER ? 128u : (maxlen < 16u ? maxlen : 16u) << 3, cap1 = INNER ? 8u * LZ_S1 : (maxlen < LZ_S1 ? maxlen : LZ_S1) << 3;
	uint32_t kk[LZ_SELF];                                     // candidate k's key, 0 if it does not exist; bit 16 (length 16): it reached 16 bytes
	{
		uint32_t lb[LZ_SELF];                                 // length in bits (the low three dropped below)
		{
			LzS1 c[LZ_SELF];                                  // (all loads in flight together)
			#pragma unroll
			for (uint32_t k = 0; k < LZ_SELF; ++k) { c[k] = lz_ld_s1(s_data, q[k]); }
			#pragma unroll
			for (uint32_t k = 0; k < LZ_SELF; ++k) {
				// INNER: no cap. What it kept out is a value above 64 (v_ffbl_b32 of 0 is -1), and none reaches lz_key: a lane whose candidate exists and
				// agreed on all 64 bits makes `more` non-zero, `more` alone decides the second stage here, and inside it every lane with lb >= 64,
				// its candidate existing or not, takes l2, which capb caps; where the second stage does not run, only candidates that do not exist
				// can hold such a value, and their key is 0 by the select on ex[k] below, whatever lb says. (Elsewhere a lane with max_len <= 8
				// relies on the cap: its candidate of 64 equal bits is not looked at again.)
				const uint32_t x0 = c[k].x ^ o0, x1 = c[k].y ^ o1;
				if (INNER) { const uint32_t a = ffbl_raw(x0), b = ffbl_raw(x1) | 32u; lb[k] = a < b ? a : b; } else { lb[k] = lz_diff_bits_s1(x0, x1, cap1); }
			}
		}
		u64 more = 0;
		#pragma unroll
		for (uint32_t k = 0; k < LZ_SELF; ++k) { more |= __builtin_amdgcn_ballot_w64(lb[k] >= 8u * LZ_S1) & ex[k]; }
		if (INNER ? more : more & __builtin_amdgcn_ballot_w64(maxlen > LZ_S1)) {
			const LzS2 a = lz_ld_s2(s_data, p);
			LzS2 c[LZ_SELF];
			#pragma unroll
			for (uint32_t k = 0; k < LZ_SELF; ++k) { c[k] = lz_ld_s2(s_data, q[k]); }
			#pragma unroll
			for (uint32_t k = 0; k < LZ_SELF; ++k) {                     // (a candidate that stopped inside the first stage keeps its bits)
				const uint32_t l2 = lz_diff_bits_s2(c[k].z ^ a.z, c[k].w ^ a.w, capb);
				lb[k] = lb[k] >= 8u * LZ_S1 ? l2 : lb[k];
			}
		}
		#pragma unroll
		for (uint32_t k = 0; k < LZ_SELF; ++k) {
			asm("v_cndmask_b32 %0, 0, %1, %2" : "=v"(kk[k]) : "v"(lz_key(lb[k], q[k])), "s"(ex[k]));
			key = kk[k] > key ? kk[k] : key;
		}
	}
	// 2. greedy walk; unresolved positions (a fifth older candidate exists and max_len was not reached) are finished by the whole wave
	// when (and only when) the walk lands on them, and so are the long-pending ones (a candidate reached 16 bytes, max_len > 16: the
	// key is provisional), whose candidates are extended first. (The masks are built from ballots of single compares, combined on the
	// scalar unit: the ballot of a combined condition costs two more vector instructions. len <= maxlen, so "not reached" is
	// key < maxlen << 12; a long-pending lane's provisional key never reaches it.)
	const u64 five = ex[LZ_SELF];
	u64 un = five & __builtin_amdgcn_ballot_w64(key < (maxlen << 12));
	// (which candidates reached 16 bytes stays in the lanes, as bit 16 of the four keys -- a compare stops at 16 bytes, so the bit is "length 16", and
	// the key of a candidate that does not exist is 0: as four 64-bit masks they were eight scalar registers held across the walk for its rarest stop.
	// The best key has the bit iff one of the four has it.)
	const u64 lp = sgpr64(INNER ? __builtin_amdgcn_ballot_w64(key >= (16u << 12)) : __builtin_amdgcn_ballot_w64(key >= (16u << 12)) & __builtin_amdgcn_ballot_w64(maxlen > 16u));
	u64 mm = __builtin_amdgcn_ballot_w64(key >= (3u << 12)) & ~un;              // resolved or long-pending positions that have a match
	// The serial loop only decides which candidates are TAKEN; everything else (which positions are literal tokens)
	// is derived in parallel afterwards.
	u64 matchmask = 0;
	const uint32_t wn = FULL ? 64u : (uint32_t)__builtin_amdgcn_readfirstlane((int)(wend - wbase));
	// Every resolved match lane precomputes where the walk goes after taking it: the first stop (match, unresolved or long-pending
	// position) at or after its end, relative to the window (>= wn leaves it). The scalar walk is then one v_readlane per taken
	// match; it leaves the asm block on an unresolved or long-pending position (st = 1), which the whole wave resolves. Stops are
	// only ever removed at the walk's own position, so the table never goes stale ahead.
	un = sgpr64(un); mm = sgpr64(mm);
	const u64 pend = sgpr64(un | lp);
	// (a target at or beyond wn only has to be >= wn: the walk ends there and the position after the window comes from the
	// match ends below. So no guard for nx >= 64: the shift count wraps, and nx + anything is already >= 64 >= wn.)
	const uint32_t nx = lane + (key >> 12);
	const u64 restl = (un | mm) >> (nx & 63u);
	const uint32_t zl = min3u(ffbl_raw((uint32_t)restl), ffbl_raw((uint32_t)(restl >> 32)) | 32u, 64u);   // 64 = no stop left
	const uint32_t J = (nx + zl < wn) ? nx + zl : wn;
	uint32_t mp;
	{
		// first stop at or after the next token start, on the scalar unit: the asm output pins the chain there
		u64 rest; asm("s_lshr_b64 %0, %1, %2" : "=s"(rest) : "s"(un | mm), "s"(rel) : "scc");
		mp = rest ? rel + ctz64(rest) : wn;
	}
	// The loop has ONE exit, at its bottom, and the event is a plain `if` inside it: the finishing step holds a divergent branch, so this region's
	// control flow is structurized, and every `break` of a uniform loop becomes a 64-bit flag that is set, selected, ANDed with exec and branched on
	// (four scalar instructions for each; `asm goto`, which would make the stop a branch target, is dropped by this compiler's back end without a
	// word). Conditions that cross a join are kept as 32-bit scalars, pinned by an empty asm, for the same reason.
	if (mp < wn) do {
		// v_readlane needs 4 wait states after the write of its lane select (mp): on the loop edge the five scalar
		// instructions in between provide them, on entry the s_nop does. The walk leaves on a stop that is pending (mp < wn), which the
		// whole wave resolves, or behind the window (mp >= wn): no flag, mp tells.
#define LZ_WALK(WN_) \
			"s_nop 3\n\t" \
			"1:\n\t" \
			"s_bitcmp1_b64 %[pend], %[mp]\n\t" \
			"s_cbranch_scc1 3f\n\t" \
			"s_bitset1_b64 %[mk], %[mp]\n\t" \
			"v_readlane_b32 %[mp], %[J], %[mp]\n\t" \
			"s_cmp_lt_u32 %[mp], " WN_ "\n\t" \
			"s_cbranch_scc1 1b\n\t" \
			"3:\n\t"
		if (FULL) {                                                // (the window's length is the inline constant 64: no register holds it across the walk)
			asm volatile(LZ_WALK("64") : [mp] "+s"(mp), [mk] "+s"(matchmask) : [pend] "s"(pend), [J] "v"(J) : "scc");
		} else {
			asm volatile(LZ_WALK("%[wn]") : [mp] "+s"(mp), [mk] "+s"(matchmask) : [pend] "s"(pend), [wn] "s"(wn), [J] "v"(J) : "scc");
		}
#undef LZ_WALK
		if (mp < wn) {
			const uint32_t sL = (uint32_t)__builtin_amdgcn_readlane((int)s, (int)mp);
			const uint32_t maxL = INNER ? maxlen : (uint32_t)__builtin_amdgcn_readlane((int)maxlen, (int)mp);   // (INNER: the window's, a scalar already)
			const uint32_t pL = wbase + mp;
			uint32_t kbest = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)mp);
			uint32_t fin = 1u;                                         // (a stop that is not long-pending is unresolved)
			if (lz_bit64(lp, mp)) {
				// long-pending: extend its candidates that reached 16 bytes, oldest first, with the whole wave; the first one that reaches
				// max_len cannot be beaten (an older one would have to be longer). Then it is unresolved only if a fifth candidate exists
				// and max_len was not reached.
				const uint32_t qv = s_bucket[sL + lane % LZ_SELF];           // (its first LZ_SELF entries: the candidates above)
				uint32_t nst = 0;
				#pragma unroll
				for (uint32_t k = 0; k < LZ_SELF; ++k) {
					if ((uint32_t)__builtin_amdgcn_readlane((int)kk[k], (int)mp) >> 16) {
						const uint32_t qk = (uint32_t)__builtin_amdgcn_readlane((int)qv, (int)k);
						const uint32_t l = lz_lcp_wave(s_data, qk, pL, 16u, maxL, lane, nst);
						const uint32_t kk = (l << 12) | (qk ^ 4095u);
						kbest = kk > kbest ? kk : kbest;
						if (l == maxL) { break; }
					}
				}
				fin = kbest < (maxL << 12) ? lz_bit64(un, mp) : 0u;    // (un's bit: the provisional key is below max_len, so it is `five`'s)
#ifdef LZ4_PROFILE_EVENTS
				if (lane == 0) { atomicAdd(&g_lz4_prof[LZ4_NEV + 2], 1ull); atomicAdd(&g_lz4_prof[LZ4_NEV + 3], (unsigned long long)nst); }
#endif
			}
			asm volatile("" : "+s"(fin));
			if (fin) {
				// finish position wbase+mp: the candidates after the first LZ_SELF of its bucket, oldest first, 64 per step
				// (the own-entry rule again: the candidates of a step are the lanes below the first entry that is not < pL, and the step that holds
				// pL's own entry is the last. fin implies a fifth candidate, so the own entry lies at or behind `base`, inside the array.)
				// Two stages: every step compares the first 8 bytes; bytes 8..15 and the tail beyond 16 only in a step in which a candidate
				// agreed on all of them (a step holds few candidates that do: tools/dev/lz_stage_study.c).
				const uint32_t a0 = (uint32_t)__builtin_amdgcn_readlane((int)o0, (int)mp), a1 = (uint32_t)__builtin_amdgcn_readlane((int)o1, (int)mp);
#ifdef LZ4_PROFILE_EVENTS
				uint32_t nsteps = 0, ntail = 0;
#endif
				const uint32_t cap1L = (maxL < LZ_S1 ? maxL : LZ_S1) << 3;   // (not read by the INNER copy: see the step's first stage below)
				// The step's candidates are younger than the best's, and the older one wins on equal length: only a candidate STRICTLY longer than the
				// best (and at least 3 bytes long: a best below 3 is "no match" downstream, which sub-3 key it holds is never read) can change kbest.
				// `need` is that length in bits, a function of kbest: computed here and again only behind a winner.
				// (kbest >> 12) < maxL here, so need <= 8 maxL: a candidate that reached max_len always wins.
				uint32_t need = kbest >> 12; need = lz_need_bits(need > 2u ? need : 2u);
				uint32_t base = sL + LZ_SELF;
				u64 go;                                                // all-ones: another step
				do {
					const uint32_t qq = s_bucket[base + lane];         // unconditional load (past the array's end it reads the table: behind the own entry)
					const u64 lt = __builtin_amdgcn_ballot_w64(qq < pL);
					const u64 vmask = lt & ~(lt + 1u);                 // the lanes below the first one at or beyond pL's own entry
					const LzS1 c1 = lz_ld_s1(s_data, qq);
					// (INNER: no cap, as in the window's first stage and for its reason: a lane of vmask that agreed on all 64 bits starts the second
					// stage, where every lane with l2 >= 64 takes l3; where it does not run, only lanes outside vmask can hold more than 64, and `win`
					// never has them. With the literal 64 as the cap the compiler makes two v_min_u32 of the v_min3_u32.)
					uint32_t l2;                                       // in bits
					if (INNER) { const uint32_t f0 = ffbl_raw(c1.x ^ a0), f1 = ffbl_raw(c1.y ^ a1) | 32u; l2 = f0 < f1 ? f0 : f1; } else { l2 = lz_diff_bits_s1(c1.x ^ a0, c1.y ^ a1, cap1L); }
					uint32_t it = 0;
					// (no test of max_len > 8 in front of the second stage: l2 is capped at 8 min(max_len, 8), so below 8 no candidate reaches 64 bits, and
					// at exactly 8 the second stage's cap is 64 too and it hands every candidate the 64 it came with. A max_len below 9 exists only in the last
					// 8 bytes of a chunk; the test was three scalar instructions of every step.)
					if (__builtin_amdgcn_ballot_w64(l2 >= 8u * LZ_S1) & vmask) {
						// (a candidate that stopped inside the first stage keeps its bits)
						// (max_len is read afresh here, which the empty asm enforces: hoisted out of the loop, "max_len > 16" becomes a 64-bit mask that
						// lives across it and the second stage's cap another register -- see the note on blocks per CU at lznt1_chunk4_kernel)
						uint32_t mL = maxL; asm volatile("" : "+s"(mL));
						const LzS2 a = lz_ld_s2(s_data, pL), c = lz_ld_s2(s_data, qq);
						const uint32_t l3 = lz_diff_bits_s2(c.z ^ a.z, c.w ^ a.w, (mL < 16u ? mL : 16u) << 3);
						l2 = l2 >= 8u * LZ_S1 ? l3 : l2;
						if (mL > 16u && l2 >= 128u && __builtin_amdgcn_inverse_ballot_w64(vmask)) { const uint32_t l = lz_lcp_tail(s_data, qq, pL, maxL, it); l2 = (l < maxL ? l : maxL) << 3; }
					}
					// One compare and a ballot find the winners; in three steps of four there are none and nothing is reduced (tools/dev/lz_best_study.c).
					go = lt;                                           // (some entry not < pL: all older candidates seen)
					const u64 win = __builtin_amdgcn_ballot_w64(l2 >= need) & vmask;
					if (win) {
						// longest, then oldest (older entries hold the larger 4095 - q); every winner's key is above the old kbest
						uint32_t k2; asm("v_cndmask_b32 %0, 0, %1, %2" : "=v"(k2) : "v"(lz_key(l2, qq)), "s"(win));
						kbest = wave_max_u32(k2);
						const uint32_t len = kbest >> 12;               // >= 3
						need = lz_need_bits(len);
						go = len == maxL ? (u64)0 : go;                // max_len reached: nothing can beat it
					}
#ifdef LZ4_PROFILE_EVENTS
					++nsteps; ntail += wave_max_u32(it);
#endif
					base += 64u;
					asm volatile("" : "+s"(go));                       // (one 64-bit compare and one branch: left to itself the compiler rebuilds the two conditions as flags)
				} while (go == ~(u64)0);
#ifdef LZ4_PROFILE_EVENTS
				if (lane == 0) { atomicAdd(&g_lz4_prof[LZ4_NEV], (unsigned long long)nsteps); atomicAdd(&g_lz4_prof[LZ4_NEV + 1], (unsigned long long)ntail); }
#endif
			}
			// mp is resolved now, and the literals before it are settled: clear its bit of `un`, write its key back (v_writelane takes its lane from m0 where
			// the value comes from a scalar register too), take its match or step over it as a literal, and go to the first stop at or after the
			// next token start. A next start at or beyond wn needs no guard: the shift count wraps, s_ff1 of zero is -1, and whatever (0 .. 64) is
			// added to it, mp stays >= wn, which is all the loop asks.
			{
				uint32_t t; u64 rs;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"      // (m0 is a reserved register to the compiler, which uses it nowhere in these kernels)
				asm volatile(
					"s_bitset0_b64 %[un], %[mp]\n\t"
					"s_mov_b32 m0, %[mp]\n\t"
					"s_lshr_b32 %[t], %[kb], 12\n\t"
					"s_cmp_gt_u32 %[t], 2\n\t"
					"s_cselect_b32 %[t], %[t], 1\n\t"
					"s_cbranch_scc0 5f\n\t"
					"s_bitset1_b64 %[mk], %[mp]\n\t"
					"5:\n\t"
					"v_writelane_b32 %[key], %[kb], m0\n\t"
					"s_add_u32 %[mp], %[mp], %[t]\n\t"
					"s_or_b64 %[rs], %[un], %[mm]\n\t"
					"s_lshr_b64 %[rs], %[rs], %[mp]\n\t"
					"s_ff1_i32_b64 %[t], %[rs]\n\t"
					"s_min_u32 %[t], %[t], 64\n\t"
					"s_add_u32 %[mp], %[mp], %[t]\n\t"
					: [un] "+s"(un), [mk] "+s"(matchmask), [mp] "+s"(mp), [key] "+v"(key), [t] "=&s"(t), [rs] "=&s"(rs)
					: [kb] "s"(kbest), [mm] "s"(mm)
					: "scc", "m0");
#pragma clang diagnostic pop
			}
		}
	} while (mp < wn);
	// tokens of the window = positions >= entry that no taken match covers: covered <=> the furthest end of the taken
	// matches starting at or before me lies beyond me and I am not such a start myself
	matchmask = sgpr64(matchmask);
	uint32_t mend; asm("v_cndmask_b32 %0, 0, %1, %2" : "=v"(mend) : "v"(p + (key >> 12)), "s"(matchmask));   // the mask itself selects: no per-lane bit test
	const uint32_t reach = wave_incl_scan_max(mend);
	const u64 range = FULL ? ~(u64)0 << rel : (~(u64)0 << rel) & (wn >= 64u ? ~(u64)0 : (((u64)1 << wn) - 1u));     // entry <= p < wend, on the scalar unit
	const u64 tokmask = range & (matchmask | __builtin_amdgcn_ballot_w64(reach <= p));
	const uint32_t wreach = (uint32_t)__builtin_amdgcn_readlane((int)reach, 63);
	const uint32_t cur = wreach > wend ? wreach : wend;

	r.key = key; r.o0 = o0; r.shift = shift; r.tokmask = tokmask; r.matchmask = matchmask;
	return cur;
}

// One returning LDS atomic for the 64 positions of a batch; `serial`: the same, one lane at a time in lane order (kernels.h: a device whose
// same-address atomics are not served in lane order -- DS operations of a wave execute in program order)
template <bool serial>
__device__ __forceinline__ uint32_t lz_ordered_add(uint32_t* addr, uint32_t v, bool active, uint32_t lane)
{
	uint32_t old = 0;
	if (!serial) { if (active) { old = __hip_atomic_fetch_add(addr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); } }
	else { for (uint32_t l = 0; l < 64u; ++l) { if (lane == l && active) { old = __hip_atomic_fetch_add(addr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); } wave_fence(); } }
	return old;
}

// DEV (compress plans with device tables): the grid is the plan's bound of chunks, and the blocks past the batch's real count return at once
// with a size of 0 (what scan_sizes reads for them); host plans run the <.., false> instances
template <bool serial, bool DEV = false>    // (a template, not an argument: the default kernels are the code they were)
__global__ __launch_bounds__(64) void lznt1_chunk_kernel(const uint8_t* __restrict__ d_in, BatchTables bt,
                                                        uint8_t* __restrict__ slots, uint32_t* __restrict__ slot_size)
{
	// ONE LDS object, the chunk FIRST: its 16-byte reads then need no address arithmetic beyond the AND that aligns them (the DS offset
	// fields reach 1 KiB / 64 KiB from the register address), and the bucket array is followed by the count table (lz_window reads up to
	// four entries past its own entry in the bucket array)
	struct __attribute__((aligned(16))) Lds {
		uint8_t  data[4096 + 32];
		uint16_t bucket[4096];      // positions sorted by (hash, position)
		uint16_t cnt[LZ_TBL];       // counts -> bucket ends
		uint32_t flagacc[16];       // flag bits of the groups in flight
		uint32_t flagpos[16];       // their byte position in the image
	};
	__shared__ Lds L;
	uint8_t* const s_data = L.data; uint16_t* const s_cnt = L.cnt; uint16_t* const s_bucket = L.bucket;
	uint32_t* const s_flagacc = L.flagacc; uint32_t* const s_flagpos = L.flagpos;

	const uint32_t lane = threadIdx.x;
	const uint32_t c = blockIdx.x;
	if (DEV && past_real_chunks(bt, c)) { if (lane == 0) { slot_size[c] = 0; } return; }
	const uint32_t u = unit_of_chunk(bt.chunk_prefix, bt.n_units, c);
	const u64 coff = (u64)(c - bt.chunk_prefix[u]) * 4096u;
	const u64 left = bt.in_len[u] - coff;
	const uint32_t n = left < 4096u ? (uint32_t)left : 4096u;
	const uint8_t* __restrict__ src = d_in + bt.in_off[u] + coff;
	uint8_t* __restrict__ img = slots + (u64)c * LZNT1_SLOT;              // chunk image: 2-byte header + payload

	LZ_T0
	// ---- A. stage the chunk, clear the count table -----------------------------------------------------------
	{
		const uint32_t nvec = (((uintptr_t)src & 15u) == 0) ? (n & ~15u) : 0u;
		for (uint32_t i = lane * 16u; i < nvec; i += 1024u) {
			*reinterpret_cast<uint4*>(s_data + i) = *reinterpret_cast<const uint4*>(src + i);
		}
		for (uint32_t i = nvec + lane; i < n; i += 64u) { s_data[i] = src[i]; }
		for (uint32_t i = n + lane; i < 4096u + 32u; i += 64u) { s_data[i] = 0; }
		for (uint32_t i = lane * 8u; i < LZ_TBL; i += 512u) { *reinterpret_cast<uint4*>(s_cnt + i) = make_uint4(0, 0, 0, 0); }
		if (lane < 16u) { s_flagacc[lane] = 0; }
	}
	__syncthreads();
	LZ_T(0)

	// ---- B1. histogram of the position hashes (two u16 counters per dword); the value each atomic RETURNS is the
	// position's rank inside its bucket: batches are issued in ascending position order, and within one DS instruction
	// the LDS unit serialises same-address atomics in lane order (gfx950 behaviour, checked by tools/dev/lds_order_test.hip
	// and, indirectly, by every parity test: a different order would change which candidate wins a tie) ------------------
	const uint32_t nb = (n + 63u) >> 6;
	uint32_t rk[32];                                             // ranks of my 64 positions, two per register
	#pragma unroll
	for (uint32_t b = 0; b < 64u; ++b) {
		uint32_t r = 0;
		if (b < nb) {
			const uint32_t p = b * 64u + lane;
			{
				const bool act = p + 2u < n;
				const uint32_t h = lz_hash(ld32(s_data + (act ? p : 0u)) & 0xFFFFFFu);
				const uint32_t old = lz_ordered_add<serial>(reinterpret_cast<uint32_t*>(s_cnt) + (h >> 1), (h & 1u) ? 0x10000u : 1u, act, lane);
				r = act ? ((h & 1u) ? old >> 16 : old & 0xFFFFu) : 0u;
			}
		}
		rk[b >> 1] = (b & 1u) ? (rk[b >> 1] | (r << 16)) : r;
	}
	__syncthreads();
	LZ_T(1)
	// ---- B2. inclusive scan of the 4096 counts -> bucket ENDS (bucket h = [end[h-1], end[h])): coalesced rounds of 8
	// bins per lane -----------------------------------------------------------------------------------------------------
	{
		uint32_t run = 0;
		for (uint32_t k = 0; k < LZ_TBL / 512u; ++k) {
			uint4 a = reinterpret_cast<uint4*>(s_cnt)[k * 64u + lane];
			uint32_t w[4] = { a.x, a.y, a.z, a.w };
			uint32_t sum = 0;
			#pragma unroll
			for (int i = 0; i < 4; ++i) { sum += (w[i] & 0xFFFFu) + (w[i] >> 16); }
			const uint32_t incl = wave_incl_scan_add_u32(sum);
			uint32_t r = run + incl - sum;
			#pragma unroll
			for (int i = 0; i < 4; ++i) { const uint32_t lo = w[i] & 0xFFFFu, hi = w[i] >> 16; w[i] = (r + lo) | ((r + lo + hi) << 16); r += lo + hi; }
			reinterpret_cast<uint4*>(s_cnt)[k * 64u + lane] = make_uint4(w[0], w[1], w[2], w[3]);
			run += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
		}
	}
	__syncthreads();
	// ---- B3. scatter: bucket[start[h] + rank] = p (positions of a bucket end up in ascending order) --------------------
	#pragma unroll
	for (uint32_t b = 0; b < 64u; ++b) {
		if (b < nb) {
			const uint32_t p = b * 64u + lane;
			if (p + 2u < n) {
				const uint32_t h = lz_hash(ld32(s_data + p) & 0xFFFFFFu);
				const uint32_t start = s_cnt[h - 1u];                  // (h >= 1)
				const uint32_t r = (b & 1u) ? rk[b >> 1] >> 16 : rk[b >> 1] & 0xFFFFu;
				s_bucket[start + r] = (uint16_t)p;
			}
		}
	}
	__syncthreads();
	LZ_T(2)

	// ---- C. lazy windows: Find -> greedy walk (finishing positions on demand) -> emit --------------------------------
	uint32_t entry = 0, T = 0, S = 0;                            // next token start, tokens so far, sum of token sizes so far
	bool raw = false;
	const uint32_t nw = (n + 63u) >> 6;
	for (uint32_t w = 0; w < nw; ++w) {
		const uint32_t wbase = w * 64u;
		const uint32_t wend = (wbase + 64u < n) ? wbase + 64u : n;
		if (entry >= wend) { continue; }                         // window wholly covered by a match
		LzWin r;
		const uint32_t cur = lz_window<false>(s_data, s_cnt, s_bucket, n, lane, wbase, entry, r);
		const uint32_t p = wbase + lane;
		const uint32_t key = r.key, o0 = r.o0, shift = r.shift;
		const u64 tokmask = r.tokmask, matchmask = r.matchmask;
		const bool is_m = (matchmask >> lane) & (u64)1, is_tok = (tokmask >> lane) & (u64)1;
		entry = cur;
		LZ_T(4)

		// 3. emit: pos(t) = 2 (header) + (t div 8 + 1) + sum size(u<t)
		const uint32_t tb = popc_below(tokmask), mbl = popc_below(matchmask);
		const uint32_t t = T + tb;
		const uint32_t pos = 3u + (t >> 3) + S + tb + mbl;
		if (is_tok) {
			if ((t & 7u) == 0) { wst32(&s_flagpos[(t >> 3) & 15u], pos - 1u); }
			if (is_m) {
				const uint32_t best = key >> 12;
				const uint32_t tok = ((p - (4095u - (key & 0xFFFu)) - 1u) << shift) | (best - 3u);
				img[pos] = (uint8_t)tok; img[pos + 1u] = (uint8_t)(tok >> 8);
			} else { img[pos] = (uint8_t)o0; }
		}
		if (is_m) { atomicOr(&s_flagacc[(t >> 3) & 15u], 1u << (t & 7u)); }
		wave_fence();
		const uint32_t nt = (uint32_t)__popcll(tokmask), nm = (uint32_t)__popcll(matchmask);
		// groups completed in this window: their flag byte is final
		if (is_tok && (t & 7u) == 7u) {
			const uint32_t g = (t >> 3) & 15u;
			img[wld32(&s_flagpos[g])] = (uint8_t)wld32(&s_flagacc[g]);
			wst32(&s_flagacc[g], 0u);
		}
		wave_fence();
		T += nt; S += nt + nm;
		LZ_T(5)
		if (((T + 7u) >> 3) + S >= n) { raw = true; break; }    // running size reached n (:85-86) => store raw
	}

	// ---- D. header / raw chunk -----------------------------------------------------------------------------------------
	const uint32_t csize = ((T + 7u) >> 3) + S;
	uint32_t total;
	if (!raw && csize < n) {
		if (lane == 0) {
			if (T & 7u) { const uint32_t g = (T >> 3) & 15u; img[s_flagpos[g]] = (uint8_t)s_flagacc[g]; }   // the last, partial group
			img[0] = (uint8_t)(0xB000u | (csize - 1u)); img[1] = (uint8_t)((0xB000u | (csize - 1u)) >> 8);
		}
		total = 2u + csize;
	} else {
		const uint32_t hdr = 0x3000u | (n - 1u);
		for (uint32_t k = lane; k < (n + 2u + 3u) / 4u; k += 64u) {
			reinterpret_cast<uint32_t*>(img)[k] = (k == 0) ? (hdr | (ld16(s_data) << 16)) : ld32(s_data + 4u * k - 2u);
		}
		total = 2u + n;
	}
	if (lane == 0) { slot_size[c] = total; }
	LZ_T(6)
	LZ_TEND
}
#ifdef LZ_PROFILE
extern "C" void mscomp_amd_debug_lz_prof(unsigned long long* out, int reset)
{
	(void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lz_prof), sizeof(unsigned long long) * 16);
	if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_lz_prof), z, sizeof z); }
}
#endif

// ===================================================================================================================
// Four waves per chunk (same bytes as the kernel above)
// ===================================================================================================================
// The sort (B) ranks the positions with one returning atomic each, like the kernel above, on three waves at once: the rank
// trick needs the positions in order only inside a wave's own part of the chunk, every part counts in a field of its own
// of a bucket's word, and the counts of the parts in front are added afterwards (section B below). The lazy parse (C), most
// of the time, is split: the parse's only state is the position of the next token, so wave j parses the windows
// [16 j, 16 j + 16) SPECULATIVELY as if a token started at position 1024 j, records per window the token mask, the match
// mask, the 16-bit match tokens (a match token depends on its position only) and the parse position after it; then wave
// j repairs the seam BEHIND its segment (it continues with its true position into segment j+1 until the position after
// a window equals the recorded one), wave 0 checks that no repair ran through a whole segment (else it cascades,
// serially), scans tokens / bytes per window, and the four waves emit their segments at known offsets; the flag bytes
// are OR-ed into a per-group LDS array and stored at the end.
// Segments (in windows): 4 of shrinking length (21 / 17 / 14 / 12) -- a window costs more the later it lies in the chunk
// (fuller buckets) and every seam costs a repair. Round 5, after the window parse lost a quarter of its vector instructions (the
// finishing steps, which grow along the chunk, lost less), configs[4]: boundaries 16/32/48: 56.9 ms, 18/34/49: 54.9, 20/37/51: 52.6,
// 22/40/53: 52.5, 24/43/55 (rounds 3-4): 53.5, 26/46/57: 54.4. With the 12-bit hash (fewer finishing steps late in a chunk), configs[4] in ms and
// configs[1..3]'s kernel time: 18/34/49: 53.14 / 1.043, 19/36/50: 52.49 / 1.012, 20/37/51: 52.29 / 0.991, 21/38/52: 52.33 / 0.977,
// 22/40/53: 52.67 / 0.978, 23/41/54: 52.95 / 0.969, 24/43/55: 53.53 / 0.966.
#define LZ4_NSEG 4u
#ifndef LZ4_B1
#define LZ4_B1 21u
#define LZ4_B2 38u
#define LZ4_B3 52u
#endif
__device__ __forceinline__ uint32_t lz4_seg_start(uint32_t j) { return j == 0 ? 0u : j == 1 ? LZ4_B1 : j == 2 ? LZ4_B2 : j == 3 ? LZ4_B3 : 64u; }
// the sort's three parts (wave 0: batches [0, P1), wave 1: [P1, P2), wave 2: [P2, 64)). A part's count field is as wide as its length asks: 10 bits up
// to 15 batches (960 positions), else 11 (up to 31 batches = 1 984); the three fields share one dword
#ifndef LZ4_P1
#define LZ4_P1 15u
#define LZ4_P2 39u
#endif
__host__ __device__ constexpr uint32_t lz4_max3(uint32_t a, uint32_t b, uint32_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
__host__ __device__ constexpr uint32_t lz4_field_bits(uint32_t batches) { return batches * 64u <= 0x3FFu ? 10u : 11u; }
#define LZ4_PMAX lz4_max3(LZ4_P1, LZ4_P2 - LZ4_P1, 64u - LZ4_P2)    // batches in the longest part
#define LZ4_F0 lz4_field_bits(LZ4_P1)                               // field widths of parts 0, 1, 2 (part 0 at bit 0, the others behind it)
#define LZ4_F1 lz4_field_bits(LZ4_P2 - LZ4_P1)
#define LZ4_F2 lz4_field_bits(64u - LZ4_P2)
static_assert(LZ4_P1 >= 1u && LZ4_P1 < LZ4_P2 && LZ4_P2 < 64u, "three parts, none empty");
static_assert(LZ4_P1 * 64u <= (1u << LZ4_F0) - 1u && (LZ4_P2 - LZ4_P1) * 64u <= (1u << LZ4_F1) - 1u && (64u - LZ4_P2) * 64u <= (1u << LZ4_F2) - 1u, "a part fits its count field");
static_assert(LZ4_F0 + LZ4_F1 + LZ4_F2 <= 32u, "the three fields share a dword");
static_assert(LZ4_P1 <= LZ4_PMAX && LZ4_P2 - LZ4_P1 <= LZ4_PMAX && 64u - LZ4_P2 <= LZ4_PMAX, "LZ4_PMAX");
#define LZ4_MAXM 22u                                             // matches that can START in one window of 64 positions
#ifdef LZ4_PROFILE
extern "C" void mscomp_amd_debug_lz4_prof(unsigned long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lz4_prof), sizeof(unsigned long long) * LZ4_NPROF); unsigned long long z[LZ4_NPROF] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_lz4_prof), z, sizeof z); }
#endif
static_assert(LZNT1_REC == 2u * 64u * LZ4_MAXM * sizeof(uint16_t), "kernels.h: LZNT1_REC = two areas of 64 windows of match tokens");
// (Blocks per CU by the scalar registers: a SIMD has 800 and gives a wave its count rounded up to a multiple of 16, plus 16, so a CU admits
// min(8, 800 / (ceil16(TotalSGPRs) + 16)) blocks of 256 threads: up to 80 registers 8 blocks, 81 to 96 SEVEN, 97 to 112 six -- while the compiler's own
// occupancy figure says 8 up to 100. Rounds 7 to 14 took 96 for the limit of eight blocks and ran at seven (93 to 96 registers: 6.79 waves per busy
// CU-cycle, 5.81 above 96; round 13 in profiles/HISTORY.md and its correction in round 15). Since round 15 the kernel uses 77 (76 since round 17) and runs at eight
// (7.76): lz_window keeps "candidate k reached 16 bytes" in the lanes instead of four 64-bit masks, and what sort and parse never read waits in the
// lanes of one vector register (LZ4_PARK below). tests/test_lznt1_resources.py holds all four instances at 80, without spills: an `amdgpu_num_sgpr`
// limit gets there too, by spilling, which the same test forbids. 68 since round 18; 72 since round 23, with two bodies behind one branch; 70 since round 25.)
// One LDS object, the chunk first (see the kernel above), 20 480 B -> 8 blocks per CU by the LDS. The chunk has no pad: the reads that run past its
// end (lz_ld128 / lds_ld32 reach up to 16 bytes beyond byte 4095, into the bucket array) and the bytes between n and 4096 only feed
// (a) keys of positions p with p + 3 <= n, whose fourth byte is masked off, (b) compares whose result is capped by
// max_len <= n - p (16-byte compares at 8 min(max_len, 16) bits, lz_lcp_tail clamped to max_len; a candidate q < p stops even
// earlier), (c) the raw chunk's copy, whose dwords past 2 + n land in the slot's slack and are never concatenated.
// (Declared here, not in the kernel: the kernel owns the one __shared__ object and hands it to whichever of its two bodies runs.)
struct Lz4Ctl {                                                            // parse state, polled or small
	u64      tok[64], mat[64];                                             // token / match mask per window
	uint16_t endc[64];                                                     // parse position after the window
	uint32_t prog[LZ4_NSEG];                                               // windows finished in segment j (index + 1)
	uint32_t used[LZ4_NSEG];                                               // entry position the seam in front of segment j was repaired against
	uint32_t segctr;                                                       // next segment to hand out
	uint32_t total[2];
	uint8_t  rep[64];                                                      // the window's match tokens are in the repair area (1) or the speculative one (0)
};
struct __attribute__((aligned(16))) Lz4Lds {
	uint8_t  data[4096];
	uint16_t bucket[4096];
	union {
		uint16_t cnt[LZ_TBL];                                              // after the parse: prefixes and flags (below)
		struct { uint32_t ends[LZ_TBL * 12u / 32u]; Lz4Ctl ctl; } parse;   // parse: the ends as 12-bit fields, then the control words
	} t;
};
static_assert(LZ_TBL == 4096u, "the pack below hands 16 bucket ends to each of 256 threads");
static_assert(sizeof(Lz4Lds) <= 20480, "eight blocks per CU");
static_assert(offsetof(Lz4Lds, t) == offsetof(Lz4Lds, bucket) + sizeof(Lz4Lds::bucket) && sizeof(Lz4Lds::bucket) + sizeof(Lz4Lds::t) == LZ_TBL * sizeof(uint32_t),
              "the sort's count words (one dword per bucket) lie over the bucket array and the union behind it");
// What sort and parse never read -- the slot's and the size index's addresses, the chunk and wave numbers -- waits in the lanes of one vector
// register until the parse is over: held in scalar registers across it these six cost the kernel its eighth block (see above). Lanes 6 to 10
// carry what the kernel hands to its body: the chunk's address, the record's address and the chunk's length (lz4_chunk_body).
// LZ4_FETCH reads a lane back; the empty asm in front of it redefines the register there, so the read cannot be moved up to the entry again.
#define LZ4_PARK(i, v) { park = lane == (i) ? (uint32_t)(v) : park; }
#define LZ4_FETCH(i) ({ asm volatile("" : "+v"(park)); (uint32_t)__builtin_amdgcn_readlane((int)park, (int)(i)); })
// FULL slots of the sort: slot i of a wave's part is batch pb0 + i, in the round of eight from i & ~7 on. A round runs in the waves whose part is
// longer than its first slot; slot i needs the test "batch inside my part" only if one of those parts ends at or before i. (With 15 / 24 / 25
// batches: slot 15 alone, where wave 0's part has ended.) And in a full chunk the only positions without a key are lanes 62 and 63 of batch 63,
// the last slot of the last part.
__host__ __device__ constexpr bool lz4_slot_sure(uint32_t i)
{
	const uint32_t j0 = i & ~7u, l0 = LZ4_P1, l1 = LZ4_P2 - LZ4_P1, l2 = 64u - LZ4_P2;
	return !(l0 > j0 && l0 <= i) && !(l1 > j0 && l1 <= i) && !(l2 > j0 && l2 <= i);
}
#define LZ4_LAST_SLOT (64u - LZ4_P2 - 1u)
// The kernel's body from section A on. FULL: the chunk has 4096 bytes and `n` is that literal everywhere (the argument is not read): 827 744 of the
// headline's 827 936 chunks. The other body is the code for any n; the kernel takes one wave-uniform branch between them.
template <bool serial, bool DEV, bool FULL>
__device__ __forceinline__ void lz4_chunk_body(Lz4Lds& L, uint32_t park, const uint32_t tid, const uint32_t lane, uint32_t wv)
{
	// (the chunk's address, its length and the record's address arrive in the parked lanes too. The kernel's branch is structurized with the
	// divergent code inside the bodies: the compiler lays the body for any n in front and the full-chunk body behind it under a 64-bit flag, so as
	// scalar arguments these five were live across the whole of the first body, and with them the kernel had 82 scalar registers: seven blocks.
	// From the lanes it has 72.)
	// (as GLOBAL pointers: a pointer rebuilt from integers has lost its address space, and every access through it would be a FLAT one -- see section D)
	typedef __attribute__((address_space(1))) const uint8_t  gc_u8;
	typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
	typedef __attribute__((address_space(1))) const u32x4    gc_u4;
	typedef __attribute__((address_space(1))) const uint32_t gc_u32;
	typedef __attribute__((address_space(1))) uint16_t       g_u16;
	gc_u8* __restrict__ const src = (gc_u8*)((uintptr_t)LZ4_FETCH(6) | ((uintptr_t)LZ4_FETCH(7) << 32));
	g_u16* __restrict__ const rec = (g_u16*)((uintptr_t)LZ4_FETCH(8) | ((uintptr_t)LZ4_FETCH(9) << 32));
	const uint32_t n = FULL ? 4096u : LZ4_FETCH(10);
	// (an assembler comment at both ends of each body, no instruction: it tells the two copies apart in the listing, where the census of a body is taken)
#define LZ4_BODY_EDGE(what) { if (FULL) { asm volatile("; lznt1 full-chunk body " what); } else { asm volatile("; lznt1 any-length body " what); } }
	LZ4_BODY_EDGE("begins")
	typedef Lz4Ctl Ctl;
	uint32_t c;                                                            // (re-fetched from the parked lanes behind the parse, like wv)
	uint32_t* const s_cw = reinterpret_cast<uint32_t*>(L.bucket);         // [LZ_TBL] the sort's count words (section B)
	uint8_t* const s_data = L.data; uint16_t* const s_cnt = L.t.cnt; uint16_t* const s_bucket = L.bucket;
	Ctl& C = L.t.parse.ctl;
	u64* const s_tok = C.tok; u64* const s_mat = C.mat; uint16_t* const s_endc = C.endc; uint8_t* const s_rep = C.rep;
	uint32_t* const s_prog = C.prog; uint32_t* const s_used = C.used; uint32_t& s_segctr = C.segctr; uint32_t* const s_total = C.total;
	uint16_t* const s_T = s_cnt;                                           // [64] tokens before window w          } after the parse, in the
	uint16_t* const s_S = s_cnt + 64;                                      // [64] token bytes before window w     } dead packed ends
	uint16_t* const s_flagpos = s_cnt + 128;                               // [512] byte position of group g's flag byte
	uint32_t* const s_flagacc = reinterpret_cast<uint32_t*>(s_cnt + 640);  // [512] its bits (1280 + 2048 B <= the ends' 6144 B)


#ifdef LZ4_PROFILE
	uint32_t z_prev; asm volatile("v_mov_b32 %0, %1" : "=v"(z_prev) : "s"((uint32_t)__builtin_readcyclecounter()));   // (the low dword: a phase is far below 2^32 cycles)
	uint32_t z_acc = 0;                                                    // (lane i keeps slot i; the last time stamp in a vector register too: with scalar ones the build loses its eighth block)
#define LZ4_T(i) { uint32_t t_; asm volatile("v_mov_b32 %0, %1" : "=v"(t_) : "s"((uint32_t)__builtin_readcyclecounter())); z_acc += lane == (i) ? t_ - z_prev : 0u; z_prev = t_; }
#define LZ4_TEND { if (lane < LZ4_NSLOT) { atomicAdd(&g_lz4_prof[LZ4_NSLOT * wv + lane], (unsigned long long)z_acc); } }
#else
#define LZ4_T(i)
#define LZ4_TEND
#endif
	// ---- A. stage the chunk, clear the count table (all waves) ------------------------------------------------------
	{
		const uint32_t nvec = (((uintptr_t)src & 15u) == 0) ? (n & ~15u) : 0u;
		for (uint32_t i = tid * 16u; i < nvec; i += 4096u) { *reinterpret_cast<u32x4*>(s_data + i) = *(gc_u4*)(src + i); }
		for (uint32_t i = nvec + tid; i < n; i += 256u) { s_data[i] = src[i]; }
		for (uint32_t i = n + tid; i < 4096u; i += 256u) { s_data[i] = 0; }
		for (uint32_t i = tid * 4u; i < LZ_TBL; i += 1024u) { *reinterpret_cast<uint4*>(s_cw + i) = make_uint4(0, 0, 0, 0); }
	}
	LZ4_T(0)
	__syncthreads();
	LZ4_T(1)
	// ---- B. position-sorted buckets: a stable counting sort by hash, ONE returning atomic per position, three waves at once -------
	// The chunk's 64 batches of 64 positions are three consecutive parts -- batches [0, 15), [15, 39), [39, 64) = 960 / 1536 / 1600
	// positions, for waves 0 / 1 / 2 -- and a bucket's count word holds one counter per part: 10 bits for part 0, 11 bits each for parts
	// 1 and 2 (LZ4_F0 / F1 / F2 follow the parts' lengths). A field cannot count past its part's length (960 <= 1023, 1600 <= 2047), so
	// nothing carries into a neighbour and there is no overflow path. Other splits (round 12, headline MB/s against 69 1xx for this one):
	// 25 / 24 / 15 69 158 / 68 902, 27 / 22 / 15 69 002 / 69 082, 29 / 20 / 15 68 569 / 68 832 -- wave 0 without a re-read gains nothing from a longer part. The 4096 words lie over the bucket array and the table union behind it (16 KiB, both dead until B3 / B4).
	//   B1. a wave walks its part in ascending batches and adds 1 to its field. What the atomic returns in that field is the position's
	//       rank among the same-hash positions of its PART: batches of a wave execute in order, the lanes of one DS instruction are served
	//       in lane order (what `serial` replaces), and the other waves' adds go to other fields. This is the only pass that HASHES a position
	//       (unaligned dword read, mask, multiply, shift, select for hash 0): hash and rank stay in one register per position, hash << 12 | rank.
	//   B2. the counts are final: waves 1 and 2 add the counts of the parts in front of their own to their ranks -- the count word is read at
	//       the hash kept in the register; the sum stays below 4 096, so nothing carries into the hash; every thread takes
	//       the words of 16 consecutive buckets and sums them; waves 0 and 1 leave their totals in the two halves of word 0 (bucket 0 is
	//       always empty, lz_hash), wave 3's prefix is the chunk's number of keys minus its own total: no barrier for the partial sums.
	//   B3. every table word has been read: a thread writes the ENDS of its 16 buckets as 12-bit fields (6 dwords at 24 tid), and the
	//       control words are initialised behind them.
	//   B4. scatter with plain stores: bucket[end[h - 1] + rank] = p, h and rank from the register.
	// Wave 3 has no part: it stages, scans and packs with the others.
	{
		const uint32_t nb = (n + 63u) >> 6;
		const uint32_t pb0 = wv == 0 ? 0u : wv == 1u ? LZ4_P1 : wv == 2u ? LZ4_P2 : 64u;     // my part: batches [pb0, pb1)
		const uint32_t pe = wv == 0 ? LZ4_P1 : wv == 1u ? LZ4_P2 : 64u;
		const uint32_t pb1 = pe < nb ? pe : nb;
		const uint32_t fsh = wv == 0 ? 0u : wv == 1u ? LZ4_F0 : LZ4_F0 + LZ4_F1;          // my field
		const uint32_t fm = (1u << (wv == 0 ? LZ4_F0 : wv == 1u ? LZ4_F1 : LZ4_F2)) - 1u;
		uint32_t hr[LZ4_PMAX];                                            // per position of mine: hash << 12 | rank
		#pragma unroll
		for (uint32_t i = 0; i < LZ4_PMAX; ++i) { hr[i] = 0; }
		// B1. rounds of 8 batches: their atomics are issued back to back (DS operations of a wave execute in order; the wavefront-scope
		// form keeps the compiler from waiting for each one). An inactive lane's rank stays 0. This is the ONLY place that hashes a position.
		// FULL: a slot that is surely a batch of the wave's part carries no predicate, so its atomic stands under no exec-mask bracket and its `old` is not
		// zeroed first; batch 63 keeps the position test (lanes 62 and 63). The atomic's operand is made once per wave, in a register of its own
		// (left to the compiler it is moved there again in every batch).
		uint32_t inc = 1u << fsh;
		if (FULL) { asm("v_mov_b32 %0, %1" : "=v"(inc) : "s"(1u << fsh)); }
		#pragma unroll
		for (uint32_t j0 = 0; j0 < LZ4_PMAX; j0 += 8u) {
			if (pb0 + j0 < pb1) {
				uint32_t h[8], old[8];
				#pragma unroll
				for (uint32_t j = 0; j < 8u; ++j) { if (j0 + j < LZ4_PMAX) { h[j] = lz_hash(lz_ld32_lane(s_data + (pb0 + j0) * 64u + (lane & 0x3Cu) + 64u * j, lane) & 0xFFFFFFu); } }   // (batches below 64: inside the chunk)
				#pragma unroll
				for (uint32_t j = 0; j < 8u; ++j) {
					if (j0 + j < LZ4_PMAX) {
						const uint32_t b = pb0 + j0 + j;
						const bool act = FULL ? (lz4_slot_sure(j0 + j) || b < pb1) && (j0 + j != LZ4_LAST_SLOT || b * 64u + lane + 2u < n)
						                      : b < pb1 && b * 64u + lane + 2u < n;
						old[j] = lz_ordered_add<serial>(s_cw + h[j], inc, act, lane);
					}
				}
				#pragma unroll
				for (uint32_t j = 0; j < 8u; ++j) { if (j0 + j < LZ4_PMAX) { hr[j0 + j] = (h[j] << 12) | ((old[j] >> fsh) & fm); } }
			}
		}
		LZ4_T(2)
		__syncthreads();
		LZ4_T(3)
		// B2. (a lane without a key has rank 0 and adds at most the lengths of parts 0 and 1 of some other bucket, below 4 096: nothing carries into
		// the hash above the rank)
		static_assert(LZ4_P2 * 64u < 4096u, "rank + counts in front stay in 12 bits");
		if (wv == 1u || wv == 2u) {
			const uint32_t m1 = wv == 2u ? (1u << LZ4_F1) - 1u : 0u;
			#pragma unroll
			for (uint32_t j0 = 0; j0 < LZ4_PMAX; j0 += 8u) {
				if (pb0 + j0 < pb1) {
					uint32_t w[8];
					#pragma unroll
					for (uint32_t j = 0; j < 8u; ++j) { if (j0 + j < LZ4_PMAX) { w[j] = s_cw[hr[j0 + j] >> 12]; } }
					#pragma unroll
					for (uint32_t j = 0; j < 8u; ++j) { if (j0 + j < LZ4_PMAX) { hr[j0 + j] += (w[j] & ((1u << LZ4_F0) - 1u)) + ((w[j] >> LZ4_F0) & m1); } }
					__builtin_amdgcn_sched_barrier(0);                        // (the rounds are independent: merged, their reads in flight cost the eighth block's registers)
				}
			}
		}
		uint32_t tot[8], sum = 0;                                         // the sizes of buckets 16 tid .. 16 tid + 15, two per register
		#pragma unroll
		for (uint32_t k = 0; k < 4u; ++k) {
			const uint4 a = reinterpret_cast<const uint4*>(s_cw)[4u * tid + k];
			uint32_t x[4] = { a.x, a.y, a.z, a.w };
			#pragma unroll
			for (uint32_t i = 0; i < 4u; ++i) { x[i] = (x[i] & ((1u << LZ4_F0) - 1u)) + ((x[i] >> LZ4_F0) & ((1u << LZ4_F1) - 1u)) + (x[i] >> (LZ4_F0 + LZ4_F1)); }
			if (k == 0 && tid == 0) { x[0] = 0; }                          // (word 0 counts nothing: it carries the wave totals)
			sum += (x[0] + x[1]) + (x[2] + x[3]);
			tot[2u * k] = x[0] | (x[1] << 16); tot[2u * k + 1u] = x[2] | (x[3] << 16);
			__builtin_amdgcn_sched_barrier(0);                            // (as above)
		}
		const uint32_t incl = wave_incl_scan_add_u32(sum);
		const uint32_t wtot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
		if (lane == 63u && wv < 2u) { reinterpret_cast<uint16_t*>(s_cw)[wv] = (uint16_t)wtot; }
		LZ4_T(4)
		__syncthreads();
		LZ4_T(5)
		// B3.
		{
			const uint32_t x = s_cw[0];
			const uint32_t keys = n > 2u ? n - 2u : 0u;                   // positions p with p + 2 < n
			const uint32_t wpre = wv == 0 ? 0u : wv == 1u ? (x & 0xFFFFu) : wv == 2u ? (x & 0xFFFFu) + (x >> 16) : keys - wtot;
			uint32_t r = wpre + incl - sum;
			uint32_t* const o = L.t.parse.ends + 6u * tid;
			#pragma unroll
			for (int k = 0; k < 2; ++k) {                                 // 8 ends -> 3 dwords
				uint32_t v[8];
				#pragma unroll
				for (int i = 0; i < 4; ++i) { r += tot[4 * k + i] & 0xFFFFu; v[2 * i] = r; r += tot[4 * k + i] >> 16; v[2 * i + 1] = r; }
				o[3 * k]      = v[0] | (v[1] << 12) | (v[2] << 24);
				o[3 * k + 1u] = (v[2] >> 8) | (v[3] << 4) | (v[4] << 16) | (v[5] << 28);
				o[3 * k + 2u] = (v[5] >> 4) | (v[6] << 8) | (v[7] << 20);
			}
			if (tid < LZ4_NSEG) { s_prog[tid] = 0; s_used[tid] = 0; }
			if (tid < 16u) { reinterpret_cast<uint32_t*>(s_rep)[tid] = 0; }
			if (tid == 0) { s_segctr = 0; }
		}
		LZ4_T(6)
		__syncthreads();
		LZ4_T(7)
		// B4. (start(h): the lookup of lz_window<true>)
		#pragma unroll
		for (uint32_t j0 = 0; j0 < LZ4_PMAX; j0 += 8u) {
			if (pb0 + j0 < pb1) {
				uint32_t st[8];
				#pragma unroll
				for (uint32_t j = 0; j < 8u; ++j) {
					if (j0 + j < LZ4_PMAX) {
						const uint32_t bit = (hr[j0 + j] >> 12) * 12u - 12u;          // (every lane of a round that ran holds a hash >= 1, active or not)
						const uint32_t* const t = L.t.parse.ends + (bit >> 5);
						st[j] = __builtin_amdgcn_alignbit(t[1], t[0], bit) & 0xFFFu;
					}
				}
				#pragma unroll
				for (uint32_t j = 0; j < 8u; ++j) {
					if (j0 + j < LZ4_PMAX) {
						const uint32_t b = pb0 + j0 + j, p = b * 64u + lane;
						const bool act = FULL ? (lz4_slot_sure(j0 + j) || b < pb1) && (j0 + j != LZ4_LAST_SLOT || p + 2u < n)   // (B1's predicate)
						                      : b < pb1 && p + 2u < n;
						if (act) { s_bucket[st[j] + (hr[j0 + j] & 0xFFFu)] = (uint16_t)p; }
					}
				}
			}
		}
	}
	LZ4_T(8)
	__syncthreads();
	const uint32_t* const tbl = L.t.parse.ends;
	LZ4_T(9)

	// ---- C1. speculative parse of my segment ------------------------------------------------------------------------
	const uint32_t nw = (n + 63u) >> 6;
	// one window: parse, record (the match tokens into area a_). Hands back the parse position after it, wave-uniform.
	// (The lanes that record are the match mask itself, as the exec mask: `(mask >> lane) & 1` is two ANDs with the lane's bit and a 64-bit
	// compare in every lane. The record's base is a scalar pointer -- w_ and a_ are uniform -- so a lane adds a 32-bit offset to it.)
	// The two arms -- the window lies behind the position already (a match covers it whole), or it is parsed -- only PRODUCE the token mask, the match
	// mask and the position; one store sequence behind their join writes the window's control words, EVERY lane the same value to the same address
	// (relaxed wavefront-scope stores: plain ds_write, no LDS cycle more than one lane's -- SQ_LDS_BANK_CONFLICT is the same to the digit). Under
	// `lane == 0` in each arm these were three divergent regions per window: the structurizer merged the arms' stores into one region fed by 64-bit
	// flags, turned the uniform "behind the position" test into flag code and bracketed every store with an exec save and restore -- 10
	// scalar instructions per window by the counters (profiles/HISTORY.md round 25). The record store keeps its region: it is per-lane work.
	// in_ (with FULL): the loop may run windows 1 to 62 through lz_window's INNER copy, picked by one scalar test on w_. The speculative loop alone
	// says so: each copy is 4 to 6 KB of code, and tests/test_lznt1_full_listing.py holds the kernel below 64 KB.
	// (which windows: 1 to 62 but 1, 2, 4, 8, 16 and 32, where lane 0 has a larger split than lanes 1 to 63 -- lz_window, INNER. One bit of a
	// constant mask: written as `w < 63 && (w & (w - 1))` the two conditions become 64-bit flags, eight scalar instructions per window.)
#define LZ4_INNER_WINDOWS 0x7FFFFFFEFFFEFEE8ull
#define LZ4_WINDOW(w_, entry_, cur_out, a_, in_) { \
		const uint32_t wb_ = (w_) * 64u; const uint32_t we_ = FULL ? wb_ + 64u : ((wb_ + 64u < n) ? wb_ + 64u : n); \
		u64 tk_ = 0, mt_ = 0; \
		if ((entry_) >= we_) { cur_out = (entry_); } \
		else { \
			LzWin r_; \
			if (FULL && (in_) && lz_bit64(LZ4_INNER_WINDOWS, (w_))) { cur_out = lz_window<true, true, true>(s_data, tbl, s_bucket, n, lane, wb_, (entry_), r_); } \
			else { cur_out = lz_window<true, FULL>(s_data, tbl, s_bucket, n, lane, wb_, (entry_), r_); } \
			if (__builtin_amdgcn_inverse_ballot_w64(r_.matchmask)) { \
				const uint32_t p_ = wb_ + lane, best_ = r_.key >> 12; \
				g_u16* __restrict__ const recw_ = rec + ((a_) * 64u + (w_)) * LZ4_MAXM; \
				recw_[popc_below(r_.matchmask)] = (uint16_t)(((p_ - (4095u - (r_.key & 0xFFFu)) - 1u) << r_.shift) | (best_ - 3u)); \
			} \
			tk_ = r_.tokmask; mt_ = r_.matchmask; \
		} \
		cur_out = LZ4_UNI(cur_out); \
		wst64(&s_tok[w_], tk_); wst64(&s_mat[w_], mt_); wst16(&s_endc[w_], cur_out); \
		if (a_) { wst8(&s_rep[w_], 1u); } }
	// The window loops run on the scalar unit: the window number, the parse position and what is read back from the control words (a recorded
	// position, a progress word) are wave-uniform, and LZ4_UNI says so where each value is born -- a read of LDS lands in a vector register, and
	// the loop's own increment, left to the compiler, is copied into both arms of the `lane == 0` store in front of it, which makes the counter a
	// value joined under a divergent branch: window number and position then live in vector registers, the "window already behind the
	// position" test and the loop's back edge become exec-mask code. Since round 25 no `lane == 0` store is left in the loops (LZ4_WINDOW above; the
	// progress word the same way, by the workgroup-scope store it always was): masks and position first, wave_fence(), then the progress word -- DS
	// operations of a wave execute in program order, which is all the seam protocol asks.
#define LZ4_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
	// the segments are handed out in order (with four of them: one per wave)
	for (;;) {
		uint32_t seg = 0;
		if (lane == 0) { seg = atomicAdd(&s_segctr, 1u); }
		seg = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg);
		const uint32_t a0 = lz4_seg_start(seg);
		if (a0 >= nw) { break; }
		const uint32_t a1 = (lz4_seg_start(seg + 1u) < nw) ? lz4_seg_start(seg + 1u) : nw;
		uint32_t entry = a0 * 64u;                                 // (exact for segment 0)
		for (uint32_t w = a0; w < a1; w = LZ4_UNI(w + 1u)) {
			uint32_t cur;
			LZ4_WINDOW(w, entry, cur, 0u, 1)
			entry = cur;
			wave_fence();
			__hip_atomic_store(&s_prog[seg], w + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		}
		// repair the seam behind my segment: continue with my position (true unless my own segment never re-synchronised)
		// into the next segment until the position after a window equals the recorded one
		if (a1 < nw) {
			if (lane == 0) { s_used[seg + 1u] = entry; }
			if (entry != a1 * 64u) {
				const uint32_t wlim = (lz4_seg_start(seg + 2u) < nw) ? lz4_seg_start(seg + 2u) : nw;
				for (uint32_t w = a1; w < wlim; w = LZ4_UNI(w + 1u)) {
					while (LZ4_UNI(__hip_atomic_load(&s_prog[seg + 1u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) <= w) { __builtin_amdgcn_s_sleep(2); }
					wave_fence();
					const uint32_t spec = LZ4_UNI(s_endc[w]);
					uint32_t cur;
					LZ4_WINDOW(w, entry, cur, 1u, 0)
					entry = cur;
					if (cur == spec) { break; }
				}
			}
		}
	}
	LZ4_T(10)
	__syncthreads();
	LZ4_T(11)
	// ---- C3. (wave 0) cascade check, then tokens / bytes before every window -----------------------------------------
	wv = LZ4_FETCH(5);
	if (wv == 0) {
		for (uint32_t j = 1; j < LZ4_NSEG && lz4_seg_start(j) < nw; ++j) {
			uint32_t e2 = LZ4_UNI(s_endc[lz4_seg_start(j) - 1u]);
			if (e2 == LZ4_UNI(s_used[j])) { continue; }                        // (else a repair ran through the whole of segment j-1: rare)
			uint32_t wl = lz4_seg_start(j);                           // first window NOT walked
			for (uint32_t w = lz4_seg_start(j); w < nw; w = LZ4_UNI(w + 1u)) {
				const uint32_t spec = LZ4_UNI(s_endc[w]);
				uint32_t cur;
				LZ4_WINDOW(w, e2, cur, 1u, 0)
				e2 = cur;
				wave_fence();
				wl = w + 1u;
				if (cur == spec) { break; }
			}
			// every seam this walk crossed is consistent now
			if (lane == 0) { for (uint32_t jj = j + 1u; jj < LZ4_NSEG && lz4_seg_start(jj) < wl; ++jj) { s_used[jj] = s_endc[lz4_seg_start(jj) - 1u]; } }
			wave_fence();
		}
	}
	LZ4_T(12)
	__syncthreads();                                              // the packed ends are dead from here on: prefixes and flags take their place
	LZ4_T(13)
	for (uint32_t i = tid; i < 512u; i += 256u) { s_flagacc[i] = 0; }
	// the last window is parsed: back come the wave and chunk numbers and the two addresses
	wv = LZ4_FETCH(5); c = LZ4_FETCH(4);
	const uint32_t w0 = wv * 16u, w1 = (w0 + 16u < nw) ? w0 + 16u : nw;
	// (a pointer rebuilt from integers has lost its address space, and every store through it would be a FLAT one behind a 64-bit vector add, counted on
	// lgkmcnt with the LDS reads: the two come back as GLOBAL pointers, so a store is global_store_* with this scalar base and a 32-bit lane offset)
	typedef __attribute__((address_space(1))) uint8_t  g_u8;
	typedef __attribute__((address_space(1))) uint32_t g_u32;
	g_u8* __restrict__ const img = (g_u8*)((uintptr_t)LZ4_FETCH(0) | ((uintptr_t)LZ4_FETCH(1) << 32)) + (u64)c * LZNT1_SLOT;
	g_u32* __restrict__ const szp = (g_u32*)((uintptr_t)LZ4_FETCH(2) | ((uintptr_t)LZ4_FETCH(3) << 32)) + c;
	// ---- D0. the match tokens of my 16 windows, from the records in global memory (L2-warm: written by this block) into my piece of the dead
	// bucket array, in ONE coalesced pass of dwords (a window's LZ4_MAXM tokens are 11 dwords; 176 per wave = three loads per lane, all in
	// flight together, under wave 0's scans). Lane l < 16 knows window w0 + l: how many matches start in it and which area holds its tokens;
	// a dword is fetched only if the window has a token for it. The emission loop then reads LDS alone.
	static_assert(LZNT1_SLOT <= 0xFFFFFFFFu && (LZ4_MAXM & 1u) == 0 && LZ4_NSEG * 16u * LZ4_MAXM <= 4096u, "a window's tokens are whole dwords; four pieces fit the bucket array");
	uint32_t* const s_ptk = reinterpret_cast<uint32_t*>(s_bucket) + wv * (16u * LZ4_MAXM / 2u);
	// The emission loop's control words wait in the lanes as well: lane l (every 16 lanes alike) holds the token mask and the match mask of window
	// w0 + l here, and the tokens and token bytes in front of it behind wave 0's scans below. An iteration reads them with v_readlane, so the loop
	// tests and branches on the scalar unit and the masks are its exec masks.
	const uint32_t wl0 = w0 + (lane & 15u);
	const u64 tokv = wl0 < w1 ? s_tok[wl0] : (u64)0, matv = wl0 < w1 ? s_mat[wl0] : (u64)0;
#ifndef LZ4_PROBE_EMIT
	{
		const uint32_t info = wl0 < w1 ? (uint32_t)__popcll(matv) | ((uint32_t)s_rep[wl0] << 8) : 0u;
		gc_u32* __restrict__ const rec32 = (gc_u32*)rec;
		uint32_t v[3]; bool ld[3];
		#pragma unroll
		for (uint32_t k = 0; k < 3u; ++k) {
			const uint32_t idx = lane + 64u * k, wl = idx / (LZ4_MAXM / 2u), m2 = idx - wl * (LZ4_MAXM / 2u);
			const uint32_t inf = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(wl * 4u), (int)info);
			ld[k] = idx < 16u * LZ4_MAXM / 2u && 2u * m2 < (inf & 0xFFu);
			v[k] = ld[k] ? rec32[((inf >> 8) * 64u + w0 + wl) * (LZ4_MAXM / 2u) + m2] : 0u;
		}
		#pragma unroll
		for (uint32_t k = 0; k < 3u; ++k) { if (ld[k]) { s_ptk[lane + 64u * k] = v[k]; } }
	}
#endif
	if (wv == 0) {
		const u64 tm = lane < nw ? s_tok[lane] : (u64)0, mk = lane < nw ? s_mat[lane] : (u64)0;
		const uint32_t nt = (uint32_t)__popcll(tm), ns = nt + (uint32_t)__popcll(mk);
		const uint32_t ti = wave_incl_scan_add_u32(nt), si = wave_incl_scan_add_u32(ns);
		s_T[lane] = (uint16_t)(ti - nt); s_S[lane] = (uint16_t)(si - ns);
		if (lane == 63u) { s_total[0] = ti; s_total[1] = si; }
	}
	LZ4_T(14)
	__syncthreads();
	LZ4_T(15)
	const uint32_t T = s_total[0], S = s_total[1];
	const uint32_t csize = ((T + 7u) >> 3) + S;
	uint32_t total;
	if (csize < n) {
		// ---- D1. emission of my windows: pos(t) = 2 (header) + (t div 8 + 1) + sum size(u<t) --------------------------
		// the match tokens come from my piece of LDS (D0): token k of window w at 16-bit index (w - w0) LZ4_MAXM + k. No global load and no
		// dependent LDS read sit in the loop; the byte stores address the chunk's slot with one scalar base and 32-bit offsets.
		// Every token lane reads its literal byte and a token word (a lane without a match reads the word behind the window's last token: inside the
		// bucket array, never used), selects the low byte by the match mask and stores it; the match lanes then store the high byte and set their
		// flag bit. One region under the token mask with the match lanes' inside it, and the flag-position store under its own test.
		const uint32_t tsv = (uint32_t)s_T[wl0] | ((uint32_t)s_S[wl0] << 16);   // (wl0 < 64: wave 0 wrote all 64 entries)
		const uint32_t nwin = LZ4_UNI(w1 > w0 ? w1 - w0 : 0u);
		#pragma unroll 1
		for (uint32_t k = 0; k < nwin; ++k) {
			const u64 tokmask = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(tokv >> 32), (int)k) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)tokv, (int)k);
			if (tokmask == 0) { continue; }
			const u64 matchmask = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(matv >> 32), (int)k) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)matv, (int)k);
			const uint32_t ts = (uint32_t)__builtin_amdgcn_readlane((int)tsv, (int)k);
			const uint32_t tb = popc_below(tokmask), mbl = popc_below(matchmask);
			const uint32_t t = (ts & 0xFFFFu) + tb;
			const uint32_t pos = (3u + (ts >> 16)) + (t >> 3) + tb + mbl;     // (the window's part is scalar: added once)
			if (__builtin_amdgcn_inverse_ballot_w64(tokmask)) {
				if ((t & 7u) == 0) { s_flagpos[t >> 3] = (uint16_t)(pos - 1u); }
				const uint32_t lit = s_data[(w0 + k) * 64u + lane];
#ifdef LZ4_PROBE_EMIT   // dev-only, NOT exact, timing only: the emission without any token read
				const uint16_t tok = 0x1003u;
#else
				const uint16_t tok = reinterpret_cast<const uint16_t*>(s_ptk)[k * LZ4_MAXM + mbl];
#endif
				// (the mask itself selects; only the low byte is stored, so the token travels with an undefined upper half: lz_entry32)
				uint32_t lo; asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(lo) : "v"(lit), "v"(lz_entry32(tok)), "s"(matchmask));
				img[pos] = (uint8_t)lo;
				if (__builtin_amdgcn_inverse_ballot_w64(matchmask)) {
					// (the + 1 goes into the store's offset field. The offset is redefined inside this block: a value that arrives from the block above
					// already widened to 64 bits is added to the base in vector registers)
					uint32_t p1 = pos; asm("" : "+v"(p1));
					(img + p1)[1] = (uint8_t)(tok >> 8);
					atomicOr(&s_flagacc[t >> 3], 1u << (t & 7u));
				}
			}
		}
		LZ4_T(16)
		__syncthreads();
		LZ4_T(17)
		#pragma unroll 1
		for (uint32_t g = tid; g < ((T + 7u) >> 3); g += 256u) { uint32_t fp = s_flagpos[g]; asm("" : "+v"(fp)); img[fp] = (uint8_t)s_flagacc[g]; }   // (at most 512 groups: two rounds; a 32-bit offset to the scalar base)
		if (tid == 0) { img[0] = (uint8_t)(0xB000u | (csize - 1u)); img[1] = (uint8_t)((0xB000u | (csize - 1u)) >> 8); }
		total = 2u + csize;
	} else {
		const uint32_t hdr = 0x3000u | (n - 1u);
		for (uint32_t k = tid; k < (n + 2u + 3u) / 4u; k += 256u) {
			uint32_t o = 4u * k; asm("" : "+v"(o));                     // (a 32-bit byte offset to the scalar base, kept from becoming a 64-bit induction variable)
			*(g_u32*)(img + o) = (k == 0) ? (hdr | (ld16(s_data) << 16)) : ld32(s_data + 4u * k - 2u);
		}
		total = 2u + n;
	}
	if (tid == 0) { *szp = total; }
	LZ4_T(18)
	LZ4_TEND
	LZ4_BODY_EDGE("ends")
#undef LZ4_BODY_EDGE
#undef LZ4_WINDOW
#undef LZ4_INNER_WINDOWS
#undef LZ4_UNI
}

template <bool serial, bool DEV = false>                         // DEV: as lznt1_chunk_kernel
__global__ __launch_bounds__(256) void lznt1_chunk4_kernel(const uint8_t* __restrict__ d_in, BatchTables bt,
                                                          uint8_t* __restrict__ slots, uint32_t* __restrict__ slot_size, uint16_t* __restrict__ recs)
{
	__shared__ Lz4Lds L;
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const uint32_t c = blockIdx.x, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
	if (DEV && past_real_chunks(bt, c)) { if (tid == 0) { slot_size[c] = 0; } return; }
	uint32_t park = 0;
	LZ4_PARK(0, (uintptr_t)slots) LZ4_PARK(1, (uintptr_t)slots >> 32) LZ4_PARK(2, (uintptr_t)slot_size) LZ4_PARK(3, (uintptr_t)slot_size >> 32)
	LZ4_PARK(4, c) LZ4_PARK(5, wv)
	const uint32_t u = unit_of_chunk(bt.chunk_prefix, bt.n_units, c);
	const u64 coff = (u64)(c - bt.chunk_prefix[u]) * 4096u;
	const u64 left = bt.in_len[u] - coff;
	const uint32_t n = left < 4096u ? (uint32_t)left : 4096u;
	const uint8_t* __restrict__ src = d_in + bt.in_off[u] + coff;
	// the window's match tokens, in order: area 0 is written by the speculative parse of the window's own segment, area 1 by a seam
	// repair or the cascade (s_rep says which holds). Two areas, because the repairing wave would otherwise race the speculative
	// wave's global stores to the same words: its progress word in LDS does not wait for them.
	uint16_t* __restrict__ rec = recs + (u64)c * (LZNT1_REC / sizeof(uint16_t));
	// Two bodies, one wave-uniform branch: every chunk of a unit but its last has 4096 bytes, and with that literal for n the window prologue, the
	// sort's predicates and the geometry are constants. Only a unit's last chunk can take the other body, the code for any n.
	LZ4_PARK(6, (uintptr_t)src) LZ4_PARK(7, (uintptr_t)src >> 32) LZ4_PARK(8, (uintptr_t)rec) LZ4_PARK(9, (uintptr_t)rec >> 32) LZ4_PARK(10, n)
	asm volatile("" : "+v"(park));                                         // (and the selects that fill it stay here: left alone they sink to the first read)
	if ((uint32_t)__builtin_amdgcn_readfirstlane((int)n) == 4096u) { lz4_chunk_body<serial, DEV, true>(L, park, tid, lane, wv); }
	else { lz4_chunk_body<serial, DEV, false>(L, park, tid, lane, wv); }
#undef LZ4_PARK
#undef LZ4_FETCH
}

// DEV = true: the instances of compress plans with device tables, compiled in lznt1_dev.hip (this file included with LZNT1_DEV_TU defined), so
// that this file's code object holds the host plans' kernels alone, as before
template <bool DEV>
static void launch_lznt1_chunks_t(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, uint8_t* slots, uint32_t* slot_size, uint16_t* recs,
                                  int mode, bool serial)
{
	if (mode == 1) {
		if (serial) { hipLaunchKernelGGL((lznt1_chunk_kernel<true, DEV>), dim3(bt.n_chunks), dim3(64), 0, st, d_in, bt, slots, slot_size); }
		else { hipLaunchKernelGGL((lznt1_chunk_kernel<false, DEV>), dim3(bt.n_chunks), dim3(64), 0, st, d_in, bt, slots, slot_size); }
	} else {
		if (serial) { hipLaunchKernelGGL((lznt1_chunk4_kernel<true, DEV>), dim3(bt.n_chunks), dim3(256), 0, st, d_in, bt, slots, slot_size, recs); }
		else { hipLaunchKernelGGL((lznt1_chunk4_kernel<false, DEV>), dim3(bt.n_chunks), dim3(256), 0, st, d_in, bt, slots, slot_size, recs); }
	}
}
void launch_lznt1_chunks_dev(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, uint8_t* slots, uint32_t* slot_size, uint16_t* recs,
                             int mode, bool serial);
#ifndef LZNT1_DEV_TU
void launch_lznt1_chunks(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, uint8_t* slots, uint32_t* slot_size, uint16_t* recs, bool dev)
{
	if (bt.n_chunks == 0) { return; }
	const int forced = g_sw.lznt1.load(std::memory_order_relaxed);   // (host.h Switches: 0 = default, 1 = one wave per chunk, 2 = four waves per chunk)
	const int mode = forced ? forced : 2;                             // four waves per chunk: 1.43 vs 1.74 ms on the headline workload
	const bool serial = serial_atomics_on_current_device();
	if (dev) { launch_lznt1_chunks_dev(st, d_in, bt, slots, slot_size, recs, mode, serial); }
	else { launch_lznt1_chunks_t<false>(st, d_in, bt, slots, slot_size, recs, mode, serial); }
}
#else
void launch_lznt1_chunks_dev(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, uint8_t* slots, uint32_t* slot_size, uint16_t* recs,
                             int mode, bool serial)
{
	launch_lznt1_chunks_t<true>(st, d_in, bt, slots, slot_size, recs, mode, serial);
}
#endif

} // namespace msc
