// common.h -- device helpers shared by the gfx950 kernels (wave64 idioms, LDS byte access, batch tables).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msc {

typedef uint64_t u64;

// ---- wave64 helpers (gfx950: wavefront = 64 lanes, hard-coded) -----------------------------------------
__device__ __forceinline__ uint32_t lane_id()
{
	return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}
// number of set bits of m strictly below this lane
__device__ __forceinline__ uint32_t popc_below(u64 m)
{
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ uint32_t ctz64(u64 m) { return (uint32_t)__builtin_ctzll(m); }
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ u64 sgpr64(u64 v)   // tell the compiler a wave-uniform 64-bit value lives in SGPRs
{
	return ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
// op over the values of all 64 lanes, in every lane (a butterfly; op associative and commutative, v of 32 or 64 bits)
template <class T, class Op>
__device__ __forceinline__ T wave_all(T v, Op op)
{
	#pragma unroll
	for (uint32_t d = 32u; d; d >>= 1) { v = op(v, __shfl_xor(v, d, 64)); }
	return v;
}

// DPP scans over the 64 lanes: row_shr 1,2,4,8 then row_bcast 15/31, the max/add folded into the DPP instruction itself
// (the builtin form costs v_mov + v_mov_dpp + op per step). A lane whose DPP source is out of range or whose row is
// masked off keeps its value. Two wait states are required between a VALU write and a DPP read of the same VGPR.
#define MSC_DPP_SCAN(op) \
	"s_nop 1\n\t" op " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t" \
	"s_nop 1\n\t" op " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t" \
	"s_nop 1\n\t" op " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t" \
	"s_nop 1\n\t" op " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t" \
	"s_nop 1\n\t" op " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t" \
	"s_nop 1\n\t" op " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t" \
	"s_nop 1"
__device__ __forceinline__ uint32_t wave_incl_scan_max(uint32_t v) { asm volatile(MSC_DPP_SCAN("v_max_u32_dpp") : "+v"(v)); return v; }
__device__ __forceinline__ uint32_t wave_incl_scan_add_u32(uint32_t v) { asm volatile(MSC_DPP_SCAN("v_add_u32_dpp") : "+v"(v)); return v; }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_max(v), 63); }

// ---- LDS / global byte-granular access ----------------------------------------------------------------
// gfx950 has unaligned DS access enabled: a misaligned 4-byte LDS read is ONE ds_read_b32.
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__device__ __forceinline__ uint32_t ld16(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }
__device__ __forceinline__ void     st16(uint8_t* p, uint32_t v) { uint16_t w = (uint16_t)v; __builtin_memcpy(p, &w, 2); }
__device__ __forceinline__ void     st32(uint8_t* p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

// Index of the first non-zero byte of the 16-byte value x (little endian), 16 when x == 0. Branch-free, 10 VALU:
// v_ffbl_b32 returns 0xFFFFFFFF for a zero dword (the builtin ctz is undefined there, so the instruction is named
// directly); OR-ing 32 / 64 / 96 into a bit index below 32 ADDS the dword's offset and leaves the all-ones "none" as it
// is, and the unsigned minimum picks the first hit. (Round 5: v_or_b32 where rounds 1-4 had v_add_u32 ... clamp. A
// 3-operand / modifier-carrying VOP3 instruction issues at HALF the rate of a VOP1 / VOP2 one on this GPU -- 1 against 2
// wave-instructions per CU and cycle, tools/dev/issue_peak.hip -- and the clamp made the three adds VOP3.)
__device__ __forceinline__ uint32_t ffbl_raw(uint32_t x) { uint32_t r; asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x)); return r; }
__device__ __forceinline__ uint32_t min3u(uint32_t a, uint32_t b, uint32_t c) { const uint32_t t = a < b ? a : b; return t < c ? t : c; }
__device__ __forceinline__ uint32_t first_nz_byte16(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3)
{
	const uint32_t a = ffbl_raw(x1) | 32u, b = ffbl_raw(x2) | 64u, c = ffbl_raw(x3) | 96u;
	return min3u(min3u(ffbl_raw(x0), a, b), c, 128u) >> 3;
}

// v_alignbyte_b32 with a BYTE ADDRESS as its shift: the instruction takes the byte shift from bits [1:0] of its third operand and ignores
// the rest (the gfx9-family ISA documents say so; util.hip alignbyte_check_kernel asks the device, tests/test_gpu_alignbyte.py), so the
// `& 3` in front of it is a vector instruction for nothing. The helper is the one place that relies on it: = {hi, lo} >> 8 (addr & 3).
__device__ __forceinline__ uint32_t alignbyte_addr(uint32_t hi, uint32_t lo, uint32_t addr) { return __builtin_amdgcn_alignbyte(hi, lo, addr); }

// 16 bytes at ANY byte offset of an LDS array whose base is 4-byte aligned. A byte-misaligned ds_read_b128 is replayed
// by the LDS pipe (about 64 cycles; SQ_LDS_UNALIGNED_STALL was 77 % of the match finder's LDS cycles), so read 5 ALIGNED
// dwords and funnel-shift (v_alignbyte).
__device__ __forceinline__ uint4 lds_ld128(const uint8_t* base, uint32_t off)
{
	const uint32_t* a = reinterpret_cast<const uint32_t*>(base + (off & ~3u));
	const uint32_t sh = off & 3u;
	const uint32_t w0 = a[0], w1 = a[1], w2 = a[2], w3 = a[3], w4 = a[4];
	return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
	                  __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
}

// 4 bytes at any byte offset of such an array, same reason (two aligned dwords + v_alignbyte)
__device__ __forceinline__ uint32_t lds_ld32(const uint8_t* base, uint32_t off)
{
	const uint32_t* a = reinterpret_cast<const uint32_t*>(base + (off & ~3u));
	return __builtin_amdgcn_alignbyte(a[1], a[0], off & 3u);
}

// ---- per-position match results of the Xpress-family finders --------------------------------------------
// ONE 32-bit word per position: len - 3 in the low half, the offset in the high half (0 = no match). The kernels see the two halves
// as two arrays of uint16_t with a stride of two (`mlen3[i]`, `moff[i]`): a finder that stores a position's match touches ONE 4-byte
// word (the lazy finder's stores are scattered: two separate arrays cost two 32-byte sectors of HBM writes per match, 40 GB per pass of
// BASELINE configs[4]), and the parse kernels find both halves in the same cache line.
struct S16 {
	uint16_t* p;
	__host__ __device__ S16(const uint16_t* q) : p(const_cast<uint16_t*>(q)) {}
	__device__ __forceinline__ uint16_t& operator[](u64 i) const { return p[2u * i]; }
	__device__ __forceinline__ S16 operator+(u64 k) const { return S16(p + 2u * k); }
	__device__ __forceinline__ uint32_t word(u64 i) const { return *reinterpret_cast<const uint32_t*>(p + 2u * i); }   // both halves of position i (called on the LENGTH view: p is word aligned)
};

// ---- batch tables (uploaded once per plan) ------------------------------------------------------------
// unit u owns chunks [chunk_prefix[u], chunk_prefix[u+1]); input = in_off/in_len, output = out_off/out_cap.
struct BatchTables {
	const u64*      in_off;        // n_units
	const u64*      in_len;        // n_units
	const u64*      out_off;       // n_units
	const u64*      out_cap;       // n_units
	const uint32_t* chunk_prefix;  // n_units+1
	uint32_t        n_units;
	uint32_t        n_chunks;
};

// ---- the counts a plan is sized by ------------------------------------------------------------------------
// One definition for the host (plan.hip, plan_dev.hip: exact tables of host plans, bounds of dev plans) and for the table passes that build the same
// tables on the device (devplan.hip): a dev plan gives the host plan's bytes and statuses because both take their counts from here.
// `format` is the MSCompFormat value: 2 LZNT1, 3 Xpress, 4 Xpress+Huffman.
#define LZD_SEG        49152u                             // LZNT1 decompression: input bytes per segment of the header walk
#define XHC_TILE_BYTES 16384u                             // Xpress+Huffman decompression: input bytes per tile of the candidate search
// chunks of a unit of n input bytes when it is compressed: 4 KiB chunks for LZNT1, 64 KiB for the Xpress formats (Xpress: link chunks, one
// stream per unit); an empty unit has none and gets 0 bytes of output
__host__ __device__ inline u64 compress_chunk_bytes(int format) { return format == 2 ? 4096u : 65536u; }
__host__ __device__ inline u64 compress_chunks(int format, u64 n) { const u64 k = compress_chunk_bytes(format); return (n + k - 1u) / k; }
// ... and when it is decompressed: LZNT1, segments of the header walk; Xpress+Huffman, tiles of the candidate search; at least one
__host__ __device__ inline u64 decode_chunks(int format, u64 n)
{
	if (format == 2) { return n ? (n + LZD_SEG - 1u) / LZD_SEG : 1u; }
	if (format == 4) { return n ? (n + XHC_TILE_BYTES - 1u) / XHC_TILE_BYTES : 1u; }
	return 1u;
}
// token slots of a unit of `len` compressed bytes with room for `cap`: a token takes at least one input byte (Xpress; an Xpress+Huffman
// symbol at least one bit) and gives at least one output byte, and a match is cut into one more token per LZT_MAXLEN bytes; 64 slots of slack
#define LZT_MAXLEN 32766u                                 // longest match a 32-bit token holds (15 bits); longer ones are cut into pieces (xpress_decode.hip, xhuff_decode.hip)
__host__ __device__ inline u64 token_slots(int format, u64 len, u64 cap)
{
	const u64 by_in = (format == 3 ? 1u : 8u) * len + cap / 32766u + 1u;
	return (cap < by_in ? cap : by_in) + 64u;
}
// candidate chunk starts of an Xpress+Huffman unit: a chunk gives 65536 bytes and takes at least 260; a quarter more for windows that only
// look like a table
__host__ __device__ inline u64 candidate_slots(u64 len, u64 cap)
{
	const u64 by_out = cap / 65536u + 2u, by_len = len / 260u + 1u, most = by_out < by_len ? by_out : by_len;
	return most + most / 4u + 2u;
}
// ---- the optional paths of a decompress / size plan --------------------------------------------------------
// Which units take them and what they add to the path's tables: plan.hip plan_create_impl decides with these on the host, the path pass of a
// dev plan with large units (devplan.hip dv_paths_kernel) on the device, so both make the same decisions for the same per-unit values.
#define XPS_MIN_IN (512u << 10)                           // Xpress streams with at least this much input are walked by segments (xpress_decode.hip, xps_*)
#define LZG_MIN_CAP (1u << 20)                            // units with at least this much output capacity get their bytes from all CUs (lzglobal.hip), when the plan has the scratch for it
#ifndef LZG_TILE_SHIFT
#define LZG_TILE_SHIFT 13                                   // output bytes per tile of lzg_expand_kernel: 8 KiB (32 KiB tiles: expansion 0.78 -> 1.37 ms, passes 4.1 -> 4.6 ms on the 12 files)
#endif
__host__ __device__ inline bool xps_takes(u64 len) { return len >= XPS_MIN_IN; }
__host__ __device__ inline u64 xps_segments(u64 len, uint32_t seg_bytes) { return (len + seg_bytes - 1u) / seg_bytes; }
// the all-CU byte stage: 32-bit word indices, so one unit with room for 4 GiB keeps the whole batch on the block kernel
__host__ __device__ inline bool lzg_too_large(u64 cap) { return cap >= 0xFFFFFF00ull; }
__host__ __device__ inline bool lzg_takes(u64 cap) { return cap >= LZG_MIN_CAP && !lzg_too_large(cap); }
__host__ __device__ inline u64 lzg_token_blocks(int format, u64 len, u64 cap) { return (token_slots(format, len, cap) + 8191u) / 8192u; }
__host__ __device__ inline u64 lzg_tiles(u64 cap) { return (cap + (1u << LZG_TILE_SHIFT) - 1u) >> LZG_TILE_SHIFT; }
__host__ __device__ inline u64 lzg_words(u64 cap) { return cap + 64u; }
// ... and whether it pays, from the summed and the largest capacity of the units it would take: the all-CU stage costs about 22 ms per GB
// of output whatever the units are (74 ms for 192 files, 3.39 GB), the block-per-unit kernel about 1 ms per MB of the LARGEST unit as long
// as there are no more large units than CUs (51 ms for the same 192 files, whose largest is 51 MB; 60 ms for 12 of them, where the all-CU
// stage takes 5 ms). Products and quotients of doubles only: the host and the device round them alike.
__host__ __device__ inline bool lzg_pays(u64 cap_total, u64 cap_max)
{
	const double mb = 1.0 / (1 << 20), c_all = 0.022 * (double)cap_total * mb, per_cu = (double)cap_total * mb / 256.0;
	const double c_blk = 1.0 * ((double)cap_max * mb > per_cu ? (double)cap_max * mb : per_cu);
	return c_all < c_blk;
}
// Xpress+Huffman: a buffer of several chunks keeps its candidates' tokens in scratch (no second walk): scratch slots of a unit
__host__ __device__ inline u64 scratch_slots(u64 len, u64 cap) { return cap > 65536u ? candidate_slots(len, cap) : 0u; }

// the largest output of n input bytes (the reference's *_max_compressed_size), and the capacity mscomp_amd_plan_layout gives such a unit
__host__ __device__ inline u64 lznt1_max_out(u64 n)       { return n + 3u + 2u * ((n + 4095u) / 4096u); }
__host__ __device__ inline u64 xpress_max_out(u64 n)      { return n + 4u + 4u * (n / 32u); }
__host__ __device__ inline u64 xpress_huff_max_out(u64 n) { return n + 34u + 258u + 258u * (n / 65536u); }
__host__ __device__ inline u64 layout_cap(int format, u64 n)
{
	return format == 2 ? lznt1_max_out(n) + 2u            // room for the uncounted End_of_buffer
	     : format == 3 ? xpress_max_out(n) : format == 4 ? xpress_huff_max_out(n) : n;
}

// largest u with chunk_prefix[u] <= c   (uniform per block: scalar loads)
__device__ __forceinline__ uint32_t unit_of_chunk(const uint32_t* __restrict__ prefix, uint32_t n_units, uint32_t c)
{
	uint32_t lo = 0, hi = n_units;      // invariant: prefix[lo] <= c < prefix[hi]
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (prefix[mid] <= c) { lo = mid; } else { hi = mid; }
	}
	return lo;
}
// the same over a u64 prefix: largest g with prefix[g] <= c (LZNT1: the exclusive scan of the per-segment chunk counts, empty segments share an
// entry with their successor; Xpress+Huffman: the candidate slots of the units)
__device__ __forceinline__ uint32_t seg_of_flat(const u64* __restrict__ prefix, uint32_t n_seg, u64 c)
{
	uint32_t lo = 0, hi = n_seg;
	while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (prefix[mid] <= c) { lo = mid; } else { hi = mid; } }
	return lo;
}

// Plans whose tables are built on the device (DEV kernel instances): the grid is sized for the plan's bound, and a chunk at or past the batch's
// real count (chunk_prefix[n_units], written by the table pass) belongs to no unit -- unit_of_chunk would hand it to the last one
__device__ __forceinline__ bool past_real_chunks(const BatchTables& bt, uint32_t c) { return c >= bt.chunk_prefix[bt.n_units]; }

// LDS bytes [0, n) -> global dst (any alignment), one wave (the LZNT1 chunk kernel and lz_copy_kernel)
__device__ __forceinline__ void lzd_store(uint8_t* __restrict__ dst, const uint8_t* lds, uint32_t n, uint32_t lane)
{
	uint32_t head = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
	if (head > n) { head = n; }
	if (lane < head) { dst[lane] = lds[lane]; }
	const uint32_t body = (n - head) >> 2;
	uint32_t* __restrict__ d32 = reinterpret_cast<uint32_t*>(dst + head);
	for (uint32_t i = lane; i < body; i += 64u) { d32[i] = lds_ld32(lds, head + i * 4u); }
	for (uint32_t i = head + body * 4u + lane; i < n; i += 64u) { dst[i] = lds[i]; }
}

// Cooperative byte copy global->global: src is 4-byte aligned (a scratch slot), dst has any alignment.
// Body moves aligned dwords on the destination side, funnel-shifting two source dwords.
__device__ __forceinline__ void copy_from_aligned(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src,
                                                  uint32_t n, uint32_t tid, uint32_t nthr)
{
	uint32_t head = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
	if (head > n) { head = n; }
	if (tid < head) { dst[tid] = src[tid]; }
	const uint32_t body = (n - head) >> 2;
	const uint32_t* __restrict__ s32 = reinterpret_cast<const uint32_t*>(src);
	uint32_t* __restrict__ d32 = reinterpret_cast<uint32_t*>(dst + head);
	// four destination dwords per thread and step (round 5: one dword per step left ~10 dependent load -> shift -> store rounds per 2.4 KiB chunk
	// image in flight one at a time; the destination is only dword-aligned, the 16 bytes go out as the compiler sees fit for that alignment)
	const uint32_t body4 = body & ~3u;
	for (uint32_t i = tid * 4u; i < body4; i += nthr * 4u) {
		const uint32_t a0 = s32[i], a1 = s32[i + 1u], a2 = s32[i + 2u], a3 = s32[i + 3u], a4 = head ? s32[i + 4u] : 0u;   // (index <= body, like the one-dword form's s32[i + 1]: at most 3 bytes behind the image, inside the slot's slack)
		uint32_t v[4];
		if (head == 0) { v[0] = a0; v[1] = a1; v[2] = a2; v[3] = a3; }
		else { v[0] = __builtin_amdgcn_alignbyte(a1, a0, head); v[1] = __builtin_amdgcn_alignbyte(a2, a1, head); v[2] = __builtin_amdgcn_alignbyte(a3, a2, head); v[3] = __builtin_amdgcn_alignbyte(a4, a3, head); }
		__builtin_memcpy(__builtin_assume_aligned(d32 + i, 4), v, 16);
	}
	if (head == 0) {
		for (uint32_t i = body4 + tid; i < body; i += nthr) { d32[i] = s32[i]; }
	} else {
		for (uint32_t i = body4 + tid; i < body; i += nthr) { d32[i] = __builtin_amdgcn_alignbyte(s32[i + 1], s32[i], head); }
	}
	for (uint32_t i = head + body * 4u + tid; i < n; i += nthr) { dst[i] = src[i]; }
}

// ---- shared by devplan.hip and blocks.hip: the table passes' block scan, and the 16-byte-lane copy of compaction ----
#define DV_THREADS 1024u
#define DV_WAVES   (DV_THREADS / 64u)

__device__ __forceinline__ u64 sat_add(u64 a, u64 b) { const u64 s = a + b; return s < a ? ~(u64)0 : s; }

// Inclusive scan of K values per thread over the block (saturating add: associative, so the order of the partial sums does not matter),
// continued from carry; carry becomes carry + the tile's total in every thread.
template <int K>
__device__ __forceinline__ void dv_block_scan(u64 (&v)[K], u64 (&carry)[K], u64 (*s_w)[DV_WAVES])
{
	const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
	#pragma unroll
	for (int k = 0; k < K; ++k) {
		#pragma unroll
		for (uint32_t d = 1; d < 64u; d <<= 1) { const u64 o = __shfl_up(v[k], d, 64); if (lane >= d) { v[k] = sat_add(v[k], o); } }
		if (lane == 63u) { s_w[k][w] = v[k]; }
	}
	__syncthreads();
	#pragma unroll
	for (int k = 0; k < K; ++k) {
		u64 before = carry[k], tot = carry[k];
		for (uint32_t i = 0; i < DV_WAVES; ++i) { if (i < w) { before = sat_add(before, s_w[k][i]); } tot = sat_add(tot, s_w[k][i]); }
		v[k] = sat_add(v[k], before);
		carry[k] = tot;
	}
	__syncthreads();
}

// inclusive running maximum over the block, continued from carry; carry becomes the maximum over everything so far in every thread
// (diff.hip, match.hip: the row that starts the run a row ends)
__device__ __forceinline__ void dv_block_max(u64& v, u64& carry, u64* s_m)
{
	const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
	#pragma unroll
	for (uint32_t d = 1; d < 64u; d <<= 1) { const u64 o = __shfl_up(v, d, 64); if (lane >= d && o > v) { v = o; } }
	if (lane == 63u) { s_m[w] = v; }
	__syncthreads();
	u64 before = carry, tot = carry;
	for (uint32_t i = 0; i < DV_WAVES; ++i) { const u64 x = s_m[i]; if (i < w && x > before) { before = x; } if (x > tot) { tot = x; } }
	if (before > v) { v = before; }
	carry = tot;
	__syncthreads();
}

// largest r with first[r] <= b (first[0] = 0 <= b < first[n]): the resource that holds block b of a block container, or the request that
// holds unit b of a block reader; empty ones in front of it are skipped (blocks.hip, reader.hip)
__device__ __forceinline__ uint32_t res_of_block(const u64* __restrict__ first, uint32_t n, u64 b)
{
	uint32_t lo = 0, hi = n;
	while (hi - lo > 1) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (first[mid] <= b) { lo = mid; } else { hi = mid; }
	}
	return lo;
}

#define CPD_THREADS 256u
struct __attribute__((packed)) cpd_u16 { uint32_t w[4]; };  // 16 bytes of alignment 1

template <bool ZERO>
__device__ __forceinline__ void cpd_move(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, u64 cnt, uint32_t tid)
{
	u64 head = (16u - ((uintptr_t)dst & 15u)) & 15u;
	if (head > cnt) { head = cnt; }
	const u64 body = (cnt - head) >> 4, tail0 = head + body * 16u;
	const bool has_head = tid < head, has_tail = tid >= 64u && tail0 + (tid - 64u) < cnt;   // (the tail on the second wave: at most 15 bytes)
	uint4* __restrict__ d16 = reinterpret_cast<uint4*>(dst + head);
	if (ZERO) {
		if (has_head) { dst[tid] = 0; }
		if (has_tail) { dst[tail0 + (tid - 64u)] = 0; }
		for (u64 k = tid; k < body; k += CPD_THREADS) { d16[k] = make_uint4(0, 0, 0, 0); }
		return;
	}
	// every load of a step before its stores: a piece of up to 16 KiB + 30 bytes costs one round trip to memory, not one per access
	const uint8_t hb = has_head ? src[tid] : (uint8_t)0, tb = has_tail ? src[tail0 + (tid - 64u)] : (uint8_t)0;
	const bool same = (((uintptr_t)src + head) & 15u) == 0;              // source and destination aligned alike: 16-byte loads
	const uint4* __restrict__ sa = reinterpret_cast<const uint4*>(src + head);
	const cpd_u16* __restrict__ su = reinterpret_cast<const cpd_u16*>(src + head);
	for (u64 k0 = 0; k0 < body || k0 == 0; k0 += 4u * CPD_THREADS) {
		uint4 v[4];
		#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) {
			const u64 k = k0 + j * CPD_THREADS + tid;
			if (k < body) {
				if (same) { v[j] = sa[k]; }
				else { const cpd_u16 t = su[k]; v[j] = make_uint4(t.w[0], t.w[1], t.w[2], t.w[3]); }
			}
		}
		if (k0 == 0) {
			if (has_head) { dst[tid] = hb; }
			if (has_tail) { dst[tail0 + (tid - 64u)] = tb; }
		}
		#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) {
			const u64 k = k0 + j * CPD_THREADS + tid;
			if (k < body) { d16[k] = v[j]; }
		}
	}
}

#define DD_PIECE_SHIFT 14u                                 // the confirm passes of dedup and diff compare in pieces of 16 KiB, as the raw copy and the gather move
#define DD_SLICE_MIN   6u                                  // ... and a block takes six pieces at least: what it looks up per row is paid once per 96 KiB or less

// Shared by dedup.hip and diff.hip. Whether the cnt bytes at a and at b differ, by NT threads (NT >= 128): the two sides have independent
// alignment -- stored blocks are packed without padding --, so, as cpd_move moves them, a bytewise head up to a's next 16-byte boundary,
// a body of 16-byte loads on a (16-byte loads on b too where it is aligned alike, loads of alignment 1 otherwise, four of either side in
// flight per thread), a bytewise tail on the second wave. The answer is this thread's part: the caller folds it.
template <uint32_t NT>
__device__ __forceinline__ bool cpd_differs(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, u64 cnt, uint32_t tid)
{
	u64 head = (16u - ((uintptr_t)a & 15u)) & 15u;
	if (head > cnt) { head = cnt; }
	const u64 body = (cnt - head) >> 4, tail0 = head + body * 16u;
	bool d = false;
	if (tid < head) { d = a[tid] != b[tid]; }
	if (tid >= 64u && tail0 + (tid - 64u) < cnt) { d = d || a[tail0 + (tid - 64u)] != b[tail0 + (tid - 64u)]; }
	const bool same = (((uintptr_t)b + head) & 15u) == 0;
	const uint4* __restrict__ pa = reinterpret_cast<const uint4*>(a + head);
	const uint4* __restrict__ pb = reinterpret_cast<const uint4*>(b + head);
	const cpd_u16* __restrict__ ub = reinterpret_cast<const cpd_u16*>(b + head);
	for (u64 k0 = 0; k0 < body; k0 += 4u * NT) {
		uint4 x[4], y[4];
		#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) {
			const u64 k = k0 + j * NT + tid;
			x[j] = y[j] = make_uint4(0, 0, 0, 0);
			if (k < body) {
				x[j] = pa[k];
				if (same) { y[j] = pb[k]; }
				else { const cpd_u16 t = ub[k]; y[j] = make_uint4(t.w[0], t.w[1], t.w[2], t.w[3]); }
			}
		}
		#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) { d = d || ((x[j].x ^ y[j].x) | (x[j].y ^ y[j].y) | (x[j].z ^ y[j].z) | (x[j].w ^ y[j].w)) != 0; }
	}
	return d;
}

// ---- shared by reader.hip and writer.hip: the action word of a unit, the piece of the byte-moving passes, and one wave's move ----
#define RD_SKIP   0u                                      // not an owner (or no unit at all): nothing to decode, read or check
#define RD_COPY   1u                                      // a raw block: read in d_packed
#define RD_DECODE 2u                                      // decoded into its cache slot
#define RD_FAIL   3u                                      // failed a table check: never read (the action word of a unit: kind | data length << 2)
#define RD_PIECE_SHIFT 14u                                // the gather and the patch move their bytes in pieces of 16 KiB

// cnt <= 16 KiB bytes by one wave, as cpd_move moves a piece by a block: a bytewise head up to the destination's next 16-byte boundary
// (lanes 0..14), a body of 16-byte stores (16-byte loads where the source is aligned alike, loads of alignment 1 otherwise, four in flight
// per lane), a bytewise tail (lanes 16..30). No byte outside the two ranges is touched.
__device__ __forceinline__ void rd_wave_move(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t cnt, uint32_t lane)
{
	uint32_t head = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
	if (head > cnt) { head = cnt; }
	const uint32_t body = (cnt - head) >> 4, tail0 = head + body * 16u;
	const bool has_head = lane < head, has_tail = lane >= 16u && tail0 + (lane - 16u) < cnt;
	const uint8_t hb = has_head ? src[lane] : (uint8_t)0, tb = has_tail ? src[tail0 + (lane - 16u)] : (uint8_t)0;
	const bool same = (((uintptr_t)src + head) & 15u) == 0;
	uint4* __restrict__ d16 = reinterpret_cast<uint4*>(dst + head);
	const uint4* __restrict__ sa = reinterpret_cast<const uint4*>(src + head);
	const cpd_u16* __restrict__ su = reinterpret_cast<const cpd_u16*>(src + head);
	for (uint32_t k0 = 0; k0 < body || k0 == 0; k0 += 4u * 64u) {
		uint4 v[4];
		#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) {
			const uint32_t k = k0 + j * 64u + lane;
			if (k < body) {
				if (same) { v[j] = sa[k]; }
				else { const cpd_u16 x = su[k]; v[j] = make_uint4(x.w[0], x.w[1], x.w[2], x.w[3]); }
			}
		}
		if (k0 == 0) {
			if (has_head) { dst[lane] = hb; }
			if (has_tail) { dst[tail0 + (lane - 16u)] = tb; }
		}
		#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) {
			const uint32_t k = k0 + j * 64u + lane;
			if (k < body) { d16[k] = v[j]; }
		}
	}
}

} // namespace msc
