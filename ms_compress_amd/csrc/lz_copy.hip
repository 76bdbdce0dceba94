// lz_copy.hip -- tokens -> bytes, the last stage of the gfx950 Xpress and Xpress+Huffman decompressors (the 32-bit tokens come
// from xpress_decode.hip / xhuff_decode.hip; the units of LZG_MIN_CAP and more go to all CUs, lzglobal.hip, when the plan has that stage).
//   lz_copy_kernel        a wave per unit, 64 bytes at a time (sources chased with ds_bpermute / LDS / HBM)       [comments at the kernels]
//   lz_copy_block_kernel  a block per unit of LZB_MIN_KB and more, 8 KiB at a time
#include "kernels.h"
#include "host.h"

namespace msc {

// The output of a unit is produced 2048 bytes at a time. The tokens that start in the window set a bit per start and leave their
// word at that position; then 64 bytes at a time find their token (highest start at or below them; the token running when the
// row begins is carried in registers), hence their source: a literal, or byte (i - s) mod off of the match's first period. A
// source in an earlier window is read back from HBM, one in an earlier row of the window from LDS, one in the same row is chased
// with ds_bpermute pointer jumping (as in the LZNT1 chunk kernel).
#define LZC_W 2048u
struct LzcLds { __attribute__((aligned(16))) uint8_t win[LZC_W + 64]; uint32_t info[LZC_W]; u64 bm[LZC_W / 64u]; };

// The capacity from which a unit is left to lzglobal.hip: a value the host knows (host plans; plain dev plans: none), or -- DEV, a dev plan with
// large units -- LZG_MIN_CAP when this execution's path pass left units on that stage (its count, in device memory), none otherwise
template <bool DEV> struct LzgMin { u64 v; __device__ __forceinline__ u64 get() const { return v; } };
template <> struct LzgMin<true> { const uint32_t* cnt; __device__ __forceinline__ u64 get() const { return cnt[0] ? (u64)LZG_MIN_CAP : ~(u64)0; } };

template <bool DEV>
__global__ __launch_bounds__(64) void lz_copy_kernel(BatchTables bt, const u64* __restrict__ tok_prefix, const uint32_t* __restrict__ tok,
                                                    const u64* __restrict__ ntok, const u64* __restrict__ d_out_len, const int32_t* __restrict__ d_status,
                                                    uint8_t* __restrict__ d_out, uint32_t lzb_min, LzgMin<DEV> lzg_min_cap)
{
	__shared__ LzcLds L;
	const uint32_t lane = threadIdx.x, u = blockIdx.x;
	if (d_status[u] != 0 || bt.out_cap[u] >= lzg_min_cap.get()) { return; }   // (units with that much room: lzglobal.hip)
	const u64 total = d_out_len[u], nt = ntok[u];
	if (total >= lzb_min) { return; }                                    // larger units: lz_copy_block_kernel
	const uint32_t* __restrict__ mytok = tok + tok_prefix[u];
	uint8_t* dst = d_out + bt.out_off[u];
	u64 t = 0, tpos = 0;                                                 // next token to place, its output offset
	u64 cur_s = 0; uint32_t cur_w = 0x80000000u;                         // the token running at the current position
	for (u64 w0 = 0; w0 < total; w0 += LZC_W) {
		const uint32_t wlen = total - w0 < LZC_W ? (uint32_t)(total - w0) : LZC_W;
		if (lane < LZC_W / 64u) { L.bm[lane] = 0; }
		__syncthreads();
		// ---- the tokens that start in this window ----
		while (t < nt && tpos < w0 + wlen) {
			const u64 ti = t + lane;
			const uint32_t w = ti < nt ? mytok[ti] : 0x80000000u;
			const uint32_t len = ti < nt ? ((w & 0x80000000u) ? 1u : (w >> 16) & 0x7FFFu) : 0u;
			const uint32_t incl = wave_incl_scan_add_u32(len);
			const u64 p = tpos + incl - len;
			const bool in = ti < nt && p < w0 + wlen;
			if (in) {
				const uint32_t q = (uint32_t)(p - w0);
				L.info[q] = w;
				atomicOr(reinterpret_cast<uint32_t*>(L.bm) + (q >> 5), 1u << (q & 31u));
			}
			const uint32_t k = (uint32_t)__builtin_popcountll(__ballot(in));     // a prefix of the lanes
			t += k;
			tpos += k == 64u ? (uint32_t)__builtin_amdgcn_readlane((int)incl, 63) : (uint32_t)__builtin_amdgcn_readlane((int)incl, (int)(k ? k - 1u : 0u)) * (k ? 1u : 0u);
			if (k < 64u) { break; }
		}
		__syncthreads();
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");               // earlier windows of this unit are read back from HBM
		// ---- bytes ----
		for (uint32_t rowbase = 0; rowbase < wlen; rowbase += 64u) {
			const u64 word = L.bm[rowbase >> 6];
			const u64 i = w0 + rowbase + lane;
			const u64 mine = word & ((2ull << lane) - 1ull);
			const u64 s = mine ? w0 + rowbase + 63u - (uint32_t)__builtin_clzll(mine) : cur_s;
			const uint32_t inf = mine ? L.info[(uint32_t)(s - w0)] : cur_w;
			if (word) { cur_s = w0 + rowbase + 63u - (uint32_t)__builtin_clzll(word); cur_w = L.info[(uint32_t)(cur_s - w0)]; }
			const bool lit = (inf & 0x80000000u) != 0;
			uint32_t val = inf & 0xFFu;
			const uint32_t rowend = rowbase + 64u < wlen ? 64u : wlen - rowbase;
			bool resolved = lit || lane >= rowend;
			uint32_t ptr = lane;                                         // in-row source lane while unresolved
			if (!resolved) {
				const uint32_t off = inf & 0xFFFFu, dd = (uint32_t)(i - s);
				uint32_t rem = dd;
				if (dd >= off) {
					const uint32_t q = (uint32_t)((float)dd * __builtin_amdgcn_rcpf((float)off));
					int32_t rr = (int32_t)dd - (int32_t)(q * off);
					if (rr < 0) { rr += (int32_t)off; } else if (rr >= (int32_t)off) { rr -= (int32_t)off; }
					rem = (uint32_t)rr;
				}
				const u64 sp = s - off + rem;                            // absolute source position, < s
				if (sp >= w0 + rowbase) { ptr = (uint32_t)(sp - (w0 + rowbase)); }
				else if (sp >= w0) { val = L.win[(uint32_t)(sp - w0)]; resolved = true; }
				else { val = dst[sp]; resolved = true; }
			}
			while (__ballot(!resolved)) {
				const uint32_t tl = resolved ? lane : ptr;
				const uint32_t tv = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(tl << 2), (int)(val | (resolved ? 0x100u : 0u)));
				const uint32_t tp = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(tl << 2), (int)ptr);
				if (!resolved) { if (tv & 0x100u) { val = tv & 0xFFu; resolved = true; } else { ptr = tp; } }
			}
			L.win[rowbase + lane] = (uint8_t)val;
			__syncthreads();
		}
		lzd_store(dst + w0, L.win, wlen, lane);
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
		__syncthreads();
	}
}


// ---- the same for a LARGE unit: one block of 1024 threads, 8 KiB of output at a time -------------------------------------------------
// lz_copy_kernel walks the output of a unit with one wave (0.4 GB/s: 539 of the 665 ms the 12 files of the bench corpus took as 12 buffers).
// Here a tile of 8192 output bytes is resolved by the whole block: the tokens that start in the tile are placed 1024 at a time (block scan
// of their lengths), every byte finds its token (start bits + a per-word "last start so far" from a block max-scan) and its source one
// match offset back -- in the last 64 KiB of output, kept in an LDS ring (offsets reach at most 65535 back: resolved), or inside the tile
// (a pointer); pointers are then jumped (ptr = ptr[ptr], at most 13 rounds, usually 2-4) until every byte has its value. One word per byte
// holds "value" or "pointer", so a racing read sees one or the other, both of which are right.
#define LZB_T    8192u
#ifndef LZB_NT
#define LZB_NT   1024u
#endif
#define LZB_RING 73728u                                            // 65536 + LZB_T, a multiple of LZB_T: a tile never wraps
struct LzbLds {
	__attribute__((aligned(16))) uint8_t ring[LZB_RING];
	uint32_t info[LZB_T];                                          // token word at its start position; later: 0x80000000 | value, or the in-tile source
	uint32_t bm[LZB_T / 32u];
	uint32_t last[LZB_T / 32u];                                    // highest token start in the words before this one (LZB_T = none in this tile)
	uint32_t wsum[16];
	uint32_t carry[4];                                             // tpos (2 words), token running at the tile start: its position relative to the tile (biased), its word
	uint32_t tokbuf[LZB_T + LZB_T / 64u];                          // the next LZB_T tokens of the unit (a tile cannot start more): fetched while the tile before is resolved
};

#ifdef LZB_PROFILE
__device__ unsigned long long g_lzb_prof[8];
extern "C" void mscomp_amd_debug_lzb_prof(unsigned long long* out) { (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lzb_prof), 64); unsigned long long z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_lzb_prof), z, 64); }
#define LZB_TM(i) { const unsigned long long t_ = __builtin_readcyclecounter(); if (tid == 0) { atomicAdd(&g_lzb_prof[i], t_ - lzb_prev); } lzb_prev = t_; }
#define LZB_CN(i, v) { if (tid == 0) { atomicAdd(&g_lzb_prof[i], (unsigned long long)(v)); } }
#else
#define LZB_TM(i)
#define LZB_CN(i, v)
#endif
static PerDeviceOnce g_lzb_attr;                                          // the dynamic-LDS attribute of lz_copy_block_kernel, per device (two launch sites)
template <bool DEV>
__global__ __launch_bounds__(LZB_NT) void lz_copy_block_kernel(BatchTables bt, const u64* __restrict__ tok_prefix, const uint32_t* __restrict__ tok,
                                                              const u64* __restrict__ ntok, const u64* __restrict__ d_out_len, const int32_t* __restrict__ d_status,
                                                              uint8_t* __restrict__ d_out, uint32_t lzb_min, LzgMin<DEV> lzg_min_cap)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t lzb_smem[];
	LzbLds& L = *reinterpret_cast<LzbLds*>(lzb_smem);
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6, u = blockIdx.x;
	if (d_status[u] != 0 || bt.out_cap[u] >= lzg_min_cap.get()) { return; }   // (units with that much room: lzglobal.hip)
	const u64 total = d_out_len[u], nt = ntok[u];
	if (total < lzb_min) { return; }
	const uint32_t* __restrict__ mytok = tok + tok_prefix[u];
	uint8_t* __restrict__ dst = d_out + bt.out_off[u];
	u64 t = 0, tpos = 0;                                             // next token to place, its output offset (uniform)
	uint32_t run_w = 0x80000000u;                                    // the token running at the tile start
	uint32_t rbase = 0;                                              // the tile's place in the ring (w0 mod LZB_RING)
	uint32_t pre[LZB_T / LZB_NT];                                    // tokens t + r * 1024 + tid, on their way from HBM
	#pragma unroll
	for (uint32_t r = 0; r < LZB_T / LZB_NT; ++r) { const u64 ti = (u64)r * LZB_NT + tid; pre[r] = ti < nt ? mytok[ti] : 0x80000000u; }
#ifdef LZB_PROFILE
	unsigned long long lzb_prev = __builtin_readcyclecounter();
#endif
	for (u64 w0 = 0; w0 < total; w0 += LZB_T) {
		const uint32_t wlen = total - w0 < LZB_T ? (uint32_t)(total - w0) : LZB_T;
		LZB_CN(6, 1)
		if (tid < LZB_T / 32u) { L.bm[tid] = 0; }
		if (tid == 0) { L.carry[0] = 0; L.carry[3] = 0; }
		#pragma unroll
		for (uint32_t r = 0; r < LZB_T / LZB_NT; ++r) { const uint32_t i_ = r * LZB_NT + tid; L.tokbuf[i_ + (i_ >> 6)] = pre[r]; }   // (one word of padding per 64: the reads below, 8 words apart from lane to lane, meet no bank twice)
		__syncthreads();
		// ---- the tokens that start in this tile: a tile cannot start more than LZB_T, thread j looks at tokens 8 j .. 8 j + 7 of the buffer ----
		if (t < nt && tpos < w0 + wlen) {
			constexpr uint32_t TPT = LZB_T / LZB_NT;                     // tokens per thread
			uint32_t w[TPT], len[TPT], sum = 0;
			#pragma unroll
			for (uint32_t r = 0; r < TPT; ++r) {
				w[r] = L.tokbuf[tid * TPT + r + ((tid * TPT + r) >> 6)];
				len[r] = (t + tid * TPT + r < nt) ? ((w[r] & 0x80000000u) ? 1u : (w[r] >> 16) & 0x7FFFu) : 0u;
				sum += len[r];
			}
			const uint32_t incl = wave_incl_scan_add_u32(sum);
			if (lane == 63u) { L.wsum[wv] = incl; }
			__syncthreads();
			uint32_t base = 0;
			for (uint32_t k = 0; k < wv; ++k) { base += L.wsum[k]; }
			u64 p = tpos + base + incl - sum;
			uint32_t cnt = 0; u64 after = 0;
			uint32_t accw = 0xFFFFFFFFu, accb = 0;                        // start bits of my tokens, collected per 32-position word (8 atomics on a shared word cost 15 000 cycles per tile)
			#pragma unroll
			for (uint32_t r = 0; r < TPT; ++r) {
				if (t + tid * TPT + r < nt && p < w0 + wlen) {
					const uint32_t q = (uint32_t)(p - w0);
					L.info[q] = w[r];
					if ((q >> 5) != accw) { if (accb) { atomicOr(&L.bm[accw], accb); } accw = q >> 5; accb = 0; }
					accb |= 1u << (q & 31u);
					++cnt; after = p + len[r];
				}
				p += len[r];
			}
			if (accb) { atomicOr(&L.bm[accw], accb); }
			// the tokens placed are a prefix of the buffer; the end of the last one is where the next token starts
			{	// one update per wave (a thousand updates of one word are served one after the other)
				const uint32_t cw = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_add_u32(cnt), 63);
				const uint32_t aw = wave_max_u32(cnt ? (uint32_t)(after - w0) : 0u);
				if (lane == 0 && cw) { atomicAdd(&L.carry[3], cw); atomicMax(&L.carry[0], aw); }
			}
			__syncthreads();
			const uint32_t placed = L.carry[3];
			if (placed) { t += placed; tpos = w0 + L.carry[0]; }
		}
		__syncthreads();
		#pragma unroll
		for (uint32_t r = 0; r < LZB_T / LZB_NT; ++r) { const u64 ti = t + (u64)r * LZB_NT + tid; pre[r] = ti < nt ? mytok[ti] : 0x80000000u; }   // (for the next tile)
		__syncthreads();
		LZB_TM(0)
		// ---- per 32-position word: the highest token start before it (block max-scan over 256 words) ----
		if (tid < LZB_T / 32u) {
			const uint32_t wd = L.bm[tid];
			const uint32_t hi = wd ? tid * 32u + 31u - (uint32_t)__builtin_clz(wd) + 1u : 0u;      // biased by 1: 0 = no start in this word
			const uint32_t incl = wave_incl_scan_max(hi);
			if (lane == 63u) { L.wsum[wv] = incl; }
			L.last[tid] = incl;                                         // (inclusive for now)
		}
		__syncthreads();
		if (tid < LZB_T / 32u) {
			uint32_t before = 0;
			for (uint32_t k = 0; k < wv; ++k) { before = before > L.wsum[k] ? before : L.wsum[k]; }
			const uint32_t incl = L.last[tid] > before ? L.last[tid] : before;
			const uint32_t mine = L.bm[tid] ? tid * 32u + 31u - (uint32_t)__builtin_clz(L.bm[tid]) + 1u : 0u;
			// exclusive: the maximum over the words before this one
			const uint32_t prev_lane = (uint32_t)__shfl_up((int)incl, 1, 64);
			uint32_t excl = lane ? prev_lane : before;
			(void)mine;
			L.wsum[4u + 0u] = 0;                                        // (keeps the slot initialised)
			L.last[tid] = excl;                                         // biased start position, 0 = none before this word in the tile
			if (tid == LZB_T / 32u - 1u) { L.carry[2] = incl; }        // the last start of the tile (biased; 0 = none)
		}
		__syncthreads();
		LZB_TM(1)
		// ---- bytes: value, or where in the tile the value comes from (32-bit, relative to the tile) ----
		uint32_t myw[LZB_T / LZB_NT];
		#pragma unroll
		for (uint32_t r = 0; r < LZB_T / LZB_NT; ++r) {
			const uint32_t q = r * LZB_NT + tid;
			uint32_t word = 0x80000000u;
			if (q < wlen) {
				const uint32_t bits = L.bm[q >> 5] & (0xFFFFFFFFu >> (31u - (q & 31u)));
				const uint32_t sb = bits ? (q & ~31u) + 32u - (uint32_t)__builtin_clz(bits) : L.last[q >> 5];   // biased start of my token (0: it runs since before the tile)
				const uint32_t inf = sb ? L.info[sb - 1u] : run_w;
				if (inf & 0x80000000u) { word = 0x80000000u | (inf & 0xFFu); }
				else {
					const int32_t rel = (int32_t)q - (int32_t)(inf & 0xFFFFu);     // one offset back: the same byte
					if (rel >= 0) { word = (uint32_t)rel; }
					else { const int32_t ri = (int32_t)rbase + rel; word = 0x80000000u | L.ring[ri < 0 ? ri + (int32_t)LZB_RING : ri]; }
				}
			}
			myw[r] = word;
		}
		// the token running when the next tile begins
		const uint32_t lastb = L.carry[2];
		if (lastb) { run_w = L.info[lastb - 1u]; }
		__syncthreads();
		#pragma unroll
		for (uint32_t r = 0; r < LZB_T / LZB_NT; ++r) { L.info[r * LZB_NT + tid] = myw[r]; }
		__syncthreads();
		LZB_TM(2)
		for (;;) {
			LZB_CN(7, 1)
			bool open = false;
			#pragma unroll
			for (uint32_t r = 0; r < LZB_T / LZB_NT; ++r) {
				const uint32_t q = r * LZB_NT + tid;
				uint32_t mine = myw[r];
				if (!(mine & 0x80000000u)) {
					uint32_t tw = __hip_atomic_load(&L.info[mine], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					if (!(tw & 0x80000000u)) { tw = __hip_atomic_load(&L.info[tw], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }   // (two hops per round: half the barriers)
					mine = tw;                                              // its value, or where IT looks
					myw[r] = mine;
					__hip_atomic_store(&L.info[q], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
					open |= !(mine & 0x80000000u);
				}
			}
			if (!__syncthreads_or(open ? 1 : 0)) { break; }
		}
		LZB_TM(3)
		// ---- the tile: into the ring and out ----
		#pragma unroll
		for (uint32_t r = 0; r < LZB_T / LZB_NT; ++r) { const uint32_t q = r * LZB_NT + tid; if (q < wlen) { L.ring[rbase + q] = (uint8_t)myw[r]; } }
		__syncthreads();
		{
			uint8_t* __restrict__ o = dst + w0;
			const uint8_t* src = L.ring + rbase;
			uint32_t head = (uint32_t)((4u - ((uintptr_t)o & 3u)) & 3u);
			if (head > wlen) { head = wlen; }
			if (tid < head) { o[tid] = src[tid]; }
			const uint32_t body = (wlen - head) >> 2;
			uint32_t* __restrict__ o32 = reinterpret_cast<uint32_t*>(o + head);
			for (uint32_t k = tid; k < body; k += LZB_NT) { o32[k] = lds_ld32(src, head + k * 4u); }
			for (uint32_t k = head + body * 4u + tid; k < wlen; k += LZB_NT) { o[k] = src[k]; }
		}
		rbase += LZB_T; if (rbase >= LZB_RING) { rbase -= LZB_RING; }
		__syncthreads();
		LZB_TM(4)
	}
}

void prepare_lz_copy_block()
{
	if (!g_lzb_attr.needed()) { return; }
	(void)hipFuncSetAttribute(reinterpret_cast<const void*>(lz_copy_block_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(LzbLds));
	(void)hipFuncSetAttribute(reinterpret_cast<const void*>(lz_copy_block_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(LzbLds));
	g_lzb_attr.done();
}
// lzg_cnt: a dev plan with large units (the DEV instances read the stage's count of this execution there); lzg_min_cap: every other plan
void launch_lz_copy(hipStream_t st, const BatchTables& bt, const u64* tok_prefix, const uint32_t* tok, const u64* ntok, const u64* d_out_len, const int32_t* d_status, uint8_t* d_out, u64 lzg_min_cap, const uint32_t* lzg_cnt)
{
	if (bt.n_units == 0) { return; }
	prepare_lz_copy_block();
	if (lzg_cnt) { hipLaunchKernelGGL(lz_copy_kernel<true>, dim3(bt.n_units), dim3(64), 0, st, bt, tok_prefix, tok, ntok, d_out_len, d_status, d_out, env_lzb_min_bytes(), LzgMin<true>{ lzg_cnt }); }
	else { hipLaunchKernelGGL(lz_copy_kernel<false>, dim3(bt.n_units), dim3(64), 0, st, bt, tok_prefix, tok, ntok, d_out_len, d_status, d_out, env_lzb_min_bytes(), LzgMin<false>{ lzg_min_cap }); }
}
void launch_lz_copy_block(hipStream_t st, const BatchTables& bt, const u64* tok_prefix, const uint32_t* tok, const u64* ntok, const u64* d_out_len, const int32_t* d_status, uint8_t* d_out, u64 lzg_min_cap, const uint32_t* lzg_cnt)
{
	if (bt.n_units == 0) { return; }
	prepare_lz_copy_block();
	if (lzg_cnt) { hipLaunchKernelGGL(lz_copy_block_kernel<true>, dim3(bt.n_units), dim3(LZB_NT), sizeof(LzbLds), st, bt, tok_prefix, tok, ntok, d_out_len, d_status, d_out, env_lzb_min_bytes(), LzgMin<true>{ lzg_cnt }); }
	else { hipLaunchKernelGGL(lz_copy_block_kernel<false>, dim3(bt.n_units), dim3(LZB_NT), sizeof(LzbLds), st, bt, tok_prefix, tok, ntok, d_out_len, d_status, d_out, env_lzb_min_bytes(), LzgMin<false>{ lzg_min_cap }); }
}

} // namespace msc
