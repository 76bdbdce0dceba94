// match_digest.hip -- the three passes of a block deduper made for match by digest that are its own (mscomp_amd_deduper_create_match_digest /
// _match_digest, include/mscomp_amd_match_digest.h): keys, confirm and settle with equality decided by a row's data length and the 16 bytes
// at its row of its view's digest column (digest.hip writes such a column over the blocks' DATA), so that no stored byte is read -- packed
// may be null -- and views of different codecs meet in one call. Everything else of the call is match's, launched as it is (match.hip:
// seed, tile, runs, counts; dedup.hip: the key table's clear, rule 3): the numbering, the key table (rowpass.h kt_*), the settle of the
// refuted (settle_refuted), the tiled run passes. The views travel as match's, one SpliceSrc by value; their digest columns beside them,
// one DigestCols by value that a lane indexes with its view. DESIGN.md 4.25.
#include "rowpass.h"

namespace msc {

// Row u of the numbering, of an accepted resource x: its data length and its digest -- ONE aligned 16-byte load from its view's column, at
// the table row first[r] + k (< v.nbt: rule 1; the column has 4 v.nbt words)
struct MdRow {
	u64 e;
	uint4 d;
};
__device__ __forceinline__ MdRow md_row_of(const SpliceSrc& src, const DigestCols& cols, uint32_t x, uint32_t shift, const u64* __restrict__ ufirst, u64 u)
{
	u64 s, r;
	dd_locate(src, x, s, r);
	const SpliceView& v = sp_view(src, s);
	const u64 k = u - ufirst[x], j = v.first[r] + k;
	const u64 L = v.res_len[r] - (k << shift), B = (u64)1 << shift;            // (k is a block of the resource: rule 2)
	return MdRow{ L < B ? L : B, reinterpret_cast<const uint4*>(cols.c[s])[j] };
}
__device__ __forceinline__ bool md_same(const MdRow& a, const MdRow& b)
{
	return a.e == b.e && ((a.d.x ^ b.d.x) | (a.d.y ^ b.d.y) | (a.d.z ^ b.d.z) | (a.d.w ^ b.d.w)) == 0;   // (one test of all four words: the load stays one)
}

// Keys, a fixed grid dealt over the rows, a lane per row (mt_keys_kernel): a row of an accepted resource mixes its key tuple -- data
// length, digest words h0 and h1 -- into 64 bits, claims the key's slot of the key table and puts its number into the slot's minimum. A row
// of a refused resource has no slot and its digest is not read; neither has one whose walk found no slot: it is its own representative.
// (The key uses two of the four words, and the compiler narrows this pass's load to those 8 bytes.)
__global__ __launch_bounds__(256) void md_keys_kernel(SpliceSrc src, DigestCols cols, uint32_t n, uint32_t shift, KeyTable kt,
                                                     const u64* __restrict__ ufirst, const int32_t* __restrict__ status,
                                                     uint32_t* __restrict__ slot_of, uint32_t* __restrict__ flag)
{
	const u64 units = ufirst[n];
	for (u64 u = (u64)blockIdx.x * 256u + threadIdx.x; u < units; u += (u64)gridDim.x * 256u) {
		const uint32_t x = res_of_block(ufirst, n, u);
		uint32_t slot = KT_NONE;
		if (status[x] == 0) {
			const MdRow a = md_row_of(src, cols, x, shift, ufirst, u);
			const u64 h = dd_mix(dd_mix(a.e ^ 0x9E3779B97F4A7C15ull) ^ ((u64)a.d.x | (u64)a.d.y << 32));
			slot = kt_claim(kt, h, dd_mix(kt_key(h)) % kt.slots);
			if (slot != KT_NONE) { atomicMin(&kt.min[slot], (uint32_t)u); }
		}
		slot_of[u] = slot; flag[u] = 0;
	}
}

// Confirm, a fixed grid dealt over the rows, a lane per row: the representative the tables give -- the slot's smallest row, or the row
// itself where it has no smaller one -- into rep, and the row's flag set where it is not EQUAL to that candidate: the data lengths and the
// 16 bytes of digest. No pass over data.
__global__ __launch_bounds__(256) void md_confirm_kernel(SpliceSrc src, DigestCols cols, uint32_t n, uint32_t shift, const u64* __restrict__ ufirst,
                                                        const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ tmin,
                                                        uint32_t* __restrict__ flag, uint32_t* __restrict__ rep)
{
	const u64 units = ufirst[n];
	for (u64 u = (u64)blockIdx.x * 256u + threadIdx.x; u < units; u += (u64)gridDim.x * 256u) {
		const uint32_t slot = slot_of[u];
		const uint32_t c = slot == KT_NONE ? (uint32_t)u : tmin[slot];         // (no slot: a refused resource, no digest of it is read)
		const bool cand = c < u;                                               // (c > u: a damaged table; the row stands for itself)
		rep[u] = cand ? c : (uint32_t)u;
		if (!cand) { continue; }
		const MdRow a = md_row_of(src, cols, res_of_block(ufirst, n, u), shift, ufirst, u);
		const MdRow b = md_row_of(src, cols, res_of_block(ufirst, n, c), shift, ufirst, c);
		if (!md_same(a, b)) { flag[u] = 1u; }
	}
}

// Settle, one block, as mt_settle_kernel: the list of the REFUTED -- the rows whose flag the confirm pass set -- in ascending order, eight
// rows per thread and step, their own representatives to begin with; then answered exactly (settle_refuted), with digest equality as the
// predicate: every thread loads both rows and gets the same answer.
#define MD_SETTLE_ROWS 8u
__global__ __launch_bounds__(DV_THREADS) void md_settle_kernel(SpliceSrc src, DigestCols cols, uint32_t n, uint32_t shift, const u64* __restrict__ ufirst,
                                                              const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ flag,
                                                              uint32_t* rlist, uint32_t* rep, u64* __restrict__ nref_out)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const u64 units = ufirst[n];
	u64 nref[1] = {0};
	for (u64 base = 0; base < units; base += (u64)MD_SETTLE_ROWS * DV_THREADS) {
		const u64 u0 = base + (u64)tid * MD_SETTLE_ROWS;
		uint32_t mask = 0;
		#pragma unroll
		for (uint32_t i = 0; i < MD_SETTLE_ROWS; ++i) { if (u0 + i < units && flag[u0 + i] != 0) { mask |= 1u << i; } }
		u64 a[1] = {(u64)__popc(mask)};
		dv_block_scan<1>(a, nref, s_w);
		u64 at = a[0] - (u64)__popc(mask);
		for (uint32_t i = 0; i < MD_SETTLE_ROWS; ++i) { if (mask >> i & 1u) { rlist[at++] = (uint32_t)(u0 + i); rep[u0 + i] = (uint32_t)(u0 + i); } }
	}
	settle_refuted(rlist, nref[0], slot_of, rep, [&](uint32_t g, uint32_t c) {
		return md_same(md_row_of(src, cols, res_of_block(ufirst, n, g), shift, ufirst, g), md_row_of(src, cols, res_of_block(ufirst, n, c), shift, ufirst, c));
	});
	if (tid == 0) { nref_out[0] = nref[0]; }
}

void launch_match_digest_keys(hipStream_t st, const SpliceSrc& src, const DigestCols& cols, uint32_t n, uint32_t nbt, uint32_t shift, const MatchTab& t,
                              const int32_t* status, uint32_t blocks)
{
	hipLaunchKernelGGL(md_keys_kernel, fixed_grid(nbt, 256u, blocks), dim3(256), 0, st, src, cols, n, shift, t.kt, t.ufirst, status, t.slot_of, t.flag);
}

void launch_match_digest_confirm(hipStream_t st, const SpliceSrc& src, const DigestCols& cols, uint32_t n, uint32_t nbt, uint32_t shift, const MatchTab& t, uint32_t blocks)
{
	hipLaunchKernelGGL(md_confirm_kernel, fixed_grid(nbt, 256u, blocks), dim3(256), 0, st, src, cols, n, shift, t.ufirst, t.slot_of, t.kt.min, t.flag, t.rep);
}

void launch_match_digest_settle(hipStream_t st, const SpliceSrc& src, const DigestCols& cols, uint32_t n, uint32_t shift, const MatchTab& t)
{
	hipLaunchKernelGGL(md_settle_kernel, dim3(1), dim3(DV_THREADS), 0, st, src, cols, n, shift, t.ufirst, t.slot_of, t.flag, t.rlist, t.rep, t.nref);
}

} // namespace msc
