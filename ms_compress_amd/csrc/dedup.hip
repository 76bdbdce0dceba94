// dedup.hip -- the passes of a block deduper (mscomp_amd_deduper_*, include/mscomp_amd.h): which resources of up to four block containers
// of one format and one block size hold the same bytes, decided on the STORED form -- the stored form of a block depends only on its data,
// the format and the block size -- and answered as a pick list a splicer takes. Candidates come from the tables and 32 bytes per row (a
// 64-bit key per resource, the key table over the keys: rowpass.h kt_*); the only pass over the data is the compare that confirms a candidate.
// The sources travel by value in the kernel arguments, as one SpliceSrc that a lane indexes (kernels.h sp_view). DESIGN.md 4.13.
#include "rowpass.h"

namespace msc {

// a key table cleared: dedup's, match's
__global__ __launch_bounds__(256) void dd_clear_kernel(KeyTable kt) { kt_clear(kt); }

// Seed, one block: rules 1 and 2 per resource, the status, the key word seeded with L, the mismatch flag cleared, and ufirst (n + 1): the
// rows of the resources that passed, numbered densely in resource order (no room rule: rule 1 keeps a resource's rows within its view's
// table, and the host has held the views' tables against the creation bound).
__global__ __launch_bounds__(DV_THREADS) void dd_seed_kernel(SpliceSrc src, uint32_t n, uint32_t shift,
                                                            u64* __restrict__ ufirst, u64* __restrict__ key, uint32_t* __restrict__ flag, int32_t* __restrict__ status)
{
	seed_numbering<0>(n, 0, 0, ufirst, status, [&](uint32_t g, u64& rows, bool&) {
		u64 s, r, f0, L;
		dd_locate(src, g, s, r);
		const int32_t st = view_rows(sp_view(src, s), r, shift, f0, rows, L);
		key[g] = st == 0 ? dd_mix(L ^ 0x9E3779B97F4A7C15ull) : 0; flag[g] = 0;
		return st;
	});
}

// The row passes: a fixed grid dealt over the ROWS of the resources that passed rules 1 and 2, so that one resource of a million rows
// spreads over every CU (rcrc_fold_kernel). A row finds its resource by binary search in ufirst. KEY false: rule 3 -- a row that is not
// off[j] <= off[j + 1] <= packed_len refuses its resource; every writer stores the same value. KEY true, behind it: the rows of the
// resources that are still accepted fold a 64-bit mix of (row number, stored length, CRC word, first and last min(16, s) stored bytes)
// into their resource's key word with an atomic XOR; a wave whose 64 rows share one resource folds them in registers first.
template <bool KEY>
__global__ __launch_bounds__(256) void dd_rows_kernel(SpliceSrc src, uint32_t n, uint32_t with_crc,
                                                     const u64* __restrict__ ufirst, u64* __restrict__ key, int32_t* status)
{
	const uint32_t lane = threadIdx.x & 63u, none = ~0u;                      // (none: a lane without a row to fold)
	const u64 units = ufirst[n], step = (u64)gridDim.x * 256u;
	for (u64 base = (u64)blockIdx.x * 256u + (threadIdx.x & ~63u); base < units; base += step) {
		const u64 u = base + lane;
		uint32_t g = none;
		u64 h = 0;
		if (u < units) {
			const uint32_t x = res_of_block(ufirst, n, u);
			u64 s, r;
			dd_locate(src, x, s, r);
			const SpliceView v = sp_view(src, s);
			const u64 k = u - ufirst[x], j = v.first[r] + k;                  // (j < first[r + 1] <= v.nbt: rule 1)
			const u64 o0 = v.off[j], o1 = v.off[j + 1u];
			if (!KEY) {
				if (!(o0 <= o1 && o1 <= v.packed_len)) { status[x] = -3; }     // rule 3: MSCOMP_DATA_ERROR
			} else if (status[x] == 0) {
				h = row_key(dd_mix(k + 1u), o1 - o0, with_crc, with_crc ? v.crc[j] : 0u, v.packed + o0);
				g = x;
			}
		}
		if (KEY) {
			const uint32_t g0 = uniform(g);
			if (__ballot(g != g0) == 0) {
				h = wave_all(h, [](u64 a, u64 b) { return a ^ b; });
				if (lane == 0 && g0 != none) { atomicXor(reinterpret_cast<unsigned long long*>(&key[g0]), (unsigned long long)h); }
			} else if (g != none) { atomicXor(reinterpret_cast<unsigned long long*>(&key[g]), (unsigned long long)h); }
		}
	}
}

// One thread per accepted resource: it claims its key's slot of the key table and puts its index into the slot's minimum. (No slot: a
// damaged table; the resource is then its own candidate.)
__global__ __launch_bounds__(256) void dd_insert_kernel(uint32_t n, KeyTable kt, const u64* __restrict__ key, const int32_t* __restrict__ status, uint32_t* __restrict__ slot_of)
{
	for (u64 g = (u64)blockIdx.x * 256u + threadIdx.x; g < n; g += (u64)gridDim.x * 256u) {
		if (status[g] != 0) { continue; }
		const uint32_t slot = kt_claim(kt, key[g], dd_mix(kt_key(key[g])) % kt.slots);
		if (slot != KT_NONE) { atomicMin(&kt.min[slot], (uint32_t)g); }
		slot_of[g] = slot;
	}
}

// behind it, one thread per resource: the candidate -- the smallest accepted resource with the same key, itself for a refused one or one
// without a slot -- and the first thing that can tell two resources of one key apart: their lengths
__global__ __launch_bounds__(256) void dd_cand_kernel(SpliceSrc src, uint32_t n, const int32_t* __restrict__ status,
                                                     const uint32_t* __restrict__ tmin, const uint32_t* __restrict__ slot_of, uint32_t* __restrict__ cand,
                                                     uint32_t* __restrict__ flag)
{
	for (u64 g = (u64)blockIdx.x * 256u + threadIdx.x; g < n; g += (u64)gridDim.x * 256u) {
		uint32_t c = (uint32_t)g;
		if (status[g] == 0 && slot_of[g] != KT_NONE) {
			c = tmin[slot_of[g]];
			if (c != (uint32_t)g) {
				u64 s, r, sc, rc;
				dd_locate(src, g, s, r); dd_locate(src, c, sc, rc);
				if (sp_view(src, s).res_len[r] != sp_view(src, sc).res_len[rc]) { flag[g] = 1u; }
			}
		}
		cand[g] = c;
	}
}

// Confirm: the slices of the same row numbering (confirm_slices); what a workgroup has to look up it looks up once per row (its resource
// once per resource). A row of an accepted resource that is not its key's minimum is compared with the same row of the minimum: the
// stored lengths, the CRC words, then the pieces of the slice as one stretch of bytes. A mismatch sets the resource's flag: every writer
// stores the same value, so no ordering is needed. A workgroup looks at the flag before it starts a row and skips it when set -- what
// that saves is time alone: the flag ends as 1 exactly when something differs. (A flag set by dd_cand_kernel says that the lengths
// differ: then the two resources' rows do not pair up, and no row of the resource is looked at.)
__global__ __launch_bounds__(CPD_THREADS) void dd_confirm_kernel(SpliceSrc src, uint32_t n, uint32_t ppu_shift, uint32_t with_crc,
                                                                const u64* __restrict__ ufirst, const uint32_t* __restrict__ cand, uint32_t* flag)
{
	const uint32_t tid = threadIdx.x;
	const u64 units = ufirst[n] < ((u64)1 << 56) ? ufirst[n] : (u64)1 << 56;
	uint32_t g = 0;
	u64 g_end = 0;                                                         // the rows below g_end that are not below ufirst[g] are g's
	confirm_slices(units, ppu_shift, [&](u64 u, u64 at, u64 upto) {
		if (u >= g_end) { g = res_of_block(ufirst, n, u); g_end = ufirst[g + 1u]; }
		const uint32_t c = cand[g];
		if (c == g || flag[g] != 0) { return; }
		u64 s, r, sc, rc;
		dd_locate(src, g, s, r); dd_locate(src, c, sc, rc);
		const SpliceView v = sp_view(src, s), w = sp_view(src, sc);
		const u64 k = u - ufirst[g], j = v.first[r] + k, jc = w.first[rc] + k;  // (equal lengths, both accepted: equal row counts)
		const u64 o0 = v.off[j], len = v.off[j + 1u] - o0, c0 = w.off[jc], clen = w.off[jc + 1u] - c0;
		if (len != clen || (with_crc && v.crc[j] != w.crc[jc])) {
			if (tid == 0) { flag[g] = 1u; }
			return;
		}
		if (at >= len) { return; }
		if (cpd_differs<CPD_THREADS>(v.packed + o0 + at, w.packed + c0 + at, (upto < len ? upto : len) - at, tid)) { flag[g] = 1u; }
	});
}

// whether accepted resources g and c are equal, by the whole block (every thread calls it and gets the same answer): the lengths, then
// row by row the stored lengths and the CRC words, then the stored bytes
__device__ bool dd_equal(const SpliceSrc& src, uint32_t with_crc, uint32_t g, uint32_t c)
{
	const uint32_t tid = threadIdx.x;
	u64 s, r, sc, rc;
	dd_locate(src, g, s, r); dd_locate(src, c, sc, rc);
	const SpliceView v = sp_view(src, s), w = sp_view(src, sc);
	if (v.res_len[r] != w.res_len[rc]) { return false; }
	const u64 f = v.first[r], rows = v.first[r + 1u] - f, fc = w.first[rc];
	bool d = false;
	for (u64 k = tid; k < rows; k += DV_THREADS) {
		if (v.off[f + k + 1u] - v.off[f + k] != w.off[fc + k + 1u] - w.off[fc + k] || (with_crc && v.crc[f + k] != w.crc[fc + k])) { d = true; }
	}
	if (__syncthreads_or(d)) { return false; }
	for (u64 k = 0; k < rows; ++k) {
		const u64 o0 = v.off[f + k], len = v.off[f + k + 1u] - o0;
		if (__syncthreads_or(cpd_differs<DV_THREADS>(v.packed + o0, w.packed + w.off[fc + k], len, tid))) { return false; }
	}
	return true;
}

// Settle and emit, one block. The representatives the flags decide (a refused resource: itself; its key's minimum: itself; a confirmed
// one: the minimum) and the list of the REFUTED -- accepted, not the minimum, not equal to it -- in ascending order; count[3] is its
// length. The refuted are then answered exactly (settle_refuted). Then the scan over rep[g] == g: new_index, pick with its padding up to
// 2 n_max, count.
__global__ __launch_bounds__(DV_THREADS) void dd_settle_kernel(SpliceSrc src, uint32_t n, uint32_t n_max, uint32_t with_crc,
                                                              const uint32_t* __restrict__ cand, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ slot_of,
                                                              uint32_t* rlist, u64* rep, u64* new_index, u64* __restrict__ pick,
                                                              u64* __restrict__ count)
{
	__shared__ u64 s_w[2][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	u64 nref[1] = {0};
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t g = base + tid;
		const bool live = g < n;
		bool refuted = false;
		if (live) {
			const uint32_t c = cand[g];                                        // (g itself for a refused resource)
			refuted = c != g && flag[g] != 0;
			rep[g] = refuted ? g : c;
		}
		u64 a[1] = {refuted ? 1u : 0u};
		dv_block_scan<1>(a, nref, s_w);
		if (refuted) { rlist[a[0] - 1u] = g; }
	}
	settle_refuted(rlist, nref[0], slot_of, rep, [&](uint32_t g, uint32_t c) { return dd_equal(src, with_crc, g, c); });
	u64 tot[2] = {0, 0};                                                   // unique resources | stored bytes of the others
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t g = base + tid;
		const bool live = g < n, uniq = live && rep[g] == g;
		u64 s = 0, r = 0, saved = 0;
		if (live) {
			dd_locate(src, g, s, r);
			if (!uniq) { const SpliceView v = sp_view(src, s); saved = v.off[v.first[r + 1u]] - v.off[v.first[r]]; }   // (accepted: its offsets only grow)
		}
		u64 a[2] = {uniq ? 1u : 0u, saved};
		dv_block_scan<2>(a, tot, s_w);
		if (uniq) { const u64 q = a[0] - 1u; new_index[g] = q; pick[2u * q] = s; pick[2u * q + 1u] = r; }
	}
	__syncthreads();                                                     // the unique resources' new_index is read back below
	for (uint32_t g = tid; g < n; g += DV_THREADS) { if (rep[g] != g) { new_index[g] = new_index[rep[g]]; } }
	if (pick) { for (u64 e = 2u * tot[0] + tid; e < 2u * (u64)n_max; e += DV_THREADS) { pick[e] = ~(u64)0; } }
	if (tid == 0) { count[0] = tot[0]; count[1] = n; count[2] = tot[1]; count[3] = nref[0]; }
}

void launch_dedup_clear(hipStream_t st, const KeyTable& kt, uint32_t blocks)
{
	hipLaunchKernelGGL(dd_clear_kernel, fixed_grid(kt.slots, 256u, blocks), dim3(256), 0, st, kt);
}

void launch_dedup_rule3(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t rows_max, const u64* ufirst, int32_t* status, uint32_t blocks)
{
	hipLaunchKernelGGL(dd_rows_kernel<false>, fixed_grid(rows_max, 256u, blocks), dim3(256), 0, st, src, n, 0u, ufirst, static_cast<u64*>(nullptr), status);
}

void launch_dedup_judge(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t n_max, uint32_t rows_max, uint32_t shift, const DedupTab& t, int32_t* status, uint32_t blocks)
{
	if (n_max == 0) { return; }
	launch_dedup_clear(st, t.kt, blocks);
	hipLaunchKernelGGL(dd_seed_kernel, dim3(1), dim3(DV_THREADS), 0, st, src, n, shift, t.ufirst, t.key, t.flag, status);
	if (rows_max == 0) { return; }
	launch_dedup_rule3(st, src, n, rows_max, t.ufirst, status, blocks);
}

void launch_dedup_keys(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t n_max, uint32_t rows_max, bool with_crc, const DedupTab& t, int32_t* status, uint32_t blocks)
{
	if (n_max == 0) { return; }
	if (rows_max) {
		hipLaunchKernelGGL(dd_rows_kernel<true>, fixed_grid(rows_max, 256u, blocks), dim3(256), 0, st, src, n, with_crc ? 1u : 0u, t.ufirst, t.key, status);
	}
	hipLaunchKernelGGL(dd_insert_kernel, fixed_grid(n_max, 256u, blocks), dim3(256), 0, st, n, t.kt, t.key, status, t.slot_of);
	hipLaunchKernelGGL(dd_cand_kernel, fixed_grid(n_max, 256u, blocks), dim3(256), 0, st, src, n, status, t.kt.min, t.slot_of, t.cand, t.flag);
}

void launch_dedup_confirm(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t n_max, uint32_t rows_max, uint32_t shift, bool with_crc, const DedupTab& t, uint32_t blocks)
{
	if (n_max == 0 || rows_max == 0) { return; }
	const uint32_t ppu_shift = shift > DD_PIECE_SHIFT ? shift - DD_PIECE_SHIFT : 0u;
	hipLaunchKernelGGL(dd_confirm_kernel, fixed_grid((u64)rows_max << ppu_shift, DD_SLICE_MIN, blocks), dim3(CPD_THREADS), 0, st, src, n, ppu_shift,
	                   with_crc ? 1u : 0u, t.ufirst, t.cand, t.flag);
}

void launch_dedup_settle(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t n_max, bool with_crc, const DedupTab& t, u64* rep, u64* new_index, u64* pick, u64* count)
{
	hipLaunchKernelGGL(dd_settle_kernel, dim3(1), dim3(DV_THREADS), 0, st, src, n, n_max, with_crc ? 1u : 0u, t.cand, t.flag, t.slot_of, t.rlist,
	                   rep, new_index, pick, count);
}

} // namespace msc
