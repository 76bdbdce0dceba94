// match.hip -- the passes of a block deduper made for match (mscomp_amd_deduper_create_match / _match, include/mscomp_amd.h): for every block
// of the resources of a block container (next), whether an equal block lies in one of up to three store containers, earlier in next, or
// nowhere, decided on the STORED form -- the stored form of a block depends only on its data, the format and the block size -- and answered
// as two extent lists a splicer made for extents takes: the blocks seen for the first time (the delta), and stores + delta put together
// again (the patch). The unit is the ROW: the key table (rowpass.h kt_*), dedup's candidates and confirm pass over the rows of all views instead of their
// resources, diff's tiled run passes over the rows of next. The views travel by value in the kernel arguments, as one SpliceSrc that a lane indexes
// (kernels.h sp_view), the stores first and next behind them. DESIGN.md 4.18.
#include "rowpass.h"

namespace msc {

#define MT_FOUND  0u                                       // class of a row of next: its representative is a row of a store ...
#define MT_SHARED 1u                                       // ... an earlier row of next ...
#define MT_FRESH  2u                                       // ... itself

// Row u of the numbering, of a resource that passed rules 1 and 2: where it lies and what the tables say about it
struct MtRow {
	const uint8_t* p;                                      // its stored bytes (read only for a resource that passed rule 3)
	u64 len, e;                                            // stored length, data length
	uint32_t crc, x;                                       // CRC word (0 without checksums), global resource
};
__device__ __forceinline__ MtRow mt_row_of(const SpliceSrc& src, uint32_t x, uint32_t shift, uint32_t with_crc,
                                           const u64* __restrict__ ufirst, u64 u)
{
	u64 s, r;
	dd_locate(src, x, s, r);
	const SpliceView v = sp_view(src, s);
	const u64 k = u - ufirst[x], j = v.first[r] + k;                       // (j < first[r + 1] <= v.nbt: rule 1)
	const u64 o0 = v.off[j], L = v.res_len[r] - (k << shift), B = (u64)1 << shift;   // (k is a block of the resource: rule 2)
	return MtRow{ v.packed + o0, v.off[j + 1u] - o0, L < B ? L : B, with_crc ? v.crc[j] : 0u, x };
}
__device__ __forceinline__ MtRow mt_row(const SpliceSrc& src, uint32_t n, uint32_t shift, uint32_t with_crc,
                                        const u64* __restrict__ ufirst, u64 u)
{
	return mt_row_of(src, res_of_block(ufirst, n, u), shift, with_crc, ufirst, u);
}

// Seed, one block: dedup's rules 1 and 2 per resource, the room of rule 4 -- over all rows against nbt, over next's (the resources from
// n_store on) against nbn as well --, the status, and ufirst (n + 1): the rows of the resources that passed, numbered densely in
// resource order.
__global__ __launch_bounds__(DV_THREADS) void mt_seed_kernel(SpliceSrc src, uint32_t n, uint32_t n_store, uint32_t nbt, uint32_t nbn,
                                                            uint32_t shift, u64* __restrict__ ufirst, int32_t* __restrict__ status)
{
	seed_numbering<2>(n, nbt, nbn, ufirst, status, [&](uint32_t g, u64& rows, bool& of_next) {
		u64 s, r, f0, L;
		dd_locate(src, g, s, r);
		of_next = g >= n_store;
		return view_rows(sp_view(src, s), r, shift, f0, rows, L);
	});
}

// Keys, a fixed grid dealt over the rows: a row of an accepted resource mixes its key tuple -- data length, then row_key's: stored length,
// CRC word when checksums take part, first and last min(16, s) stored bytes -- into 64 bits, claims the key's slot of the key table and
// puts its number into the slot's minimum. A row of a refused resource has no slot, and neither has one whose walk found none (a damaged
// table): it is its own representative.
__global__ __launch_bounds__(256) void mt_keys_kernel(SpliceSrc src, uint32_t n, uint32_t shift, uint32_t with_crc, KeyTable kt,
                                                     const u64* __restrict__ ufirst, const int32_t* __restrict__ status,
                                                     uint32_t* __restrict__ slot_of, uint32_t* __restrict__ flag)
{
	const u64 units = ufirst[n];
	for (u64 u = (u64)blockIdx.x * 256u + threadIdx.x; u < units; u += (u64)gridDim.x * 256u) {
		const uint32_t x = res_of_block(ufirst, n, u);
		uint32_t slot = KT_NONE;
		if (status[x] == 0) {
			const MtRow a = mt_row_of(src, x, shift, with_crc, ufirst, u);
			const u64 h = row_key(dd_mix(a.e ^ 0x9E3779B97F4A7C15ull), a.len, with_crc, a.crc, a.p);
			slot = kt_claim(kt, h, dd_mix(kt_key(h)) % kt.slots);
			if (slot != KT_NONE) { atomicMin(&kt.min[slot], (uint32_t)u); }
		}
		slot_of[u] = slot; flag[u] = 0;
	}
}

// Confirm, the only pass over data: the slices of the numbering (confirm_slices). A row that is not its slot's smallest is compared with
// that row: the data lengths, the stored lengths, the CRC words, then the pieces of the slice as one stretch of bytes. A mismatch sets
// the row's flag: every writer stores the same value, so no ordering is needed; a workgroup that finds the flag set skips the row, which
// saves time alone. The workgroup that holds a row's first piece leaves the representative the tables give in rep -- the candidate, or
// the row itself where it has none --, for the settle to correct where a flag is set. Rows that follow one another mostly have
// candidates that do, so both resources are looked up once per resource, not once per row.
__global__ __launch_bounds__(CPD_THREADS) void mt_confirm_kernel(SpliceSrc src, uint32_t n, uint32_t shift, uint32_t ppu_shift,
                                                                uint32_t with_crc, const u64* __restrict__ ufirst, const uint32_t* __restrict__ slot_of,
                                                                const uint32_t* __restrict__ tmin, uint32_t* flag, uint32_t* __restrict__ rep)
{
	const uint32_t tid = threadIdx.x;
	uint32_t x = 0, cx = 0;
	u64 x_end = 0, c_lo = 0, c_end = 0;                                    // the rows below x_end that are not below ufirst[x] are x's; [c_lo, c_end) are cx's
	confirm_slices(ufirst[n], ppu_shift, [&](u64 u, u64 at, u64 upto) {      // (units <= n_blocks_total < 2^31)
		const uint32_t slot = slot_of[u];
		const uint32_t c = slot == KT_NONE ? (uint32_t)u : tmin[slot];     // (no slot: a refused resource, no byte of it is read)
		const bool cand = c < u;                                           // (c > u: a damaged table; the row stands for itself)
		if (at == 0 && tid == 0) { rep[u] = cand ? c : (uint32_t)u; }
		if (!cand || flag[u] != 0) { return; }
		if (u >= x_end) { x = res_of_block(ufirst, n, u); x_end = ufirst[x + 1u]; }
		if (c < c_lo || c >= c_end) { cx = res_of_block(ufirst, n, c); c_lo = ufirst[cx]; c_end = ufirst[cx + 1u]; }
		const MtRow a = mt_row_of(src, x, shift, with_crc, ufirst, u), b = mt_row_of(src, cx, shift, with_crc, ufirst, c);
		if (a.e != b.e || a.len != b.len || a.crc != b.crc) {
			if (tid == 0) { flag[u] = 1u; }
			return;
		}
		if (at >= a.len) { return; }
		if (cpd_differs<CPD_THREADS>(a.p + at, b.p + at, (upto < a.len ? upto : a.len) - at, tid)) { flag[u] = 1u; }
	});
}

// whether rows g and c of accepted resources are equal, by the whole block (every thread calls it and gets the same answer)
__device__ bool mt_equal(const SpliceSrc& src, uint32_t n, uint32_t shift, uint32_t with_crc,
                         const u64* __restrict__ ufirst, uint32_t g, uint32_t c)
{
	const MtRow a = mt_row(src, n, shift, with_crc, ufirst, g), b = mt_row(src, n, shift, with_crc, ufirst, c);
	if (a.e != b.e || a.len != b.len || a.crc != b.crc) { return false; }
	return !__syncthreads_or(cpd_differs<DV_THREADS>(a.p, b.p, a.len, threadIdx.x));
}

// Settle, one block. The list of the REFUTED -- the rows whose flag the confirm pass set: not the smallest of their slot, not equal to it
// -- in ascending order, eight rows per thread and step; every other row keeps the representative the confirm pass left. The refuted,
// their own representatives to begin with, are then answered exactly (settle_refuted).
#define MT_SETTLE_ROWS 8u
__global__ __launch_bounds__(DV_THREADS) void mt_settle_kernel(SpliceSrc src, uint32_t n, uint32_t shift, uint32_t with_crc,
                                                              const u64* __restrict__ ufirst, const uint32_t* __restrict__ slot_of, const uint32_t* __restrict__ flag,
                                                              uint32_t* rlist, uint32_t* rep, u64* __restrict__ nref_out)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const u64 units = ufirst[n];
	u64 nref[1] = {0};
	for (u64 base = 0; base < units; base += (u64)MT_SETTLE_ROWS * DV_THREADS) {
		const u64 u0 = base + (u64)tid * MT_SETTLE_ROWS;
		uint32_t mask = 0;
		#pragma unroll
		for (uint32_t i = 0; i < MT_SETTLE_ROWS; ++i) { if (u0 + i < units && flag[u0 + i] != 0) { mask |= 1u << i; } }
		u64 a[1] = {(u64)__popc(mask)};
		dv_block_scan<1>(a, nref, s_w);
		u64 at = a[0] - (u64)__popc(mask);
		for (uint32_t i = 0; i < MT_SETTLE_ROWS; ++i) { if (mask >> i & 1u) { rlist[at++] = (uint32_t)(u0 + i); rep[u0 + i] = (uint32_t)(u0 + i); } }
	}
	settle_refuted(rlist, nref[0], slot_of, rep, [&](uint32_t g, uint32_t c) { return mt_equal(src, n, shift, with_crc, ufirst, g, c); });
	if (tid == 0) { nref_out[0] = nref[0]; }
}

// What row u0 + t of the numbering -- row t of next's -- is to the run passes. A row of a resource that a row check refused is no row at all.
struct MtRun {
	uint32_t g, cls;
	u64 k;
	bool valid, live, starts, ends;                                       // valid: a row of the numbering; starts / ends a run (rule 7)
};
__device__ __forceinline__ uint32_t mt_class(u64 u0, u64 u, uint32_t r) { return r < u0 ? MT_FOUND : r == u ? MT_FRESH : MT_SHARED; }
// whether rows u and u + 1 of one resource of next lie in one run: one class, and the representatives consecutive rows of one resource
__device__ __forceinline__ bool mt_joined(uint32_t n, const u64* __restrict__ ufirst, const uint32_t* __restrict__ rep, u64 u0, u64 u)
{
	const uint32_t ra = rep[u], rb = rep[u + 1u], ca = mt_class(u0, u, ra);
	if (ca != mt_class(u0, u + 1u, rb)) { return false; }
	if (ca == MT_FRESH) { return true; }
	return rb == ra + 1u && ufirst[res_of_block(ufirst, n, rb)] != rb;     // (rb is not the first row of its resource: ra is of the same)
}
__device__ __forceinline__ MtRun mt_run(uint32_t n, const u64* __restrict__ ufirst, const int32_t* __restrict__ status, const uint32_t* __restrict__ rep, u64 u0, u64 t)
{
	MtRun r = {0, 0, 0, false, false, false, false};
	const u64 u = u0 + t;
	if (u >= ufirst[n]) { return r; }
	r.valid = true;
	r.g = res_of_block(ufirst, n, u);
	r.k = u - ufirst[r.g];
	if (status[r.g] != 0) { return r; }
	r.live = true;
	r.cls = mt_class(u0, u, rep[u]);
	r.starts = r.k == 0 || !mt_joined(n, ufirst, rep, u0, u - 1u);
	r.ends = u + 1u == ufirst[r.g + 1u] || !mt_joined(n, ufirst, rep, u0, u);
	return r;
}

// Runs (RunScan). Tile b of ROW_TILE rows of next, eight words: the sums of run starts, fresh-run starts, found, shared and fresh blocks,
// fresh stored bytes and rows of accepted resources; then a maximum -- the last row of the tile that starts a run, + 1 (0: the tile has
// none). Every row leaves the fresh rows of its tile in front of it in flocal: with the tiles' running sums that is its rank among all
// fresh rows, which a shared run in ANOTHER tile asks its representative for.
__global__ __launch_bounds__(DV_THREADS) void mt_tile_kernel(SpliceSrc src, uint32_t n, uint32_t n_store, uint32_t nbn, uint32_t shift,
                                                            const u64* __restrict__ ufirst, const int32_t* __restrict__ status, const uint32_t* __restrict__ rep,
                                                            u64* __restrict__ tsum, uint32_t* __restrict__ flocal)
{
	__shared__ u64 s_w[7][DV_WAVES];
	const u64 u0 = ufirst[n_store], t = (u64)blockIdx.x * ROW_TILE + threadIdx.x;
	const MtRun r = mt_run(n, ufirst, status, rep, u0, t);
	const bool fresh = r.live && r.cls == MT_FRESH;
	const u64 bytes = fresh ? mt_row_of(src, r.g, shift, 0u, ufirst, u0 + t).len : 0;
	u64 a[7] = {r.starts ? 1u : 0u, r.starts && fresh ? 1u : 0u, r.live && r.cls == MT_FOUND ? 1u : 0u, r.live && r.cls == MT_SHARED ? 1u : 0u, fresh ? 1u : 0u, bytes,
	            r.live ? 1u : 0u}, sum[7] = {0, 0, 0, 0, 0, 0, 0};
	dv_block_scan<7>(a, sum, s_w);
	if (t < nbn) { flocal[t] = (uint32_t)(a[4] - (fresh ? 1u : 0u)); }
	u64 m[1] = {r.starts ? t + 1u : 0};
	RunScan<7>::tile<7>(tsum, sum, m, s_w[0]);
}

// the fresh rows of next in front of its row t (t < nbn, a row of the numbering)
__device__ __forceinline__ u64 mt_rank(const u64* __restrict__ tsum, const uint32_t* __restrict__ flocal, u64 t)
{
	const u64 b = t / ROW_TILE;
	return (b ? tsum[8u * (b - 1u) + 4u] : 0) + flocal[t];
}

// The rows again, with the sums in front of the tile. The row that ENDS a run writes its extents, whole: the run's first row is the running
// maximum of the rows that start a run. A found run names the store rows of its representatives; a fresh run its own place among the fresh
// blocks of its resource, which is where the delta puts them; a shared run the place of its representatives among the fresh blocks of
// THEIR resource. The first row of a resource leaves the five counts in front of it in pfirst, for the pass behind.
__global__ __launch_bounds__(DV_THREADS) void mt_runs_kernel(SpliceView v0, SpliceView v1, SpliceView v2, uint32_t n_src, uint32_t n, uint32_t n_store,
                                                            const u64* __restrict__ ufirst, const int32_t* __restrict__ status, const uint32_t* __restrict__ rep,
                                                            const u64* __restrict__ tsum, const uint32_t* __restrict__ flocal, u64* __restrict__ pfirst,
                                                            u64* __restrict__ delta_ext, u64* __restrict__ patch_ext)
{
	__shared__ u64 s_w[5][DV_WAVES];
	const u64 u0 = ufirst[n_store], t = (u64)blockIdx.x * ROW_TILE + threadIdx.x;
	const MtRun r = mt_run(n, ufirst, status, rep, u0, t);
	const bool fresh = r.live && r.cls == MT_FRESH;
	const u64 own[5] = {r.starts ? 1u : 0u, r.starts && fresh ? 1u : 0u, r.live && r.cls == MT_FOUND ? 1u : 0u, r.live && r.cls == MT_SHARED ? 1u : 0u, fresh ? 1u : 0u};
	u64 a[5];
	const u64 m0 = RunScan<5>::head<7>(tsum, t, own, a, s_w);
	if (r.valid && r.k == 0) { RunScan<5>::front(pfirst + 5u * (u64)(r.g - n_store), a, own); }
	if (!r.ends) { return; }
	const u64 t0 = m0 - 1u, cnt = t - t0 + 1u, q = r.g - n_store;             // the run [t0, t]: a run lies in one resource
	u64* pe = patch_ext + 4u * (a[0] - 1u);                                // (fewer runs than rows: inside 4 n_blocks_new)
	if (fresh) {
		pe[0] = n_src; pe[1] = q; pe[2] = mt_rank(tsum, flocal, t0) - mt_rank(tsum, flocal, ufirst[r.g] - u0); pe[3] = cnt;
		u64* de = delta_ext + 4u * (a[1] - 1u);
		de[0] = 0; de[1] = q; de[2] = u0 + t0 - ufirst[r.g]; de[3] = cnt;
		return;
	}
	const u64 first_rep = rep[u0 + t0];
	const uint32_t xr = res_of_block(ufirst, n, first_rep);
	if (r.cls == MT_FOUND) {
		u64 s, rr;
		dd_locate(v0, v1, v2, xr, s, rr);
		pe[0] = s; pe[1] = rr; pe[2] = first_rep - ufirst[xr]; pe[3] = cnt;
	} else {
		pe[0] = n_src; pe[1] = xr - n_store; pe[2] = mt_rank(tsum, flocal, first_rep - u0) - mt_rank(tsum, flocal, ufirst[xr] - u0); pe[3] = cnt;
	}
}

// Counts, one thread per resource of next and one more (counts_in_front, over next's part of the numbering): what lies in front of
// resource q and of resource q + 1.
__global__ __launch_bounds__(256) void mt_counts_kernel(uint32_t n, uint32_t n_store, uint32_t tiles, const u64* __restrict__ ufirst, const u64* __restrict__ tsum,
                                                       const u64* __restrict__ pfirst, const u64* __restrict__ nref, u64* __restrict__ delta_first,
                                                       u64* __restrict__ patch_first, u64* __restrict__ cls, u64* __restrict__ count)
{
	const u64 units = tiles ? ufirst[n] : 0;                                // (no tile: no row of next, and nothing left in pfirst)
	const uint32_t n_next = n - n_store;
	const u64* nfirst = ufirst + n_store;                                   // first row of every resource of next (n_next + 1)
	const u64* total = tsum + 8u * (u64)(tiles ? tiles - 1u : 0u);
	u64 tot[7] = {0, 0, 0, 0, 0, 0, 0};
	if (tiles) { for (uint32_t i = 0; i < 7u; ++i) { tot[i] = total[i]; } }
	for (u64 q = (u64)blockIdx.x * 256u + threadIdx.x; q <= n_next; q += (u64)gridDim.x * 256u) {
		u64 at[5], behind[5];
		counts_in_front(nfirst, n_next, units, pfirst, tot, nfirst[q], at);
		counts_in_front(nfirst, n_next, units, pfirst, tot, nfirst[q < n_next ? q + 1u : n_next], behind);
		if (patch_first) { patch_first[q] = at[0]; }
		if (delta_first) { delta_first[q] = at[1]; }
		if (q < n_next) { cls[3u * q] = behind[2] - at[2]; cls[3u * q + 1u] = behind[3] - at[3]; cls[3u * q + 2u] = behind[4] - at[4]; }
		else { count[0] = tot[2]; count[1] = tot[3]; count[2] = tot[4]; count[3] = tot[6]; count[4] = tot[5]; count[5] = nref ? nref[0] : 0; }
	}
}

void launch_match_seed(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t n_store, uint32_t nbt, uint32_t nbn, uint32_t shift, const MatchTab& t, int32_t* status)
{
	hipLaunchKernelGGL(mt_seed_kernel, dim3(1), dim3(DV_THREADS), 0, st, src, n, n_store, nbt, nbn, shift, t.ufirst, status);
}

void launch_match_keys(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t nbt, uint32_t shift, bool with_crc, const MatchTab& t, const int32_t* status, uint32_t blocks)
{
	hipLaunchKernelGGL(mt_keys_kernel, fixed_grid(nbt, 256u, blocks), dim3(256), 0, st, src, n, shift, with_crc ? 1u : 0u, t.kt, t.ufirst, status,
	                   t.slot_of, t.flag);
}

void launch_match_confirm(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t nbt, uint32_t shift, bool with_crc, const MatchTab& t, uint32_t blocks)
{
	const uint32_t ppu_shift = shift > DD_PIECE_SHIFT ? shift - DD_PIECE_SHIFT : 0u;
	hipLaunchKernelGGL(mt_confirm_kernel, fixed_grid((u64)nbt << ppu_shift, DD_SLICE_MIN, blocks), dim3(CPD_THREADS), 0, st, src, n, shift, ppu_shift,
	                   with_crc ? 1u : 0u, t.ufirst, t.slot_of, t.kt.min, t.flag, t.rep);
}

void launch_match_settle(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t shift, bool with_crc, const MatchTab& t)
{
	hipLaunchKernelGGL(mt_settle_kernel, dim3(1), dim3(DV_THREADS), 0, st, src, n, shift, with_crc ? 1u : 0u, t.ufirst, t.slot_of, t.flag, t.rlist,
	                   t.rep, t.nref);
}

void launch_match_runs(hipStream_t st, const SpliceSrc& src, uint32_t n_src, uint32_t n, uint32_t n_store, uint32_t nbn, uint32_t shift, const MatchTab& t, const int32_t* status,
                       u64* delta_ext, u64* patch_ext)
{
	const uint32_t tiles = row_tiles(nbn);
	hipLaunchKernelGGL(mt_tile_kernel, dim3(tiles), dim3(DV_THREADS), 0, st, src, n, n_store, nbn, shift, t.ufirst, status, t.rep, t.tsum, t.flocal);
	hipLaunchKernelGGL((rows_tilescan_kernel<7, -1>), dim3(1), dim3(DV_THREADS), 0, st, tiles, t.tsum);
	hipLaunchKernelGGL(mt_runs_kernel, dim3(tiles), dim3(DV_THREADS), 0, st, src.v[0], src.v[1], src.v[2], n_src, n, n_store, t.ufirst, status, t.rep, t.tsum, t.flocal, t.pfirst,
	                   delta_ext, patch_ext);
}

void launch_match_counts(hipStream_t st, uint32_t n, uint32_t n_store, uint32_t nbn, bool settled, const MatchTab& t, u64* delta_first, u64* patch_first, u64* cls, u64* count,
                         uint32_t blocks)
{
	hipLaunchKernelGGL(mt_counts_kernel, fixed_grid((u64)(n - n_store) + 1u, 256u, blocks), dim3(256), 0, st, n, n_store, row_tiles(nbn), t.ufirst, t.tsum, t.pfirst,
	                   settled ? t.nref : static_cast<const u64*>(nullptr), delta_first, patch_first, cls, count);
}

} // namespace msc
