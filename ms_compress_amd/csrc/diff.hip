// diff.hip -- the passes of a block deduper made for diff (mscomp_amd_deduper_create_diff / _diff, include/mscomp_amd.h): which blocks of the
// resources of a block container differ from the blocks at the same index of the resources of its previous version, decided on the STORED
// form -- the stored form of a block depends only on its data, the format and the block size -- and answered as two extent lists a splicer
// made for extents takes: the changed blocks alone (the delta), and base + delta put together again (the patch). Everything but one pass
// reads the tables alone; the only pass over the data is the compare that confirms an unchanged block. The two views travel by value in
// the kernel arguments, as a splicer's. DESIGN.md 4.16.
#include "rowpass.h"

namespace msc {

#define DF_CHANGED 1u                                      // verdict bits of a row: it is a changed block ...
#define DF_REFUTED 2u                                      // ... and its tables said otherwise: the stored bytes did (always with DF_CHANGED)
#define DF_NO_BASE (~(u64)0)

// Seed, one block: per pair rule 1, the table checks of rule 2 (the new resource before the base resource within each), the room of
// rule 3 and the status, and ufirst (n_pair + 1): the new rows of the pairs that passed, numbered densely in pair order. src: base, next.
// The two sides are one loop over a lane's index into src: written out side by side the kernel spills eight scalar registers, whichever
// way the views reach it. The loop costs the seed 0.5 us of 8.4 on an MI355X: the base side's loads follow the new side's.
__global__ __launch_bounds__(DV_THREADS) void df_seed_kernel(SpliceSrc src, uint32_t n_pair, uint32_t nbn, uint32_t shift, const u64* __restrict__ pair,
                                                            u64* __restrict__ ufirst, int32_t* __restrict__ status)
{
	seed_numbering<1>(n_pair, nbn, 0, ufirst, status, [&](uint32_t p, u64& rows, bool&) {
		int32_t st = 0;
		for (uint32_t side = 2; side-- && st != -2; ) {                       // the new resource, then the base resource
			const u64 r = pair[2u * (u64)p + side];
			if (side == 0 && r == DF_NO_BASE) { break; }
			const SpliceView& v = sp_view(src, side);
			u64 f0, n, L;
			const int32_t s1 = r < v.n_res ? view_rows(v, r, shift, f0, n, L) : -2;   // rule 1: no table entry of a resource the view does not have is read
			if (side) { rows = n; }
			if (s1 == -2 || st == 0) { st = s1; }                               // rule 2: rule 1 of either side before rule 2 of either
		}
		if (st) { rows = 0; }
		return st;
	});
}

// Row verdicts from the tables: a fixed grid dealt over the new rows of the numbering, a row finds its pair by binary search in ufirst.
// The row checks of rule 2 on both sides -- a row that is not off[j] <= off[j + 1] <= packed_len refuses its pair; every writer stores the
// same value --, then rule 5 without its last clause: no base, no such base block, another data length, another stored length, another
// CRC word: changed. Everything else is a candidate for the confirm pass.
__global__ __launch_bounds__(256) void df_verdict_kernel(SpliceView base, SpliceView next, uint32_t n_pair, uint32_t shift, uint32_t with_crc, const u64* __restrict__ pair,
                                                        const u64* __restrict__ ufirst, uint32_t* __restrict__ verdict, int32_t* status)
{
	const u64 units = ufirst[n_pair], B = (u64)1 << shift;
	for (u64 u = (u64)blockIdx.x * 256u + threadIdx.x; u < units; u += (u64)gridDim.x * 256u) {
		const uint32_t p = res_of_block(ufirst, n_pair, u);
		const u64 a = pair[2u * (u64)p], b = pair[2u * (u64)p + 1u], k = u - ufirst[p];
		const u64 j = next.first[b] + k;                                       // (< next.nbt: rule 2)
		const u64 o0 = next.off[j], o1 = next.off[j + 1u];
		bool bad = !(o0 <= o1 && o1 <= next.packed_len), changed = true;
		if (a != DF_NO_BASE) {
			const u64 g0 = base.first[a], na = base.first[a + 1u] - g0;
			if (k < na) {
				const u64 c0 = base.off[g0 + k], c1 = base.off[g0 + k + 1u];
				if (!(c0 <= c1 && c1 <= base.packed_len)) { bad = true; }
				else if (!bad) {
					const u64 L = next.res_len[b] - (k << shift), La = base.res_len[a] - (k << shift);   // (k is a block of both: no underflow)
					changed = (L < B ? L : B) != (La < B ? La : B) || o1 - o0 != c1 - c0 || (with_crc && next.crc[j] != base.crc[g0 + k]);
				}
			}
		}
		if (bad) { status[p] = -3; }                                           // MSCOMP_DATA_ERROR
		verdict[u] = changed ? DF_CHANGED : 0u;
	}
}

// Confirm, the only pass over data: the slices of the numbering (confirm_slices). A candidate row of an accepted pair has its stored bytes
// compared with the base row's, the pieces of the slice as one stretch; a mismatch stores changed + refuted into the row's verdict. Every
// writer stores the same value, so no ordering is needed; a workgroup that finds the row settled skips it, which saves time alone.
__global__ __launch_bounds__(CPD_THREADS) void df_confirm_kernel(SpliceView base, SpliceView next, uint32_t n_pair, uint32_t ppu_shift, const u64* __restrict__ pair,
                                                                const u64* __restrict__ ufirst, const int32_t* __restrict__ status, uint32_t* verdict)
{
	const uint32_t tid = threadIdx.x;
	uint32_t p = 0;
	u64 p_end = 0;                                                         // the rows below p_end that are not below ufirst[p] are p's
	bool live = false;
	confirm_slices(ufirst[n_pair], ppu_shift, [&](u64 u, u64 at, u64 upto) {  // (units <= n_blocks_new < 2^31)
		if (u >= p_end) { p = res_of_block(ufirst, n_pair, u); p_end = ufirst[p + 1u]; live = status[p] == 0; }
		if (!live || verdict[u] != 0) { return; }                          // a refused pair: no byte of it is read
		const u64 a = pair[2u * (u64)p], b = pair[2u * (u64)p + 1u], k = u - ufirst[p];
		const u64 j = next.first[b] + k, ja = base.first[a] + k;             // (a candidate: the base has the block)
		const u64 o0 = next.off[j], len = next.off[j + 1u] - o0, c0 = base.off[ja];   // (a candidate: equal stored lengths)
		if (at >= len) { return; }
		if (cpd_differs<CPD_THREADS>(next.packed + o0 + at, base.packed + c0 + at, (upto < len ? upto : len) - at, tid)) { verdict[u] = DF_CHANGED | DF_REFUTED; }
	});
}

// What row u of the numbering is to the run passes. A row of a pair that a row check refused is no row at all.
struct DfRow {
	uint32_t p;
	u64 k;
	bool live, changed, refuted, starts, ends;                            // starts / ends a run (rule 6)
};
__device__ __forceinline__ DfRow df_row(uint32_t n_pair, const u64* __restrict__ ufirst, const int32_t* __restrict__ status, const uint32_t* __restrict__ verdict, u64 u)
{
	DfRow r = {0, 0, false, false, false, false, false};
	if (u >= ufirst[n_pair]) { return r; }
	r.p = res_of_block(ufirst, n_pair, u);
	r.k = u - ufirst[r.p];
	if (status[r.p] != 0) { return r; }
	const uint32_t v = verdict[u];
	r.live = true; r.changed = (v & DF_CHANGED) != 0; r.refuted = (v & DF_REFUTED) != 0;
	r.starts = r.k == 0 || ((verdict[u - 1u] & DF_CHANGED) != 0) != r.changed;
	r.ends = u + 1u == ufirst[r.p + 1u] || ((verdict[u + 1u] & DF_CHANGED) != 0) != r.changed;
	return r;
}

// Runs (RunScan). Tile g of ROW_TILE rows, eight words: the sums of run starts, changed-run starts, changed blocks, changed stored bytes,
// rows of accepted pairs and refuted rows; then two maxima -- the last row of the tile that starts a run, + 1, and the tile's count of
// changed blocks in front of the last row of the tile that is the first of its pair, + 1 (0: the tile has none).
__global__ __launch_bounds__(DV_THREADS) void df_tile_kernel(SpliceView next, uint32_t n_pair, const u64* __restrict__ pair, const u64* __restrict__ ufirst,
                                                            const int32_t* __restrict__ status, const uint32_t* __restrict__ verdict, u64* __restrict__ tsum)
{
	__shared__ u64 s_w[6][DV_WAVES];
	const u64 u = (u64)blockIdx.x * ROW_TILE + threadIdx.x;
	const DfRow r = df_row(n_pair, ufirst, status, verdict, u);
	u64 bytes = 0;
	if (r.live && r.changed) { const u64 j = next.first[pair[2u * (u64)r.p + 1u]] + r.k; bytes = next.off[j + 1u] - next.off[j]; }
	u64 a[6] = {r.starts ? 1u : 0u, r.starts && r.changed ? 1u : 0u, r.live && r.changed ? 1u : 0u, bytes, r.live ? 1u : 0u, r.refuted ? 1u : 0u}, sum[6] = {0, 0, 0, 0, 0, 0};
	dv_block_scan<6>(a, sum, s_w);
	u64 m[2] = {r.starts ? u + 1u : 0, r.live && r.k == 0 ? a[2] - (r.changed ? 1u : 0u) + 1u : 0};
	RunScan<6>::tile<6>(tsum, sum, m, s_w[0]);
}

// The rows again, with the sums in front of the tile. The row that ENDS a run writes its extents, whole: the run's first row is the
// running maximum of the rows that start a run, so its length and first block need no second look at the rows between; the changed
// blocks in front of the pair -- they only grow along the numbering -- are the running maximum of that count over the pairs' first rows.
// The first row of a pair leaves the three counts in front of it in pfirst, for the pass behind.
__global__ __launch_bounds__(DV_THREADS) void df_runs_kernel(uint32_t n_pair, const u64* __restrict__ pair, const u64* __restrict__ ufirst, const int32_t* __restrict__ status,
                                                            const uint32_t* __restrict__ verdict, const u64* __restrict__ tsum, u64* __restrict__ pfirst,
                                                            u64* __restrict__ delta_ext, u64* __restrict__ patch_ext)
{
	__shared__ u64 s_w[3][DV_WAVES];
	const u64 u = (u64)blockIdx.x * ROW_TILE + threadIdx.x;
	const DfRow r = df_row(n_pair, ufirst, status, verdict, u);
	const u64 own[3] = {r.starts ? 1u : 0u, r.starts && r.changed ? 1u : 0u, r.live && r.changed ? 1u : 0u};
	u64 a[3], c1 = blockIdx.x ? tsum[8u * (u64)(blockIdx.x - 1u) + 7u] : 0;
	const u64 m0 = RunScan<3>::head<6>(tsum, u, own, a, s_w);
	u64 m1 = r.live && r.k == 0 ? a[2] - own[2] + 1u : 0;
	dv_block_max(m1, c1, s_w[0]);
	if (u < ufirst[n_pair] && r.k == 0) { RunScan<3>::front(pfirst + 3u * (u64)r.p, a, own); }
	if (!r.ends) { return; }
	const u64 u0 = m0 - 1u, cnt = u - u0 + 1u, k0 = u0 - ufirst[r.p];          // the run [u0, u]: a run lies in one pair
	u64* pe = patch_ext + 4u * (a[0] - 1u);                                // (fewer runs than rows: inside 4 n_blocks_new)
	if (r.changed) {
		pe[0] = 1u; pe[1] = r.p; pe[2] = a[2] - cnt - (m1 - 1u); pe[3] = cnt;
		u64* de = delta_ext + 4u * (a[1] - 1u);
		de[0] = 0; de[1] = pair[2u * (u64)r.p + 1u]; de[2] = k0; de[3] = cnt;
	} else {
		pe[0] = 0; pe[1] = pair[2u * (u64)r.p]; pe[2] = k0; pe[3] = cnt;
	}
}

// Counts, one thread per pair and one more (counts_in_front): what lies in front of pair p and of pair p + 1.
__global__ __launch_bounds__(256) void df_counts_kernel(uint32_t n_pair, uint32_t tiles, const u64* __restrict__ ufirst, const u64* __restrict__ tsum, const u64* __restrict__ pfirst,
                                                       u64* __restrict__ delta_first, u64* __restrict__ patch_first, u64* __restrict__ changed, u64* __restrict__ count)
{
	const u64 units = ufirst[n_pair];
	const u64* total = tsum + 8u * (u64)(tiles ? tiles - 1u : 0u);
	u64 tot[6] = {0, 0, 0, 0, 0, 0};
	if (tiles) { for (uint32_t i = 0; i < 6u; ++i) { tot[i] = total[i]; } }
	for (u64 p = (u64)blockIdx.x * 256u + threadIdx.x; p <= n_pair; p += (u64)gridDim.x * 256u) {
		u64 at[3], behind[3];
		counts_in_front(ufirst, n_pair, units, pfirst, tot, ufirst[p], at);
		counts_in_front(ufirst, n_pair, units, pfirst, tot, ufirst[p < n_pair ? p + 1u : n_pair], behind);
		if (patch_first) { patch_first[p] = at[0]; }
		if (delta_first) { delta_first[p] = at[1]; }
		if (p < n_pair) { changed[p] = behind[2] - at[2]; }
		else { count[0] = tot[2]; count[1] = tot[4]; count[2] = tot[3]; count[3] = tot[5]; }
	}
}

void launch_diff_seed(hipStream_t st, const SpliceView& base, const SpliceView& next, uint32_t n_pair, uint32_t nbn, uint32_t shift, const u64* pair, const DiffTab& t, int32_t* status)
{
	hipLaunchKernelGGL(df_seed_kernel, dim3(1), dim3(DV_THREADS), 0, st, SpliceSrc{{base, next}}, n_pair, nbn, shift, pair, t.ufirst, status);
}

void launch_diff_verdicts(hipStream_t st, const SpliceView& base, const SpliceView& next, uint32_t n_pair, uint32_t nbn, uint32_t shift, bool with_crc, const u64* pair,
                          const DiffTab& t, int32_t* status, uint32_t blocks)
{
	hipLaunchKernelGGL(df_verdict_kernel, fixed_grid(nbn, 256u, blocks), dim3(256), 0, st, base, next, n_pair, shift, with_crc ? 1u : 0u, pair, t.ufirst, t.verdict, status);
}

void launch_diff_confirm(hipStream_t st, const SpliceView& base, const SpliceView& next, uint32_t n_pair, uint32_t nbn, uint32_t shift, const u64* pair, const DiffTab& t,
                         const int32_t* status, uint32_t blocks)
{
	const uint32_t ppu_shift = shift > DD_PIECE_SHIFT ? shift - DD_PIECE_SHIFT : 0u;
	hipLaunchKernelGGL(df_confirm_kernel, fixed_grid((u64)nbn << ppu_shift, DD_SLICE_MIN, blocks), dim3(CPD_THREADS), 0, st, base, next, n_pair, ppu_shift, pair, t.ufirst, status, t.verdict);
}

void launch_diff_tilescan(hipStream_t st, uint32_t tiles, u64* tsum)
{
	hipLaunchKernelGGL((rows_tilescan_kernel<6, 2>), dim3(1), dim3(DV_THREADS), 0, st, tiles, tsum);
}

void launch_diff_runs(hipStream_t st, const SpliceView& next, uint32_t n_pair, uint32_t nbn, const u64* pair, const DiffTab& t, const int32_t* status, u64* delta_ext, u64* patch_ext)
{
	const uint32_t tiles = row_tiles(nbn);
	hipLaunchKernelGGL(df_tile_kernel, dim3(tiles), dim3(DV_THREADS), 0, st, next, n_pair, pair, t.ufirst, status, t.verdict, t.tsum);
	launch_diff_tilescan(st, tiles, t.tsum);
	hipLaunchKernelGGL(df_runs_kernel, dim3(tiles), dim3(DV_THREADS), 0, st, n_pair, pair, t.ufirst, status, t.verdict, t.tsum, t.pfirst, delta_ext, patch_ext);
}

void launch_diff_counts(hipStream_t st, uint32_t n_pair, uint32_t nbn, const DiffTab& t, u64* delta_first, u64* patch_first, u64* changed, u64* count, uint32_t blocks)
{
	hipLaunchKernelGGL(df_counts_kernel, fixed_grid((u64)n_pair + 1u, 256u, blocks), dim3(256), 0, st, n_pair, n_pair ? row_tiles(nbn) : 0u, t.ufirst, t.tsum, t.pfirst,
	                   delta_first, patch_first, changed, count);
}

} // namespace msc
