// repair.hip -- the passes of a block deduper made for repair (mscomp_amd_deduper_create_repair / _repair, include/mscomp_amd.h): from the
// verdicts mscomp_amd_blocks_salvage gave for a container (the primary) and for up to three copies of it (the mirrors), the extent list
// that takes every bad row of the primary from the first mirror whose row is good -- what a splicer made for extents over the same views
// turns into a container of the primary's shape. A table-only call: no stored byte is read. The views travel by value in the kernel
// arguments, as a splicer's; the scratch is a DiffTab (ufirst, pfirst, tsum; verdict holds a row's choice), and the tiles' running values
// are diff's instance of the tile scan (launch_diff_tilescan). DESIGN.md 4.19.
#include "rowpass.h"

namespace msc {

#define RP_SRC  3u                                         // choice word of a row: the source it is taken from ...
#define RP_LOST 4u                                         // ... and whether no source has it (always with source 0)

// Seed, one block: per resource of the primary rule 1, the room of rule 2 and the status, and ufirst (n_res + 1): the rows of the
// resources that passed, numbered densely in resource order. The count of resources with a lost row is cleared for the last pass.
__global__ __launch_bounds__(DV_THREADS) void rp_seed_kernel(SpliceView v0, uint32_t n_res, uint32_t nbn, uint32_t shift, u64* __restrict__ ufirst, int32_t* __restrict__ status,
                                                            u64* __restrict__ count)
{
	if (threadIdx.x == 0) { count[3] = 0; }
	seed_numbering<1>(n_res, nbn, 0, ufirst, status, [&](uint32_t r, u64& rows, bool&) {
		u64 f0, L;
		return r < v0.n_res ? view_rows(v0, r, shift, f0, rows, L) : -2;       // (no such resource: no table entry of it is read)
	});
}

// Choice, rule 3: a fixed grid dealt over the rows of the numbering, a row finds its resource by binary search in ufirst. The lowest
// source whose copy of the row is usable; none: the row is lost and stays the primary's.
__global__ __launch_bounds__(256) void rp_choice_kernel(SpliceView v0, SpliceView v1, SpliceView v2, SpliceView v3, const uint32_t* __restrict__ q0,
                                                       const uint32_t* __restrict__ q1, const uint32_t* __restrict__ q2, const uint32_t* __restrict__ q3,
                                                       uint32_t n_src, uint32_t n_res, uint32_t shift, uint32_t with_crc, const u64* __restrict__ ufirst,
                                                       uint32_t* __restrict__ choice)
{
	const u64 units = ufirst[n_res];
	for (u64 u = (u64)blockIdx.x * 256u + threadIdx.x; u < units; u += (u64)gridDim.x * 256u) {
		const uint32_t r = res_of_block(ufirst, n_res, u);
		const u64 k = u - ufirst[r], j0 = v0.first[r] + k, L0 = v0.res_len[r];   // (j0 < v0.nbt: rule 1)
		uint32_t c = RP_LOST;
		if (q0[j0] == SV_GOOD) { c = 0; }
		for (uint32_t s = 1; s < n_src && c == RP_LOST; ++s) {
			const SpliceView v = sp_view(v0, v1, v2, v3, s);
			const uint32_t* __restrict__ q = s == 1u ? q1 : s == 2u ? q2 : q3;
			if (r >= v.n_res) { continue; }
			u64 f0, n, L;
			if (view_rows(v, r, shift, f0, n, L) != 0 || L != L0) { continue; }
			if (q[f0 + k] != SV_GOOD) { continue; }                            // (k < n: equal lengths; f0 + n <= v.nbt)
			if (with_crc && v.crc[f0 + k] != v0.crc[j0]) { continue; }
			c = s;
		}
		choice[u] = c;
	}
}

// What row u of the numbering is to the run passes.
struct RpRow {
	uint32_t p, c;                                                         // resource, source
	u64 k;
	bool live, lost, starts, ends;                                         // starts / ends a run (rule 4)
};
__device__ __forceinline__ RpRow rp_row(uint32_t n_res, const u64* __restrict__ ufirst, const uint32_t* __restrict__ choice, u64 u)
{
	RpRow r = {0, 0, 0, false, false, false, false};
	if (u >= ufirst[n_res]) { return r; }
	r.p = res_of_block(ufirst, n_res, u);
	r.k = u - ufirst[r.p];
	const uint32_t v = choice[u];
	r.live = true; r.c = v & RP_SRC; r.lost = (v & RP_LOST) != 0;
	r.starts = r.k == 0 || (choice[u - 1u] & RP_SRC) != r.c;
	r.ends = u + 1u == ufirst[r.p + 1u] || (choice[u + 1u] & RP_SRC) != r.c;
	return r;
}

// Runs (RunScan), in diff's layout of six sums and two maxima, so that its instance of the tile scan serves: tile g of ROW_TILE rows, eight
// words -- the sums of run starts, fixed rows, lost rows, stored bytes of the fixed rows in their mirrors, rows, and a spare; then the last
// row of the tile that starts a run, + 1 (0: none), and a word diff's scan carries for its own use (0 here).
__global__ __launch_bounds__(DV_THREADS) void rp_tile_kernel(SpliceView v0, SpliceView v1, SpliceView v2, SpliceView v3, uint32_t n_res, const u64* __restrict__ ufirst,
                                                            const uint32_t* __restrict__ choice, u64* __restrict__ tsum)
{
	__shared__ u64 s_w[5][DV_WAVES];
	const u64 u = (u64)blockIdx.x * ROW_TILE + threadIdx.x;
	const RpRow r = rp_row(n_res, ufirst, choice, u);
	u64 bytes = 0;
	if (r.live && r.c) { const SpliceView v = sp_view(v0, v1, v2, v3, r.c); const u64 j = v.first[r.p] + r.k; bytes = v.off[j + 1u] - v.off[j]; }
	u64 a[5] = {r.starts ? 1u : 0u, r.live && r.c ? 1u : 0u, r.lost ? 1u : 0u, bytes, r.live ? 1u : 0u}, sum[5] = {0, 0, 0, 0, 0};
	dv_block_scan<5>(a, sum, s_w);
	u64 m[1] = {r.starts ? u + 1u : 0};
	RunScan<5>::tile<6>(tsum, sum, m, s_w[0]);
}

// The rows again, with the running values in front of the tile: the row that ENDS a run writes its extent, whole -- the run's first row is
// the running maximum of the rows that start one --, and the first row of a resource leaves the three counts in front of it in pfirst.
__global__ __launch_bounds__(DV_THREADS) void rp_runs_kernel(uint32_t n_res, const u64* __restrict__ ufirst, const uint32_t* __restrict__ choice, const u64* __restrict__ tsum,
                                                            u64* __restrict__ pfirst, u64* __restrict__ ext)
{
	__shared__ u64 s_w[3][DV_WAVES];
	const u64 u = (u64)blockIdx.x * ROW_TILE + threadIdx.x;
	const RpRow r = rp_row(n_res, ufirst, choice, u);
	const u64 own[3] = {r.starts ? 1u : 0u, r.live && r.c ? 1u : 0u, r.lost ? 1u : 0u};
	u64 a[3];
	const u64 m0 = RunScan<3>::head<6>(tsum, u, own, a, s_w);
	if (r.live && r.k == 0) { RunScan<3>::front(pfirst + 3u * (u64)r.p, a, own); }
	if (!r.ends) { return; }
	const u64 u0 = m0 - 1u;                                                // the run [u0, u]: a run lies in one resource
	u64* e = ext + 4u * (a[0] - 1u);                                       // (no more runs than rows: inside 4 n_blocks_new)
	e[0] = r.c; e[1] = r.p; e[2] = u0 - ufirst[r.p]; e[3] = u - u0 + 1u;
}

// Counts, one thread per resource and one more (counts_in_front): what lies in front of resource p and of resource p + 1.
__global__ __launch_bounds__(256) void rp_counts_kernel(uint32_t n_res, uint32_t tiles, const u64* __restrict__ ufirst, const u64* __restrict__ tsum, const u64* __restrict__ pfirst,
                                                       u64* __restrict__ ext_first, u64* __restrict__ fixed, u64* __restrict__ lost, u64* count, int32_t* __restrict__ status)
{
	const u64 units = ufirst[n_res];
	const u64* total = tsum + 8u * (u64)(tiles ? tiles - 1u : 0u);
	u64 tot[4] = {0, 0, 0, 0};
	if (tiles) { for (uint32_t i = 0; i < 4u; ++i) { tot[i] = total[i]; } }
	for (u64 p = (u64)blockIdx.x * 256u + threadIdx.x; p <= n_res; p += (u64)gridDim.x * 256u) {
		u64 at[3], behind[3];
		counts_in_front(ufirst, n_res, units, pfirst, tot, ufirst[p], at);
		counts_in_front(ufirst, n_res, units, pfirst, tot, ufirst[p < n_res ? p + 1u : n_res], behind);
		if (ext_first) { ext_first[p] = at[0]; }
		if (p < n_res) {
			const u64 nl = behind[2] - at[2];
			fixed[p] = behind[1] - at[1]; lost[p] = nl;
			if (nl) { status[p] = -3; atomicAdd(reinterpret_cast<unsigned long long*>(count) + 3, 1ull); }   // MSCOMP_DATA_ERROR (an accepted resource: it has rows)
		} else { count[0] = tot[1]; count[1] = tot[2]; count[2] = tot[3]; }
	}
}

void launch_repair_seed(hipStream_t st, const SpliceView& primary, uint32_t n_res, uint32_t nbn, uint32_t shift, const DiffTab& t, int32_t* status, u64* count)
{
	hipLaunchKernelGGL(rp_seed_kernel, dim3(1), dim3(DV_THREADS), 0, st, primary, n_res, nbn, shift, t.ufirst, status, count);
}

void launch_repair_choice(hipStream_t st, const SpliceSrc& src, const uint32_t* const (&verdict)[4], uint32_t n_src, uint32_t n_res, uint32_t nbn, uint32_t shift, bool with_crc,
                          const DiffTab& t, uint32_t blocks)
{
	hipLaunchKernelGGL(rp_choice_kernel, fixed_grid(nbn, 256u, blocks), dim3(256), 0, st, src.v[0], src.v[1], src.v[2], src.v[3], verdict[0], verdict[1], verdict[2], verdict[3],
	                   n_src, n_res, shift, with_crc ? 1u : 0u, t.ufirst, t.verdict);
}

void launch_repair_runs(hipStream_t st, const SpliceSrc& src, uint32_t n_res, uint32_t nbn, const DiffTab& t, u64* ext)
{
	const uint32_t tiles = row_tiles(nbn);
	hipLaunchKernelGGL(rp_tile_kernel, dim3(tiles), dim3(DV_THREADS), 0, st, src.v[0], src.v[1], src.v[2], src.v[3], n_res, t.ufirst, t.verdict, t.tsum);
	launch_diff_tilescan(st, tiles, t.tsum);
	hipLaunchKernelGGL(rp_runs_kernel, dim3(tiles), dim3(DV_THREADS), 0, st, n_res, t.ufirst, t.verdict, t.tsum, t.pfirst, ext);
}

void launch_repair_counts(hipStream_t st, uint32_t n_res, uint32_t nbn, const DiffTab& t, u64* ext_first, u64* fixed, u64* lost, u64* count, int32_t* status, uint32_t blocks)
{
	hipLaunchKernelGGL(rp_counts_kernel, fixed_grid((u64)n_res + 1u, 256u, blocks), dim3(256), 0, st, n_res, n_res ? row_tiles(nbn) : 0u, t.ufirst, t.tsum, t.pfirst,
	                   ext_first, fixed, lost, count, status);
}

} // namespace msc
