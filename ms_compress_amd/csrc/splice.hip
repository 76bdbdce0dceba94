// splice.hip -- the passes of a block splicer (mscomp_amd_splicer_*, include/mscomp_amd.h): a new block container made of picks
// (source, resource) out of up to four source containers. No block is decoded or encoded: the stored form of a block depends only on its
// data, the format and the block size, so the layout pass hands every row of the new table the ADDRESS of its stored bytes and the move
// pass (blocks.hip bk_move_kernel) carries them, back-to-back rows of one source as one copy. The sources travel by value in the kernel
// arguments. DESIGN.md 4.12.
#include "kernels.h"

namespace msc {

// Layout, one block, in the shape of rs_layout_kernel. A pass over the picks in tiles: rules 1 and 2 per pick, a scan of the block counts
// of the picks that passed them -- rule 3 holds it against the table --, then a scan of the counts that stayed, which is new_first; new_len
// and the provisional statuses. A scan over the NEW table rows then gives every row its stored length, checksum and address: a row finds
// its pick by binary search in new_first and is source row first[r] + k of it. Then rule 7 on the picks' last rows.
__global__ __launch_bounds__(DV_THREADS) void sp_layout_kernel(SpliceView v0, SpliceView v1, SpliceView v2, SpliceView v3, uint32_t n_src, uint32_t n_pick, uint32_t nbt, uint32_t shift, u64 cap,
                                                              const u64* __restrict__ pick, u64* new_first, u64* new_off, uint32_t* __restrict__ new_crc,
                                                              u64* __restrict__ new_len, int32_t* status, u64* __restrict__ addr)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const u64 B = (u64)1 << shift;
	u64 run[1] = {0}, rows[1] = {0};
	if (tid == 0) { new_first[0] = 0; new_off[0] = 0; }
	for (uint32_t base = 0; base < n_pick; base += DV_THREADS) {
		const uint32_t p = base + tid;
		const bool live = p < n_pick;
		u64 n = 0, L = 0;
		int32_t st = 0;
		if (live) {
			const u64 s = pick[2u * (u64)p], r = pick[2u * (u64)p + 1u];
			st = -2;                                                        // rule 1: nothing of the pick is read further
			if (s < n_src) {
				const SpliceView v = sp_view(v0, v1, v2, v3, s);
				if (r < v.n_res) {
					const u64 f0 = v.first[r], f1 = v.first[r + 1u];
					if (f0 <= f1 && f1 <= v.nbt) {
						L = v.res_len[r]; n = f1 - f0;
						st = n == (L >> shift) + ((L & (B - 1u)) ? 1u : 0u) ? 0 : -3;   // rule 2
						if (st) { n = 0; L = 0; }
					}
				}
			}
		}
		u64 a[1] = {n};
		dv_block_scan<1>(a, run, s_w);
		if (n && a[0] > nbt) { st = -2; n = 0; L = 0; }                      // rule 3: the total includes this pick and the refused ones
		u64 b[1] = {n};
		dv_block_scan<1>(b, rows, s_w);
		if (live) { new_first[p + 1u] = b[0]; new_len[p] = L; status[p] = st; }
	}
	const u64 nbn = rows[0];                                             // (<= nbt: every pick that stayed passed rule 3)
	__syncthreads();                                                     // new_first is read back below, by other threads of this block
	u64 sum[1] = {0};
	for (uint32_t base = 0; base < nbt; base += DV_THREADS) {
		const uint32_t j = base + tid;
		const bool live = j < nbt;
		u64 len = 0, at = 0;
		uint32_t crc = 0;
		if (live && j < nbn) {
			const uint32_t p = res_of_block(new_first, n_pick, j);
			const SpliceView v = sp_view(v0, v1, v2, v3, pick[2u * (u64)p]);
			const u64 jr = v.first[pick[2u * (u64)p + 1u]] + (j - new_first[p]);   // (< v.nbt: rule 1)
			const u64 o0 = v.off[jr], o1 = v.off[jr + 1u];
			if (o0 <= o1 && o1 <= v.packed_len) { len = o1 - o0; }
			if (new_crc) { crc = v.crc[jr]; }
			if (len) { at = (u64)(uintptr_t)(v.packed + o0); }
		}
		u64 e[1] = {len};
		dv_block_scan<1>(e, sum, s_w);
		if (live) { new_off[j + 1u] = e[0]; addr[j] = e[0] <= cap ? at : 0; if (new_crc) { new_crc[j] = crc; } }
	}
	__syncthreads();                                                     // new_off is read back below
	for (uint32_t p = tid; p < n_pick; p += DV_THREADS) {
		const u64 n0 = new_first[p], n1 = new_first[p + 1u];
		if (n1 > n0 && new_off[n1] > cap) { status[p] = -5; }               // MSCOMP_BUF_ERROR replaces MSCOMP_OK (the offsets only grow: the last block tells)
	}
}

void launch_splice_layout(hipStream_t st, const SpliceSrc& src, uint32_t n_src, uint32_t n_pick, uint32_t nbt, uint32_t shift, u64 cap, const u64* pick,
                          u64* new_first, u64* new_off, uint32_t* new_crc, u64* new_len, int32_t* status, u64* addr)
{
	hipLaunchKernelGGL(sp_layout_kernel, dim3(1), dim3(DV_THREADS), 0, st, src.v[0], src.v[1], src.v[2], src.v[3], n_src, n_pick, nbt, shift, cap, pick, new_first, new_off, new_crc, new_len, status, addr);
}

// ---- splice by block extents (mscomp_amd_splicer_splice_extents) ----
// A new resource is a list of extents (source, resource, first block k0, block count c). The extent pass -- one workgroup, extents are few
// next to rows -- judges them and lays the resources out; the row passes are tiled over a grid of ROW_TILE rows per workgroup, the
// three-launch scan: tile sums, their scan, the rows. The move is bk_move_kernel, as for picks.
//
// The extent column w (n_ext + 1 words) carries every running count of the extent pass, then the extents' first new rows. While the pass
// runs, the word of extent e is w[e + 1], read as two halves: low = the running count of non-empty extents, later of rows (clamped to 32
// bits: anything above n_blocks_table is refused); high = the running count of refused extents. w[e_lo] stays 0, so "the count in front of
// extent e" is w[e] for every e. What rules 1-3 say of an extent is cheap and is computed again in every pass instead of being kept.
// What rules 1-3 say of extent e: its status, its blocks cnt, and def = cnt B - len_e (below B; not 0: the extent ends short). Scalars and
// one exit, so that nothing of it lives in scratch memory.
__device__ __forceinline__ int32_t sx_judge(const SpliceView& v0, const SpliceView& v1, const SpliceView& v2, const SpliceView& v3, uint32_t n_src, uint32_t shift,
                                            const u64* __restrict__ ext, u64 e, u64& cnt, u64& def)
{
	const u64 s = ext[4u * e], r = ext[4u * e + 1u], k0 = ext[4u * e + 2u], c = ext[4u * e + 3u];
	int32_t st = -2;                                                   // rule 1: nothing of the extent is read further
	cnt = 0; def = 0;
	if (s < n_src) {
		const SpliceView v = sp_view(v0, v1, v2, v3, s);
		if (r < v.n_res) {
			const u64 f0 = v.first[r], f1 = v.first[r + 1u];
			// (the bound compared per view: picked by s and used this late, the compiler would fetch it from a table of the four in scratch memory)
			const bool in_table = s == 1u ? f1 <= v1.nbt : s == 2u ? f1 <= v2.nbt : s == 3u ? f1 <= v3.nbt : f1 <= v0.nbt;
			if (f0 <= f1 && in_table) {
				const u64 B = (u64)1 << shift, L = v.res_len[r], n = f1 - f0;
				if (n != (L >> shift) + ((L & (B - 1u)) ? 1u : 0u)) { st = -3; }   // rule 2
				else if (k0 <= n && (c == ~(u64)0 || c <= n - k0)) {       // rule 3: no sum of k0 and c is formed
					st = 0;
					cnt = c == ~(u64)0 ? n - k0 : c;
					if (cnt && k0 + cnt == n) { def = (n << shift) - L; }  // it reaches block n - 1: len_e = L - k0 B
				}
			}
		}
	}
	return st;
}

__global__ __launch_bounds__(DV_THREADS) void sx_extent_kernel(SpliceView v0, SpliceView v1, SpliceView v2, SpliceView v3, uint32_t n_src, uint32_t n_res, uint32_t n_ext, uint32_t nbt,
                                                              uint32_t shift, const u64* __restrict__ ext_first, const u64* __restrict__ ext, u64* new_first,
                                                              u64* new_off, u64* new_len, int32_t* status, u64* w, uint32_t* flag)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	uint32_t* w32 = reinterpret_cast<uint32_t*>(w);
	const u64 TOP = (u64)1 << 63;
	// rule 0: the extent table as a whole
	bool fall = tid == 0 && ext_first[n_res] > n_ext;
	for (uint32_t base = 0; base < n_res; base += DV_THREADS) {
		const uint32_t q = base + tid;
		if (q < n_res && ext_first[q] > ext_first[q + 1u]) { fall = true; }
	}
	const bool refused = __syncthreads_or(fall) != 0;
	if (tid == 0) { flag[0] = refused ? 1u : 0u; new_first[0] = 0; new_off[0] = 0; }
	for (uint32_t base = 0; base < n_res; base += DV_THREADS) {
		const uint32_t q = base + tid;
		if (q < n_res) { status[q] = refused ? -2 : 0; new_len[q] = 0; if (refused) { new_first[q + 1u] = 0; } }
	}
	if (refused) { return; }                                           // (the row passes read the flag and write zeros)
	const u64 e_lo = ext_first[0], n_e = ext_first[n_res];             // the extents in use: e_lo <= e < n_e <= n_ext
	if (tid == 0) { w[e_lo] = 0; }
	// the running count of non-empty extents
	u64 run[1] = {0};
	for (u64 base = e_lo; base < n_e; base += DV_THREADS) {
		const u64 e = base + tid;
		const bool live = e < n_e;
		u64 a[1] = {0};
		if (live) { u64 cnt, def; (void)sx_judge(v0, v1, v2, v3, n_src, shift, ext, e, cnt, def); a[0] = cnt ? 1u : 0u; }
		dv_block_scan<1>(a, run, s_w);
		if (live) { w32[2u * (e + 1u)] = (uint32_t)a[0]; }
	}
	__syncthreads();
	// rules 4 and 5: an extent that ends short with a non-empty one behind it in its resource is refused; the lowest refused extent of a
	// resource -- the one whose running count of refused extents is one above the count in front of the resource -- gives the status. The
	// last non-empty extent of a resource leaves what its last block lacks in new_len, under a mark that the resource has blocks.
	run[0] = 0;
	for (u64 base = e_lo; base < n_e; base += DV_THREADS) {
		const u64 e = base + tid;
		const bool live = e < n_e;
		u64 cnt = 0, def = 0;
		int32_t st = 0;
		uint32_t q = 0;
		bool later = false;
		if (live) {
			st = sx_judge(v0, v1, v2, v3, n_src, shift, ext, e, cnt, def);
			q = res_of_block(ext_first, n_res, e);
			later = w32[2u * ext_first[q + 1u]] > w32[2u * (e + 1u)];
		}
		const bool bad = st != 0 || (def != 0 && later);
		u64 a[1] = {bad ? 1u : 0u};
		dv_block_scan<1>(a, run, s_w);
		if (live) { w32[2u * (e + 1u) + 1u] = (uint32_t)a[0]; }
		__syncthreads();                                               // the count in front of the resource may come from this tile
		if (live) {
			if (bad && (uint32_t)a[0] == w32[2u * ext_first[q] + 1u] + 1u) { status[q] = st ? st : -2; }
			if (cnt && !later) { new_len[q] = def | TOP; }
		}
	}
	__syncthreads();
	// the running count of rows over the extents of the resources that passed rules 1-5
	run[0] = 0;
	for (u64 base = e_lo; base < n_e; base += DV_THREADS) {
		const u64 e = base + tid;
		const bool live = e < n_e;
		u64 a[1] = {0};
		if (live && status[res_of_block(ext_first, n_res, e)] == 0) { u64 def; (void)sx_judge(v0, v1, v2, v3, n_src, shift, ext, e, a[0], def); }
		dv_block_scan<1>(a, run, s_w);
		if (live) { w32[2u * (e + 1u)] = a[0] < 0xFFFFFFFFu ? (uint32_t)a[0] : 0xFFFFFFFFu; }
	}
	__syncthreads();
	// rule 6 per resource: the running count at its end against the table (it only grows: behind the first resource that crosses it every
	// resource with blocks is refused, so an accepted resource's rows start at the count in front of it); new_first, new_len, status
	u64 rows[1] = {0};
	for (uint32_t base = 0; base < n_res; base += DV_THREADS) {
		const uint32_t q = base + tid;
		const bool live = q < n_res;
		u64 n = 0, L = 0;
		if (live) {
			const u64 e0 = ext_first[q], e1 = ext_first[q + 1u], t = new_len[q];
			if (status[q] == 0 && e1 > e0 && (t & TOP)) {
				const uint32_t end = w32[2u * e1];
				if (end > nbt) { status[q] = -2; }
				else { n = end - w32[2u * e0]; L = (n << shift) - (t & ~TOP); }
			}
		}
		u64 b[1] = {n};
		dv_block_scan<1>(b, rows, s_w);
		if (live) { new_first[q + 1u] = b[0]; new_len[q] = L; }
	}
	// the extents' first new rows: the extents of refused resources get none
	const u64 nbn = rows[0];
	for (u64 e = e_lo + tid; e < n_e; e += DV_THREADS) {
		const u64 c = w32[2u * (e + 1u)];
		w[e + 1u] = c < nbn ? c : nbn;
	}
}

// new row j (j < nb'): its stored length, its checksum word and where its stored bytes lie
__device__ __forceinline__ void sx_row(const SpliceView& v0, const SpliceView& v1, const SpliceView& v2, const SpliceView& v3, const u64* __restrict__ ext,
                                       const u64* __restrict__ w, u64 e_lo, u64 n_e, bool with_crc, u64 j, u64& len, u64& at, uint32_t& crc)
{
	const u64 e = e_lo + res_of_block(w + e_lo, (uint32_t)(n_e - e_lo), j);
	const SpliceView v = sp_view(v0, v1, v2, v3, ext[4u * e]);
	const u64 jr = v.first[ext[4u * e + 1u]] + ext[4u * e + 2u] + (j - w[e]);   // (< v.nbt: rules 1 and 3)
	const u64 o0 = v.off[jr], o1 = v.off[jr + 1u];
	if (o0 <= o1 && o1 <= v.packed_len) { len = o1 - o0; }
	if (with_crc) { crc = v.crc[jr]; }
	if (len) { at = (u64)(uintptr_t)(v.packed + o0); }
}

// tile g: the rows' stored lengths (kept in new_off[j + 1] until the row pass), checksums and addresses, and the tile's sum
__global__ __launch_bounds__(DV_THREADS) void sx_tile_kernel(SpliceView v0, SpliceView v1, SpliceView v2, SpliceView v3, uint32_t n_res, uint32_t nbt,
                                                            const u64* __restrict__ ext_first, const u64* __restrict__ ext, const u64* __restrict__ new_first,
                                                            u64* __restrict__ new_off, uint32_t* __restrict__ new_crc, u64* __restrict__ addr,
                                                            const u64* __restrict__ w, u64* __restrict__ tsum, const uint32_t* __restrict__ flag)
{
	__shared__ u64 s_w[1][DV_WAVES];
	if (flag[0]) { return; }                                           // rule 0 (the same in every thread)
	const uint32_t j = blockIdx.x * ROW_TILE + threadIdx.x;
	u64 len = 0, at = 0;
	uint32_t crc = 0;
	if (j < nbt && j < new_first[n_res]) { sx_row(v0, v1, v2, v3, ext, w, ext_first[0], ext_first[n_res], new_crc != nullptr, j, len, at, crc); }
	if (j < nbt) { new_off[j + 1u] = len; addr[j] = at; if (new_crc) { new_crc[j] = crc; } }
	u64 a[1] = {len}, sum[1] = {0};
	dv_block_scan<1>(a, sum, s_w);
	if (threadIdx.x == 0) { tsum[blockIdx.x] = sum[0]; }
}

// the running sum of the tile sums, in place (one workgroup: a tile sum per ROW_TILE rows)
__global__ __launch_bounds__(DV_THREADS) void sx_tilescan_kernel(uint32_t tiles, u64* tsum, const uint32_t* __restrict__ flag)
{
	__shared__ u64 s_w[1][DV_WAVES];
	if (flag[0]) { return; }
	u64 run[1] = {0};
	for (uint32_t base = 0; base < tiles; base += DV_THREADS) {
		const uint32_t g = base + threadIdx.x;
		u64 a[1] = {g < tiles ? tsum[g] : 0};
		dv_block_scan<1>(a, run, s_w);
		if (g < tiles) { tsum[g] = a[0]; }
	}
}

// tile g: new_off from the sum in front of the tile; a row that ends beyond cap is not moved, and when it is the last row of its resource
// that resource gets MSCOMP_BUF_ERROR (the offsets only grow: the last block tells). A refused extent table: zeros.
__global__ __launch_bounds__(DV_THREADS) void sx_rows_kernel(uint32_t n_res, uint32_t nbt, u64 cap, const u64* __restrict__ ext_first, const u64* __restrict__ new_first,
                                                            u64* __restrict__ new_off, uint32_t* __restrict__ new_crc, u64* __restrict__ addr, int32_t* __restrict__ status,
                                                            const u64* __restrict__ w, const u64* __restrict__ tsum, const uint32_t* __restrict__ flag)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t j = blockIdx.x * ROW_TILE + threadIdx.x;
	if (flag[0]) {
		if (j < nbt) { new_off[j + 1u] = 0; if (new_crc) { new_crc[j] = 0; } }
		return;
	}
	u64 a[1] = {j < nbt ? new_off[j + 1u] : 0}, sum[1] = {blockIdx.x ? tsum[blockIdx.x - 1u] : 0};
	dv_block_scan<1>(a, sum, s_w);
	if (j >= nbt) { return; }
	new_off[j + 1u] = a[0];
	if (a[0] > cap && j < new_first[n_res]) {
		addr[j] = 0;
		const u64 e_lo = ext_first[0];
		const u64 e = e_lo + res_of_block(w + e_lo, (uint32_t)(ext_first[n_res] - e_lo), j);
		if (w[e + 1u] == (u64)j + 1u) {                                   // the last row of its extent: of its resource too?
			const uint32_t q = res_of_block(ext_first, n_res, e);
			if (new_first[q + 1u] == (u64)j + 1u) { status[q] = -5; }       // MSCOMP_BUF_ERROR replaces MSCOMP_OK
		}
	}
}

void launch_splice_extents(hipStream_t st, const SpliceSrc& src, uint32_t n_src, uint32_t n_res, uint32_t n_ext, uint32_t nbt, uint32_t shift, const u64* ext_first,
                           const u64* ext, u64* new_first, u64* new_off, u64* new_len, int32_t* status, const SpliceExtTab& t)
{
	hipLaunchKernelGGL(sx_extent_kernel, dim3(1), dim3(DV_THREADS), 0, st, src.v[0], src.v[1], src.v[2], src.v[3], n_src, n_res, n_ext, nbt, shift, ext_first, ext,
	                   new_first, new_off, new_len, status, t.ext_row, t.flag);
}

void launch_splice_tiles(hipStream_t st, const SpliceSrc& src, uint32_t n_res, uint32_t nbt, const u64* ext_first, const u64* ext, const u64* new_first, u64* new_off,
                         uint32_t* new_crc, const SpliceExtTab& t)
{
	hipLaunchKernelGGL(sx_tile_kernel, dim3(row_tiles(nbt)), dim3(DV_THREADS), 0, st, src.v[0], src.v[1], src.v[2], src.v[3], n_res, nbt, ext_first, ext, new_first,
	                   new_off, new_crc, t.addr, t.ext_row, t.tsum, t.flag);
}

void launch_splice_tilescan(hipStream_t st, uint32_t nbt, const SpliceExtTab& t)
{
	hipLaunchKernelGGL(sx_tilescan_kernel, dim3(1), dim3(DV_THREADS), 0, st, row_tiles(nbt), t.tsum, t.flag);
}

void launch_splice_rows(hipStream_t st, uint32_t n_res, uint32_t nbt, u64 cap, const u64* ext_first, const u64* new_first, u64* new_off, uint32_t* new_crc, int32_t* status,
                        const SpliceExtTab& t)
{
	hipLaunchKernelGGL(sx_rows_kernel, dim3(row_tiles(nbt)), dim3(DV_THREADS), 0, st, n_res, nbt, cap, ext_first, new_first, new_off, new_crc, t.addr, status,
	                   t.ext_row, t.tsum, t.flag);
}

} // namespace msc
