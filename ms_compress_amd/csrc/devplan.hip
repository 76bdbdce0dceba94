// devplan.hip -- the tables of a decompress plan built on the device (mscomp_amd_plan_create_decompress_dev / _execute_dev), those of a
// compress plan (mscomp_amd_plan_create_compress_dev) and of a size plan (mscomp_amd_plan_create_size_dev), the device-side layout scans
// (mscomp_amd_layout_dev, mscomp_amd_plan_layout_dev) and compaction from device tables (mscomp_amd_compact_dev). The decoders then run on
// these tables unchanged (DESIGN_DECODERS.md, "Plans with device tables").
#include "kernels.h"

namespace msc {

// SIZING (size plans): out_off is not read (every unit's is 0), out_cap holds the limits (null: 2^64 - 1 for every unit) and there is no
// bound on their sum
template <bool SIZING>
__global__ __launch_bounds__(DV_THREADS) void dv_tables_kernel(int format, uint32_t n, u64 in_max, u64 out_max,
                                                              const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                                              const u64* __restrict__ out_off, const u64* __restrict__ out_cap,
                                                              u64* __restrict__ san, uint32_t* __restrict__ chunk_prefix, u64* __restrict__ tok_prefix,
                                                              uint32_t* __restrict__ reject)
{
	__shared__ u64 s_w[3][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	u64* __restrict__ cand_prefix = tok_prefix + (n + 1u);
	u64 run[2] = {0, 0}, cnt[3] = {0, 0, 0};
	if (tid == 0) { chunk_prefix[0] = 0; tok_prefix[0] = 0; cand_prefix[0] = 0; }
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t i = base + tid;
		const bool live = i < n;
		const u64 len = live ? in_len[i] : 0, cap = !live ? 0 : SIZING && !out_cap ? ~(u64)0 : out_cap[i];
		u64 r[2] = {len, cap};
		dv_block_scan<2>(r, run, s_w);                                   // running totals up to and including unit i
		const bool rej = live && (len > 0xFFFFF000ull || r[0] > in_max || (!SIZING && r[1] > out_max));
		const u64 L = rej ? 0 : len, C = rej ? 0 : cap;                  // a rejected unit is an empty unit without room
		// the counts of a host plan (common.h; plan.hip plan_create_impl): chunks; token slots; Xpress+Huffman candidate slots
		u64 c[3] = {0, 0, 0};
		if (live) {
			if (format == 2) { c[0] = decode_chunks(2, L); }
			else if (format == 3) { c[0] = decode_chunks(3, L); c[1] = token_slots(3, L, C); }
			else { c[0] = decode_chunks(4, L); c[1] = token_slots(4, L, C); c[2] = candidate_slots(L, C); }
			san[i] = rej ? 0 : in_off[i]; san[n + i] = L; san[2u * (size_t)n + i] = rej || SIZING ? 0 : out_off[i]; san[3u * (size_t)n + i] = C;
			reject[i] = rej ? 1u : 0u;
		}
		dv_block_scan<3>(c, cnt, s_w);                                   // inclusive: the prefix entry behind unit i
		if (live) { chunk_prefix[i + 1u] = (uint32_t)c[0]; tok_prefix[i + 1u] = c[1]; cand_prefix[i + 1u] = c[2]; }
	}
}

// The path pass of a dev plan with large units: which units take the optional paths of a host plan, and those paths' tables (kernels.h
// DevPaths). It reads the sanitised rows the table pass has just written, so a rejected unit is an empty unit here too and enters no list.
// Per tile of 1024 units one scan of seven values: the stable compaction of the qualifying unit indices (rank = scanned flag) and the
// prefixes of what each adds. The verdicts that need the whole batch -- a unit too large for the all-CU stage, the stage not paying -- are
// written at the end, as counts of 0. A list that would pass the entries it was reserved for (the creation bounds say it cannot) is off too.
__global__ __launch_bounds__(DV_THREADS) void dv_paths_kernel(int format, uint32_t n, const u64* __restrict__ san, DevPaths dp)
{
	__shared__ u64 s_w[7][DV_WAVES];
	__shared__ unsigned long long s_mx;
	__shared__ uint32_t s_huge;
	const uint32_t tid = threadIdx.x;
	const u64* __restrict__ in_len = san + n;
	const u64* __restrict__ out_cap = san + 3u * (size_t)n;
	const bool xps = dp.xps_unit != nullptr, lzg = dp.lzg_unit != nullptr, scr = dp.scr_prefix != nullptr;
	u64 run[7] = {0, 0, 0, 0, 0, 0, 0}, mx = 0;
	bool huge = false;
	if (tid == 0) { s_mx = 0; s_huge = 0; if (scr) { dp.scr_prefix[0] = 0; } }
	__syncthreads();
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t i = base + tid;
		const bool live = i < n;
		const u64 L = live ? in_len[i] : 0, C = live ? out_cap[i] : 0;
		const bool qx = xps && xps_takes(L), qg = lzg && lzg_takes(C);
		if (lzg && lzg_too_large(C)) { huge = true; }
		if (qg && C > mx) { mx = C; }
		const u64 segs = qx ? xps_segments(L, dp.xps_seg_bytes) : 0, tb = qg ? lzg_token_blocks(format, L, C) : 0, tl = qg ? lzg_tiles(C) : 0, wd = qg ? lzg_words(C) : 0;
		u64 v[7] = {qx ? 1u : 0u, segs, qg ? 1u : 0u, tb, tl, wd, scr ? scratch_slots(L, C) : 0};
		dv_block_scan<7>(v, run, s_w);                                   // inclusive: rank + 1 of a unit taken, the prefix entries behind it
		if (qx && v[0] <= dp.xps_max) { const u64 k = v[0] - 1u; dp.xps_unit[k] = i; dp.xps_seg_prefix[k] = v[1] - segs; }
		if (qg && v[2] <= dp.lzg_max) { const u64 k = v[2] - 1u; dp.lzg_unit[k] = i; dp.lzg_tb_prefix[k] = v[3] - tb; dp.lzg_tile_prefix[k] = v[4] - tl; dp.lzg_word_prefix[k] = v[5] - wd; }
		if (scr && live) { dp.scr_prefix[i + 1u] = v[6]; }
	}
	if (huge) { atomicOr(&s_huge, 1u); }
	if (mx) { atomicMax(&s_mx, (unsigned long long)mx); }
	__syncthreads();
	if (tid != 0) { return; }
	if (xps) {
		const bool on = run[0] <= dp.xps_max && run[1] <= dp.xps_seg_max;
		const uint32_t nb = on ? (uint32_t)run[0] : 0u;
		if (on) { dp.xps_seg_prefix[nb] = run[1]; }
		dp.xps_cnt[0] = nb; dp.xps_cnt[1] = on ? (uint32_t)run[1] : 0u;
	}
	if (lzg) {
		const u64 nb = run[2];
		const bool fits = nb <= dp.lzg_max && run[3] <= dp.lzg_tb_max && run[4] <= dp.lzg_tile_max && run[5] <= dp.lzg_word_max;
		const bool on = nb != 0 && fits && !s_huge && lzg_pays(run[5] - 64u * nb, s_mx);   // (run[5]: sum of capacity + 64)
		if (on) { dp.lzg_tb_prefix[nb] = run[3]; dp.lzg_tile_prefix[nb] = run[4]; dp.lzg_word_prefix[nb] = run[5]; }
		dp.lzg_cnt[0] = on ? (uint32_t)nb : 0u; dp.lzg_cnt[1] = on ? (uint32_t)run[3] : 0u; dp.lzg_cnt[2] = on ? (uint32_t)run[4] : 0u;
	}
}

// The compress form: per unit the checks of a compress dev plan, the sanitised row and the chunk prefix of compress_chunks(format, L) (common.h).
// A rejected unit is an empty unit without room and has no chunks, so that no chunk-gridded kernel visits it.
__global__ __launch_bounds__(DV_THREADS) void dv_ctables_kernel(int format, uint32_t n, u64 in_max, u64 unit_max,
                                                               const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                                               const u64* __restrict__ out_off, const u64* __restrict__ out_cap,
                                                               u64* __restrict__ san, uint32_t* __restrict__ chunk_prefix, uint32_t* __restrict__ reject)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const u64 k = compress_chunk_bytes(format);                      // (read once: the choice stays in two SGPRs over the loop)
	u64 run[1] = {0}, cnt[1] = {0};
	if (tid == 0) { chunk_prefix[0] = 0; }
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t i = base + tid;
		const bool live = i < n;
		const u64 len = live ? in_len[i] : 0;
		u64 r[1] = {len};
		dv_block_scan<1>(r, run, s_w);                                   // running total of in_len up to and including unit i
		const bool rej = live && (len > unit_max || r[0] > in_max);
		const u64 L = rej ? 0 : len;
		u64 c[1] = {(L + k - 1u) / k};                                   // compress_chunks(format, L) (L <= 0xFFFFF000: no overflow)
		if (live) {
			san[i] = rej ? 0 : in_off[i]; san[n + i] = L; san[2u * (size_t)n + i] = rej ? 0 : out_off[i]; san[3u * (size_t)n + i] = rej ? 0 : out_cap[i];
			reject[i] = rej ? 1u : 0u;
		}
		dv_block_scan<1>(c, cnt, s_w);
		if (live) { chunk_prefix[i + 1u] = (uint32_t)c[0]; }             // (at most the plan's chunk bound, < 2^31)
	}
}

__global__ __launch_bounds__(256) void dv_reject_kernel(const uint32_t* __restrict__ reject, uint32_t n, u64* __restrict__ d_out_len, int32_t* __restrict__ d_status)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u < n && reject[u]) { d_status[u] = -2; d_out_len[u] = 0; }   // MSCOMP_ARG_ERROR
}

// The last kernel of a size dev plan: a rejected unit gets MSCOMP_ARG_ERROR with length and need 0; need = length for the others when the
// format's size kernels do not write need themselves (Xpress, Xpress+Huffman: every length test is "does it fit")
__global__ __launch_bounds__(256) void dv_size_finish_kernel(const uint32_t* __restrict__ reject, uint32_t n, u64* __restrict__ d_out_len, u64* __restrict__ d_need,
                                                            int32_t* __restrict__ d_status, int copy_need)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u >= n) { return; }
	if (reject[u]) { d_status[u] = -2; d_out_len[u] = 0; d_need[u] = 0; }
	else if (copy_need) { d_need[u] = d_out_len[u]; }
}

// FORMAT 0: src holds the capacities; 2 / 3 / 4 (LZNT1 / Xpress / Xpress+Huffman): src holds input lengths, and the capacity of each is the
// format's largest output (common.h layout_cap, as mscomp_amd_plan_layout), written to cap_out when that is not null
template <int FORMAT>
__global__ __launch_bounds__(DV_THREADS) void dv_layout_kernel(const u64* __restrict__ src, uint32_t n, u64 align, u64* __restrict__ off, u64* __restrict__ cap_out)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	u64 run[1] = {0};
	if (tid == 0) { off[0] = 0; }
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t i = base + tid;
		const u64 s = i < n ? src[i] : 0;
		const u64 c = layout_cap(FORMAT, s);
		if (FORMAT != 0 && cap_out && i < n) { cap_out[i] = c; }
		const u64 q = c / align + (c % align ? 1u : 0u);
		u64 v[1] = { q > ~(u64)0 / align ? ~(u64)0 : q * align };
		dv_block_scan<1>(v, run, s_w);
		if (i < n) { off[i + 1u] = v[0]; }
	}
}

__global__ __launch_bounds__(256) void dv_zero_kernel(uint32_t* __restrict__ p, uint32_t n)
{
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) { p[i] = 0; }
}

void launch_dev_zero(hipStream_t st, uint32_t* p, uint32_t n)
{
	if (n == 0) { return; }
	const uint32_t grid = (n + 255u) / 256u;
	hipLaunchKernelGGL(dv_zero_kernel, dim3(grid < 1024u ? grid : 1024u), dim3(256), 0, st, p, n);
}

void launch_dev_tables(hipStream_t st, int format, uint32_t n, u64 in_total_max, u64 out_total_max, const u64* in_off, const u64* in_len,
                       const u64* out_off, const u64* out_cap, u64* san, uint32_t* chunk_prefix, u64* tok_prefix, uint32_t* reject)
{
	hipLaunchKernelGGL(dv_tables_kernel<false>, dim3(1), dim3(DV_THREADS), 0, st, format, n, in_total_max, out_total_max, in_off, in_len, out_off, out_cap,
	                   san, chunk_prefix, tok_prefix, reject);
}

void launch_dev_paths(hipStream_t st, int format, uint32_t n, const u64* san, const DevPaths& dp)
{
	hipLaunchKernelGGL(dv_paths_kernel, dim3(1), dim3(DV_THREADS), 0, st, format, n, san, dp);
}

void launch_dev_stables(hipStream_t st, int format, uint32_t n, u64 in_total_max, const u64* in_off, const u64* in_len, const u64* limit,
                        u64* san, uint32_t* chunk_prefix, u64* tok_prefix, uint32_t* reject)
{
	hipLaunchKernelGGL(dv_tables_kernel<true>, dim3(1), dim3(DV_THREADS), 0, st, format, n, in_total_max, ~(u64)0, in_off, in_len, (const u64*)nullptr, limit,
	                   san, chunk_prefix, tok_prefix, reject);
}

void launch_dev_size_finish(hipStream_t st, const uint32_t* reject, uint32_t n, u64* d_out_len, u64* d_need, int32_t* d_status, bool copy_need)
{
	if (n == 0) { return; }
	hipLaunchKernelGGL(dv_size_finish_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, reject, n, d_out_len, d_need, d_status, copy_need ? 1 : 0);
}

void launch_dev_reject(hipStream_t st, const uint32_t* reject, uint32_t n, u64* d_out_len, int32_t* d_status)
{
	if (n == 0) { return; }
	hipLaunchKernelGGL(dv_reject_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, reject, n, d_out_len, d_status);
}

void launch_layout_dev(hipStream_t st, const u64* cap, uint32_t n, u64 align, u64* off)
{
	hipLaunchKernelGGL(dv_layout_kernel<0>, dim3(1), dim3(DV_THREADS), 0, st, cap, n, align ? align : 1u, off, nullptr);
}

void launch_clayout_dev(hipStream_t st, int format, const u64* in_len, uint32_t n, u64 align, u64* off, u64* cap)
{
	align = align ? align : 1u;
	if (format == 2) { hipLaunchKernelGGL(dv_layout_kernel<2>, dim3(1), dim3(DV_THREADS), 0, st, in_len, n, align, off, cap); }
	else if (format == 3) { hipLaunchKernelGGL(dv_layout_kernel<3>, dim3(1), dim3(DV_THREADS), 0, st, in_len, n, align, off, cap); }
	else { hipLaunchKernelGGL(dv_layout_kernel<4>, dim3(1), dim3(DV_THREADS), 0, st, in_len, n, align, off, cap); }
}

void launch_dev_ctables(hipStream_t st, int format, uint32_t n, u64 in_total_max, u64 in_unit_max, const u64* in_off, const u64* in_len,
                        const u64* out_off, const u64* out_cap, u64* san, uint32_t* chunk_prefix, uint32_t* reject)
{
	hipLaunchKernelGGL(dv_ctables_kernel, dim3(1), dim3(DV_THREADS), 0, st, format, n, in_total_max, in_unit_max, in_off, in_len, out_off, out_cap,
	                   san, chunk_prefix, reject);
}

// ---- compaction from device tables (mscomp_amd_compact_dev) ----
// The packed byte range [0, min(off[n], cap)) is cut into equal slices, one per block of a grid that is fixed by the CU count: a block finds
// the unit its slice starts in by binary search in off[] and walks the units from there, so the work follows the bytes moved and one long
// unit is spread over as many blocks as its bytes cover. Per unit piece: a bytewise head up to the destination's next 16-byte boundary, a
// body of 16-byte stores (16-byte loads where the source is aligned alike, loads of alignment 1 otherwise), a bytewise tail. No byte of the
// source outside the piece is read. A unit that ends beyond cap is left out whole, and so is everything behind it.
#define CPD_SLICE_MIN 4096u                              // a slice is a multiple of this (small batches: fewer blocks, whole pieces)

// PTRS (the block container's pack pass, blocks.hip): src_off[u] holds the address of unit u's bytes and src is not used
template <bool PTRS>
__global__ __launch_bounds__(CPD_THREADS) void cpd_copy_kernel(const uint8_t* __restrict__ src, const u64* __restrict__ src_off, const u64* __restrict__ len,
                                                              const u64* __restrict__ off, uint32_t n, u64 cap, uint8_t* __restrict__ dst)
{
	const uint32_t tid = threadIdx.x;
	const u64 total = off[n], range = total < cap ? total : cap;
	u64 per = (range + gridDim.x - 1u) / gridDim.x;
	per = (per + (CPD_SLICE_MIN - 1u)) & ~(u64)(CPD_SLICE_MIN - 1u);
	const u64 lo = (u64)blockIdx.x * per;
	if (lo >= range) { return; }
	const u64 hi = range - lo < per ? range : lo + per;
	uint32_t a = 0, b = n;                                               // the first unit with off[u + 1] > lo (there is one: off[n] > lo)
	while (a < b) { const uint32_t m = a + (b - a) / 2u; if (off[m + 1u] > lo) { b = m; } else { a = m + 1u; } }
	// the table row of the next unit is fetched while this unit's bytes move
	u64 o = off[a], L = len[a], e = off[a + 1u], so = src_off[a];
	for (uint32_t u = a; o < hi; ++u) {
		const bool more = u + 1u < n;
		const u64 nL = more ? len[u + 1u] : 0, ne = more ? off[u + 2u] : 0, nso = more ? src_off[u + 1u] : 0;
		if (L > cap - o) { break; }                                         // (o < hi <= cap) ends beyond cap: not copied, and nothing behind it is below cap
		const u64 d0 = o > lo ? o : lo, d1 = o + L < hi ? o + L : hi;
		if (d0 < d1) { cpd_move<false>(dst + d0, (PTRS ? reinterpret_cast<const uint8_t*>((uintptr_t)so) : src + so) + (d0 - o), d1 - d0, tid); }
		const u64 p0 = o + L > lo ? o + L : lo, p1 = e < hi ? e : hi;      // the padding up to the next unit
		if (p0 < p1) { cpd_move<true>(dst + p0, nullptr, p1 - p0, tid); }
		if (!more) { break; }
		o = e; L = nL; e = ne; so = nso;
	}
}

// blocks of cpd_copy_kernel that are resident on the current device at once: its grid (a block more per CU would wait for a whole round)
uint32_t compact_dev_blocks()
{
	int dev = 0, cus = 0, per_cu = 0;
	if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) { (void)hipGetLastError(); cus = 256; }
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cpd_copy_kernel<false>, (int)CPD_THREADS, 0) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 4; }
	return (uint32_t)cus * (uint32_t)per_cu;
}

void launch_compact_dev(hipStream_t st, uint32_t n, const uint8_t* src, const u64* src_off, const u64* len, u64 align, uint8_t* packed, u64 cap,
                        u64* off, uint32_t blocks)
{
	launch_layout_dev(st, len, n, align, off);
	if (n == 0 || cap == 0) { return; }
	hipLaunchKernelGGL(cpd_copy_kernel<false>, dim3(blocks), dim3(CPD_THREADS), 0, st, src, src_off, len, off, n, cap, packed);
}

// The same copy for units that lie in two buffers: src_ptr[u] = the address of unit u's len[u] bytes, off[0..n] already written (blocks.hip)
void launch_pack_ptrs(hipStream_t st, uint32_t n, const u64* src_ptr, const u64* len, const u64* off, uint8_t* packed, u64 cap, uint32_t blocks)
{
	if (n == 0) { return; }
	hipLaunchKernelGGL(cpd_copy_kernel<true>, dim3(blocks), dim3(CPD_THREADS), 0, st, (const uint8_t*)nullptr, src_ptr, len, off, n, cap, packed);
}

} // namespace msc
