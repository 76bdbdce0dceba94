// devplan.hip -- the tables of a decompress plan built on the device (mscomp_amd_plan_create_decompress_dev / _execute_dev), those of a
// compress plan (mscomp_amd_plan_create_compress_dev), and the device-side layout scans (mscomp_amd_layout_dev, mscomp_amd_plan_layout_dev). The decoders then run on these tables unchanged (DESIGN_DECODERS.md, "Plans with
// device tables").
#include "kernels.h"

namespace msc {

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
		const u64 len = live ? in_len[i] : 0, cap = live ? out_cap[i] : 0;
		u64 r[2] = {len, cap};
		dv_block_scan<2>(r, run, s_w);                                   // running totals up to and including unit i
		const bool rej = live && (len > 0xFFFFF000ull || r[0] > in_max || r[1] > out_max);
		const u64 L = rej ? 0 : len, C = rej ? 0 : cap;                  // a rejected unit is an empty unit without room
		// the host formulas of plan_create_impl: chunks_of(format, true, L); token slots; Xpress+Huffman candidate slots
		u64 c[3] = {0, 0, 0};
		if (live) {
			if (format == 2) { c[0] = L ? (L + LZD_SEG - 1u) / LZD_SEG : 1u; }
			else if (format == 3) {
				const u64 by_in = L + C / 32766u + 1u;
				c[0] = 1; c[1] = (C < by_in ? C : by_in) + 64u;
			} else {
				const u64 by_in = 8u * L + C / 32766u + 1u;
				c[0] = L ? (L + XHC_TILE_BYTES - 1u) / XHC_TILE_BYTES : 1u; c[1] = (C < by_in ? C : by_in) + 64u;
				const u64 by_out = C / 65536u + 2u, by_len = L / 260u + 1u, most = by_out < by_len ? by_out : by_len;
				c[2] = most + most / 4u + 2u;
			}
			san[i] = rej ? 0 : in_off[i]; san[n + i] = L; san[2u * (size_t)n + i] = rej ? 0 : out_off[i]; san[3u * (size_t)n + i] = C;
			reject[i] = rej ? 1u : 0u;
		}
		dv_block_scan<3>(c, cnt, s_w);                                   // inclusive: the prefix entry behind unit i
		if (live) { chunk_prefix[i + 1u] = (uint32_t)c[0]; tok_prefix[i + 1u] = c[1]; cand_prefix[i + 1u] = c[2]; }
	}
}

// The compress form: per unit the checks of a compress dev plan, the sanitised row and the chunk prefix of chunks_of(format, false, L) (api.hip).
// A rejected unit is an empty unit without room and has no chunks, so that no chunk-gridded kernel visits it.
__global__ __launch_bounds__(DV_THREADS) void dv_ctables_kernel(int format, uint32_t n, u64 in_max, u64 unit_max,
                                                               const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                                               const u64* __restrict__ out_off, const u64* __restrict__ out_cap,
                                                               u64* __restrict__ san, uint32_t* __restrict__ chunk_prefix, uint32_t* __restrict__ reject)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const u64 k = format == 2 ? 4096u : 65536u;                      // LZNT1: 4 KiB chunks; Xpress, Xpress+Huffman: 64 KiB
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
		u64 c[1] = {(L + k - 1u) / k};                                   // (L <= 0xFFFFF000: no overflow)
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

// FORMAT 0: src holds the capacities; 2 / 3 / 4 (LZNT1 / Xpress / Xpress+Huffman): src holds input lengths, and the capacity of each is the
// format's largest output (api.hip mscomp_amd_plan_layout), written to cap_out when that is not null
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
		const u64 c = FORMAT == 2 ? s + 3u + 2u * ((s + 4095u) / 4096u) + 2u     // + the uncounted End_of_buffer
		            : FORMAT == 3 ? s + 4u + 4u * (s / 32u)
		            : FORMAT == 4 ? s + 34u + 258u + 258u * (s / 65536u) : s;
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
	hipLaunchKernelGGL(dv_tables_kernel, dim3(1), dim3(DV_THREADS), 0, st, format, n, in_total_max, out_total_max, in_off, in_len, out_off, out_cap,
	                   san, chunk_prefix, tok_prefix, reject);
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

} // namespace msc
