// crc32.hip -- CRC-32 (zlib / PNG / Ethernet: reflected polynomial 0xEDB88320, initial value and final XOR 0xFFFFFFFF) of a batch of units in
// HBM, from device tables: mscomp_amd_plan_create_crc_dev / _execute_crc_dev and the block container's mscomp_amd_blocks_crc / _check
// (include/mscomp_amd.h).
//
// CRC-32 is linear over GF(2): with raw(M) the register after M from an initial value of 0, and |M| in bytes,
//   raw(A || B) = raw(A) * x^(8 |B|)  ^  raw(B)                 (mod P; leading zero bytes leave raw() alone)
//   crc32(M)    = raw(M)  ^  0xFFFFFFFF * x^(8 |M|)  ^  0xFFFFFFFF
// So a unit may be cut anywhere: every part adds raw(part) * x^(8 d), d = the bytes between the part's end and the unit's end, with an atomic
// XOR, in any order, onto a value the table pass has seeded with the last two terms. A register is a polynomial with the coefficient of x^0 in
// bit 31 (zlib's multmodp form), so "a zero byte more" is "times x^8". The algebra and the tables: crcmath.h.
#include "../../include/mscomp_amd.h"
#include "kernels.h"
#include "crcmath.h"

namespace msc {

#define CRC_THREADS 256u

// ---- the table pass ----
// One block walks the units in tiles of 1024: the bounds check of the dev plans (running total of in_len <= in_max; a rejected unit is an
// empty unit: MSCOMP_ARG_ERROR, crc 0, nothing read), cum[0..n] = the running sum of the accepted lengths -- the byte range the main kernel
// cuts into slices --, and off[i] (zero for a rejected unit). in_off / off and status may be null (the block container has checked its resources
// itself and reads its own offsets). The one block does nothing but the two scans: the seeds, which cost products, are crc_seed_kernel's.
__global__ __launch_bounds__(DV_THREADS) void crc_tables_kernel(uint32_t n, u64 in_max, const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                                               u64* __restrict__ off, u64* __restrict__ cum, int32_t* __restrict__ status)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	u64 run[1] = {0}, acc[1] = {0};
	if (tid == 0) { cum[0] = 0; }
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t i = base + tid;
		const bool live = i < n;
		const u64 len = live ? in_len[i] : 0;
		u64 r[1] = {len};
		dv_block_scan<1>(r, run, s_w);                                   // running total up to and including unit i
		const bool rej = live && r[0] > in_max;
		const u64 L = rej ? 0 : len;
		u64 c[1] = {L};
		dv_block_scan<1>(c, acc, s_w);
		if (live) {
			cum[i + 1u] = c[0];
			if (off) { off[i] = rej ? 0 : in_off[i]; }
			if (status) { status[i] = rej ? -2 : 0; }                       // MSCOMP_ARG_ERROR
		}
	}
}

// One thread per unit, behind the table pass: crc[i] = the seed of a unit of cum[i + 1] - cum[i] bytes (0 for an empty or rejected one) and,
// for the container's blocks, fac[i] = x^(8 after[i]): the factor that carries a block's terms on to the end of its resource.
__global__ __launch_bounds__(256) void crc_seed_kernel(uint32_t n, const u64* __restrict__ cum, uint32_t* __restrict__ crc, const u64* __restrict__ after, uint32_t* __restrict__ fac)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) { return; }
	if (crc) { crc[i] = crc_seed(cum[i + 1u] - cum[i]); }
	if (fac) { fac[i] = crc_xpow(after[i] << 3); }
}

// ---- the main kernel ----
// One wave, one part [p, p + len) of a unit: raw(body) and raw(tail) in every lane, the tail being the t < 16 bytes behind the last 16-byte
// boundary (all of a part that holds none). The body is laid out in rows of CRC_ROW bytes that END at that boundary, lane l taking the
// CRC_RUN bytes at 64 l of every row with aligned 16-byte loads; what a first row has in front of p counts as zeros, which a raw register
// does not see. So lane l's last byte is always CRC_RUN (63 - l) bytes short of the body's end, and the lanes combine by one multiplication
// with a constant each. No byte outside the part is read.
__device__ __forceinline__ void crc_part(const uint32_t (*t)[256], const uint32_t (*a)[256], const uint32_t* c, uintptr_t p, u64 len, uint32_t lane,
                                         uint32_t& body, uint32_t& tail, uint32_t& tlen)
{
	const uintptr_t end = p + len, e16 = end & ~(uintptr_t)15u;
	const uintptr_t t0 = e16 > p ? e16 : p;
	tlen = (uint32_t)(end - t0);
	uint32_t tb = 0;
	if (lane < tlen) { tb = *reinterpret_cast<const uint8_t*>(t0 + lane); }   // (in flight while the body runs)
	uint32_t st = 0;
	if (e16 > p) {
		const u64 rows = ((u64)(e16 - p) + (CRC_ROW - 1u)) / CRC_ROW;
		uintptr_t q = e16 - rows * CRC_ROW + (uintptr_t)lane * CRC_RUN;      // (may lie in front of p, and of the buffer: compared, not read)
		{
			const uint4 v0 = crc_load_front(q, p), v1 = crc_load_front(q + 16u, p), v2 = crc_load_front(q + 32u, p), v3 = crc_load_front(q + 48u, p);
			st = crc_step16(t, st, v0); st = crc_step16(t, st, v1); st = crc_step16(t, st, v2); st = crc_step16(t, st, v3);
		}
		for (u64 r = 1; r < rows; ++r) {
			q += CRC_ROW;
			const uint4* __restrict__ s = reinterpret_cast<const uint4*>(q);
			const uint4 v0 = s[0], v1 = s[1], v2 = s[2], v3 = s[3];
			st = a[0][st & 255u] ^ a[1][(st >> 8) & 255u] ^ a[2][(st >> 16) & 255u] ^ a[3][st >> 24];
			st = crc_step16(t, st, v0); st = crc_step16(t, st, v1); st = crc_step16(t, st, v2); st = crc_step16(t, st, v3);
		}
		st = crc_mul(st, c[lane]);
	}
	body = wave_all(st, [](uint32_t a, uint32_t b) { return a ^ b; });
	uint32_t ts = 0;
	for (uint32_t j = 0; j < tlen; ++j) { const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)tb, (int)j); ts = (ts >> 8) ^ t[0][(ts ^ b) & 255u]; }
	tail = ts;
}

// The byte range [0, cum[n]) of the batch is cut into equal slices, one per WAVE of a grid fixed by the CU count (cpd_copy_kernel cuts the
// packed range the same way, per block): a wave finds the unit its slice starts in by binary search in cum[] and walks the units from there.
// Per part of a unit: raw(body) and raw(tail), each times x^(8 distance to the unit's end) -- two lanes take the two products at once --,
// XORed onto crc[u]; and, GROUPS, the same sum times fac[u] onto gcrc[grp[u]]: the unit is a block, the group its resource, fac[u] =
// x^(8 bytes of the resource behind the block), so the resource's CRC costs one product more per part.
template <bool GROUPS>
__global__ __launch_bounds__(CRC_THREADS) void crc_kernel(const uint8_t* __restrict__ base, const u64* __restrict__ off, const u64* __restrict__ cum, uint32_t n,
                                                         uint32_t* __restrict__ crc, const uint32_t* __restrict__ grp, const uint32_t* __restrict__ fac, uint32_t* __restrict__ gcrc)
{
	__shared__ uint32_t s_t[16][256];
	__shared__ uint32_t s_a[4][256];
	__shared__ uint32_t s_c[64];
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	{
		const uint32_t* __restrict__ g = &g_crc_tab.t[0][0];
		uint32_t* s = &s_t[0][0];
		for (uint32_t i = tid; i < 16u * 256u; i += CRC_THREADS) { s[i] = g[i]; }
		for (uint32_t i = tid; i < 4u * 256u; i += CRC_THREADS) { (&s_a[0][0])[i] = (&g_crc_tab.a[0][0])[i]; }
		if (tid < 64u) { s_c[tid] = g_crc_tab.c[tid]; }
	}
	__syncthreads();
	const u64 total = cum[n], nw = (u64)gridDim.x * (CRC_THREADS / 64u), w = (u64)blockIdx.x * (CRC_THREADS / 64u) + (tid >> 6);
	u64 per = total / nw + 1u;                                          // (total < 2^50: the creators refuse larger bounds)
	per = (per + (MSCOMP_AMD_CRC_SLICE_BYTES - 1u)) & ~(u64)(MSCOMP_AMD_CRC_SLICE_BYTES - 1u);
	const u64 lo = w * per;
	if (lo >= total) { return; }
	const u64 hi = total - lo < per ? total : lo + per;
	uint32_t x = 0, y = n;                                               // the first unit with cum[u + 1] > lo (there is one: cum[n] > lo)
	while (x < y) { const uint32_t m = x + (y - x) / 2u; if (cum[m + 1u] > lo) { y = m; } else { x = m + 1u; } }
	for (uint32_t u = x; u < n; ++u) {
		const u64 o = cum[u], e = cum[u + 1u];
		if (o >= hi) { break; }
		const u64 p0 = o > lo ? o : lo, p1 = e < hi ? e : hi;
		if (p0 >= p1) { continue; }                                         // (an empty unit)
		uint32_t body, tail, tlen;
		crc_part(s_t, s_a, s_c, (uintptr_t)(base + off[u] + (p0 - o)), p1 - p0, lane, body, tail, tlen);
		// lane 0: the body, tlen bytes further from the unit's end than lane 1's tail
		uint32_t v = lane == 0 ? body : lane == 1 ? tail : 0u;
		const u64 dist = (e - p1) + (lane == 0 ? tlen : 0u);
		if (v != 0 && dist != 0) { v = crc_mul(v, crc_xpow(dist << 3)); }
		v ^= __shfl_xor(v, 1, 64);
		if (lane == 0 && v != 0) {
			atomicXor(&crc[u], v);
			if (GROUPS) { atomicXor(&gcrc[grp[u]], crc_mul(v, fac[u])); }
		}
	}
}

// ---- resource CRCs from block CRCs (mscomp_amd_res_crc_dev) ----
// crc32(A || B) = crc32(A) x^(8 |B|) ^ crc32(B) ^ (terms of the lengths alone), and along a whole resource those terms cancel: the CRC-32 of
// a resource is the XOR over its blocks j of block_crc[j] x^(8 d_j), d_j = the resource's bytes behind block j (zlib's crc32_combine applied
// along the resource). No data is read.
// One thread per resource: its status by its own two table entries, and the word the blocks are folded into.
__global__ __launch_bounds__(256) void rcrc_seed_kernel(uint32_t n_res, uint32_t nbt, uint32_t shift, const u64* __restrict__ block_first, const u64* __restrict__ res_len,
                                                       uint32_t* __restrict__ res_crc, int32_t* __restrict__ status)
{
	const uint32_t r = blockIdx.x * 256u + threadIdx.x;
	if (r >= n_res) { return; }
	const u64 f0 = block_first[r], f1 = block_first[r + 1u], L = res_len[r];
	int32_t st = 0;
	if (f0 > nbt || f1 > nbt) { st = -2; }                                 // MSCOMP_ARG_ERROR
	else if (f1 - f0 != (L >> shift) + ((L & (((u64)1 << shift) - 1u)) ? 1u : 0u)) { st = -3; }   // MSCOMP_DATA_ERROR
	status[r] = st; res_crc[r] = 0;
}
// A fixed grid dealt over the BLOCKS of the table, so that one resource of a million blocks spreads over every CU. A block finds its
// resource by binary search (res_of_block) and takes part when it lies inside an MSCOMP_OK resource. A wave whose 64 blocks share one
// resource folds them in registers first and issues one atomic.
__global__ __launch_bounds__(256) void rcrc_fold_kernel(uint32_t n_res, uint32_t nbt, uint32_t shift, const u64* __restrict__ block_first, const u64* __restrict__ res_len,
                                                       const uint32_t* __restrict__ block_crc, const int32_t* __restrict__ status, uint32_t* __restrict__ res_crc)
{
	const uint32_t lane = threadIdx.x & 63u;
	const u64 step = (u64)gridDim.x * 256u;
	for (u64 base = (u64)blockIdx.x * 256u + (threadIdx.x & ~63u); base < nbt; base += step) {
		const u64 j = base + lane;
		uint32_t r = 0xFFFFFFFFu, v = 0;
		if (j < nbt) {
			const uint32_t x = res_of_block(block_first, n_res, j);
			const u64 f0 = block_first[x], f1 = block_first[x + 1u];
			if (f0 <= j && j < f1 && status[x] == 0) {
				const u64 L = res_len[x], end = (j - f0 + 1u) << shift;          // (f1 - f0 = ceil(L / B) <= nbt: no overflow)
				r = x; v = block_crc[j];
				if (v != 0 && end < L) { v = crc_mul(v, crc_xpow((L - end) << 3)); }
			}
		}
		const uint32_t r0 = uniform(r);
		if (__ballot(r != r0) == 0) {
			v = wave_all(v, [](uint32_t a, uint32_t b) { return a ^ b; });
			if (lane == 0 && r0 != 0xFFFFFFFFu && v != 0) { atomicXor(&res_crc[r0], v); }
		} else if (r != 0xFFFFFFFFu && v != 0) { atomicXor(&res_crc[r], v); }
	}
}

// The fold along runs of a table (kernels.h launch_crc_fold_runs), one thread per row: crc(A || B) = crc(A) x^(8 |B|) ^ crc(B), applied
// piece by piece from the front -- every step but the last one by the same factor x^(8 B).
__global__ __launch_bounds__(256) void crc_foldruns_kernel(uint32_t n, const u64* __restrict__ n_live, uint32_t shift, const u64* __restrict__ first, const u64* __restrict__ len,
                                                          const uint32_t* __restrict__ crc_in, uint32_t* __restrict__ out)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n || i >= n_live[0]) { return; }
	const u64 f = first[i], L = len[i];
	if (f == ~(u64)0) { return; }
	const u64 B = (u64)1 << shift, m = (L + B - 1u) >> shift;
	const uint32_t xb = crc_xpow(B << 3);
	uint32_t v = 0;
	for (u64 k = 0; k < m; ++k) {
		const uint32_t c = crc_in[f + k];
		if (v != 0) { v = crc_mul(v, k + 1u < m ? xb : crc_xpow((L - (k << shift)) << 3)); }
		v ^= c;
	}
	out[i] = v;
}

// blocks of crc_kernel that are resident on the current device at once, four per CU at most: its grid
uint32_t crc_dev_blocks()
{
	int dev = 0, cus = 0, per_cu = 0;
	if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) { (void)hipGetLastError(); cus = 256; }
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, crc_kernel<true>, (int)CRC_THREADS, 0) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 4; }
	return (uint32_t)cus * (uint32_t)(per_cu < 4 ? per_cu : 4);
}

void launch_crc_tables(hipStream_t st, uint32_t n, u64 in_total_max, const u64* in_off, const u64* in_len, u64* off, u64* cum, int32_t* status)
{
	hipLaunchKernelGGL(crc_tables_kernel, dim3(1), dim3(DV_THREADS), 0, st, n, in_total_max, in_off, in_len, off, cum, status);
}

void launch_crc_seeds(hipStream_t st, uint32_t n, const u64* cum, uint32_t* crc, const u64* after, uint32_t* fac)
{
	if (n == 0 || (!crc && !fac)) { return; }
	hipLaunchKernelGGL(crc_seed_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, cum, crc, after, fac);
}

void launch_crc_units(hipStream_t st, uint32_t n, const uint8_t* base, const u64* off, const u64* cum, uint32_t* crc,
                      const uint32_t* grp, const uint32_t* fac, uint32_t* gcrc, uint32_t blocks)
{
	if (n == 0) { return; }
	if (gcrc) { hipLaunchKernelGGL(crc_kernel<true>, dim3(blocks), dim3(CRC_THREADS), 0, st, base, off, cum, n, crc, grp, fac, gcrc); }
	else { hipLaunchKernelGGL(crc_kernel<false>, dim3(blocks), dim3(CRC_THREADS), 0, st, base, off, cum, n, crc, grp, fac, gcrc); }
}

void launch_res_crc(hipStream_t st, uint32_t n_res, uint32_t nbt, uint32_t shift, const u64* block_first, const u64* res_len, const uint32_t* block_crc,
                    uint32_t* res_crc, int32_t* status, uint32_t blocks)
{
	if (n_res == 0) { return; }
	hipLaunchKernelGGL(rcrc_seed_kernel, dim3((n_res + 255u) / 256u), dim3(256), 0, st, n_res, nbt, shift, block_first, res_len, res_crc, status);
	if (nbt == 0) { return; }
	const uint32_t need = (nbt + 255u) / 256u;
	hipLaunchKernelGGL(rcrc_fold_kernel, dim3(need < blocks ? need : blocks), dim3(256), 0, st, n_res, nbt, shift, block_first, res_len, block_crc, status, res_crc);
}

void launch_crc_fold_runs(hipStream_t st, uint32_t n, const u64* n_live, uint32_t shift, const u64* first, const u64* len, const uint32_t* crc_in, uint32_t* out)
{
	if (n == 0) { return; }
	hipLaunchKernelGGL(crc_foldruns_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, n, n_live, shift, first, len, crc_in, out);
}

} // namespace msc
